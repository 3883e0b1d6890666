"""PMVS-style patch filter: the oracle's C restatement
(oracle/oracle.c or_filter_patches) against an independent pure-Python
statement of the spec in include/densepoints.h (dp_filter_patches), on the
golden densify output and on variants with planted occluders.  There is no
reference implementation (pmvs.h:27 is undefined, modules/filtering empty):
the spec is pinned by these two statements only ("parity unpinned" vs any
reference binary)."""
import os

import numpy as np
import pytest

import filtercases
from filter_ref import filter_spec, first_differences, with_occluders

GOLD = os.path.join(os.path.dirname(__file__), "golden", "pmvs_small.npz")


@pytest.fixture(scope="module")
def gold(orc):
    d = np.load(GOLD)
    P = d["P"]
    imgs = [d["images"][i] for i in range(len(P))]
    xr = [orc.view_geometry(P[v])[4] for v in range(len(P))]
    return P, imgs, xr, d["densify"]


@pytest.mark.parametrize("passes", [1, 2, 3])
@pytest.mark.parametrize("occl", [False, True])
def test_oracle_filter_equals_python_spec(orc, gold, passes, occl):
    P, imgs, xr, pat = gold
    if occl:
        pat = with_occluders(orc, P, pat)
    S = orc.Scene(P, imgs)
    got = S.filter_patches(pat, passes)
    want = filter_spec(P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], xr, pat, passes)
    assert np.array_equal(got, want)
    if occl and passes & 1:
        # planted occluders remove at least some of the occluded originals
        assert got[:25].sum() < 25


def test_filter_monotone_and_edge_cases(orc, gold):
    P, imgs, xr, pat = gold
    S = orc.Scene(P, imgs)
    k1 = S.filter_patches(pat, 1)
    k3 = S.filter_patches(pat, 3)
    assert (k3 <= k1).all()
    assert S.filter_patches(pat, 0).all()
    assert len(S.filter_patches(pat[:0], 3)) == 0
    one = S.filter_patches(pat[:1], 3)  # a lone patch has no occluder and no neighbour set
    assert one[0] == 1


@pytest.mark.parametrize("name", list(filtercases.CASES))
def test_case_oracle_equals_spec_and_premise_holds(orc, name):
    """Every crafted set of tests/filtercases.py: or_filter_patches equals the
    Python statement flag for flag, and the set exercises what it is named for
    (its premise, asserted on the spec's own intermediate results).  This is
    what pins the spec for these sets, the rule that visible bits at or beyond
    V are ignored (beyond_V) included."""
    case = filtercases.build(name)
    run = filtercases.runner(case, orc)
    want = run()["keep"]
    got = filtercases.oracle_flags(case, orc)
    assert np.array_equal(got, want), first_differences(got, want, case.patches)
    case.premise(case, run)
