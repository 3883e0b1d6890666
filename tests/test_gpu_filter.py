"""The patch filter's kernels (csrc/dp_filter.hip: rho, front, visibility,
neighbor) on the crafted sets of tests/filtercases.py: Engine.filter_patches
equals both the oracle (or_filter_patches) and the Python statement
(tests/filter_ref.py) flag for flag.  tests/test_filter_cpu.py asserts, without
a GPU, that each set exercises what it is named for.  Then the device form on
a caller's stream, buffer reuse across calls on one context, determinism under
contention and order independence.  No test builds a densify."""
import numpy as np
import pytest

import densepoints_amd as dp
import filtercases
from filter_ref import first_differences

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    with dp.Engine(device=0) as eng:
        yield eng


def configure(eng, case):
    """the case's options, then its views (the grid layout follows the options
    at dp_set_views), then its pyramid level"""
    eng.set_options(dp.Options(**case.options))
    P0, imgs = case.P0(), case.images()
    eng.set_views([dp.View(P0[v], imgs[v]) for v in range(len(P0))])
    if case.level:
        eng.build_pyramid(case.level + 1)
        eng.set_level(case.level)


def fresh_answer(case):
    with dp.Engine(device=0) as eng:
        configure(eng, case)
        return eng.filter_patches(case.patches, case.passes, case.frac)


@pytest.mark.parametrize("name", list(filtercases.CASES))
def test_case_equals_oracle_and_spec(engine, orc, name):
    """beyond_V (visible bits at or beyond V) is only for a library whose
    kernels mask vis to V: without the mask they index the view table with
    those bits and write through what they read there.  Never run that case
    against such a build; reverting the mask removes the case, it is not a
    demonstration of the fault."""
    case = filtercases.build(name)
    configure(engine, case)
    got = engine.filter_patches(case.patches, case.passes, case.frac)
    want = filtercases.oracle_flags(case, orc)
    assert np.array_equal(got, want), "vs oracle: " + first_differences(got, want, case.patches)
    spec = filtercases.runner(case, orc)()["keep"]
    assert np.array_equal(got, spec), "vs filter_ref: " + first_differences(got, spec, case.patches)


@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_device_form_on_callers_stream(engine, passes):
    """dp_filter_patches_device on device-resident records, a d_keep holding
    0xAA on entry and a non-default stream: every byte is 0 or 1 and equals
    the host form."""
    import torch

    case = filtercases.build("sizes-1025")
    configure(engine, case)
    want = engine.filter_patches(case.patches, passes)
    raw = np.ascontiguousarray(case.patches).view(np.uint8).reshape(-1)
    d_pat = torch.from_numpy(raw.copy()).cuda()
    d_keep = torch.full((len(case.patches),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    engine.filter_patches_device(d_pat.data_ptr(), len(case.patches), d_keep.data_ptr(), passes, stream=st.cuda_stream)
    st.synchronize()
    got = d_keep.cpu().numpy()
    assert np.isin(got, (0, 1)).all()
    assert np.array_equal(got, want), first_differences(got, want, case.patches)
    if passes == 0:
        assert got.all()


def test_reuse_of_context_buffers():
    """One context, views set once: 600 patches (passes 1, where the flags
    depend on the contended cell's winner), then 1, then 600 again, at passes
    1 and 3 -- front, alive and rho buffers reused at a smaller n with nothing
    set in between.  Only then another grid_scale, with the views set again as
    the API requires.  Each answer equals a fresh context's."""
    crowd1, one, crowd3, border5 = (filtercases.build(n) for n in ("crowd-1", "sizes-1", "crowd", "gridscale-border-5"))
    assert all(np.array_equal(crowd1.P, c.P) and crowd1.sizes == c.sizes and not c.options for c in (one, crowd3))
    fresh = {c.name: fresh_answer(c) for c in (crowd1, one, crowd3, border5)}
    with dp.Engine(device=0) as eng:
        configure(eng, crowd1)
        for case in (crowd1, one, crowd1, crowd3, border5):
            if case is border5:
                configure(eng, case)
            got = eng.filter_patches(case.patches, case.passes, case.frac)
            assert np.array_equal(got, fresh[case.name]), case.name + ": " + first_differences(
                got, fresh[case.name], case.patches)


@pytest.mark.parametrize("name", ["ties", "crowd-1", "crowd"])
def test_deterministic_under_ties_and_contention(engine, name):
    case = filtercases.build(name)
    configure(engine, case)
    runs = [engine.filter_patches(case.patches, case.passes, case.frac).tobytes() for _ in range(5)]
    assert len(set(runs)) == 1


def test_order_independent_without_ties(engine):
    """mixed has no equal depths in any cell (premise, test_filter_cpu.py), so
    a permutation of the records permutes the flags."""
    case = filtercases.build("mixed")
    configure(engine, case)
    base = engine.filter_patches(case.patches, case.passes, case.frac)
    perm = np.random.default_rng(9).permutation(len(case.patches))
    got = engine.filter_patches(np.ascontiguousarray(case.patches[perm]), case.passes, case.frac)
    assert np.array_equal(got, base[perm]), first_differences(got, base[perm], case.patches[perm])
