"""The stages of seed generation after the detector on planted keypoints
(tests/seedcases.py) through dp_probe_seed_stages, which runs
dp_generate_seeds' own code from the per-view offsets to the read-back: the
pair and job plan, the multi-job kNN, match_kernel, epipolar_match_kernel, the
t2q table under contention and triang_kernel, against the oracle's
or_seeds_from_keypoints (itself held to the numpy restatement by
tests/test_seedstage_cpu.py).  q2t and t2q of every pair, the four counts and
the points bit for bit: integers and fixed-order fp64, no tolerance."""
import ctypes
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import matcher as M

import seedcases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = np.full((8, 8, 3), 128, dtype=np.uint8)  # the probe never reads a pixel


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_case(eng, orc, name):
    c, r = SC.build(name), SC.oracle(orc, name)
    eng.set_views([dp.View(c.P[v], BLANK) for v in range(c.V)])
    m = M.Matcher(eng, M.MatcherOptions(**c.options))
    pts = m.probe_stages(c.counts, c.kp, c.desc)
    assert len(r["pairs"]) == c.V * (c.V - 1) // 2
    for p, (a, b) in enumerate(r["pairs"]):
        fa, fb, q2t = m.matches(p)
        assert (fa, fb) == (a, b)
        assert np.array_equal(q2t, r["q2t"][p]), f"{name}: q2t of pair {(a, b)} differs"
        assert np.array_equal(m.t2q(p), r["t2q"][p]), f"{name}: t2q of pair {(a, b)} differs"
    st, oc = m.stats, r["counts"]
    assert (st["pairs"], st["ratio_matches"], st["matches"], st["points"]) == \
        (oc["pairs"], oc["ratio_matches"], oc["matches"], oc["points"]), (name, st, oc)
    assert st["keypoints"] == st["keypoints_detected"] == c.size
    assert np.array_equal(bits(pts), bits(r["points"])), f"{name}: points differ"
    off = c.offsets
    for v in range(c.V):  # the planted rows are what the accessors hand back
        kp, d = m.keypoints(v)
        assert np.array_equal(bits(kp), bits(c.kp[off[v]:off[v + 1]])) and np.array_equal(d, c.desc[off[v]:off[v + 1]])
    return m


@pytest.mark.parametrize("name", SC.NAMES)
def test_stages_match_oracle(orc, name):
    with dp.Engine() as eng:
        run_case(eng, orc, name)


def test_one_context_small_to_large_and_back(orc):
    """kp, desc and the stage buffers only grow and are reused: a run must not
    see what a larger or a wider (64-byte) run left in them"""
    with dp.Engine() as eng:
        for name in SC.NAMES + SC.NAMES[::-1]:
            run_case(eng, orc, name)


def test_probe_leaves_nothing_stale_for_generate_seeds(orc):
    """dp_generate_seeds after probe runs on the same context (more views,
    64-byte rows, direct epipolar matching) still gives the golden fixture,
    and a probe run after it the oracle's result"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "seeds_small.npz"))
    import importlib.util

    spec = importlib.util.spec_from_file_location("mgs", os.path.join(ROOT, "tests", "golden", "make_golden_seeds.py"))
    mgs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mgs)
    with dp.Engine() as eng:
        for name in ("tracks12_wide", "epipolar_direct"):
            run_case(eng, orc, name)
        eng.set_views([dp.View(g["P"][v], g["images"][v]) for v in range(3)])
        m = M.Matcher(eng, M.MatcherOptions(**mgs.OPTIONS))
        pts = m.generate_seeds()
        kps = np.concatenate([m.keypoints(v)[0] for v in range(3)])
        desc = np.concatenate([m.keypoints(v)[1] for v in range(3)])
        q2t = np.concatenate([m.matches(p)[2] for p in range(3)])
        assert np.array_equal(bits(kps), bits(g["keypoints"]))
        assert np.array_equal(desc, g["descriptors"])
        assert np.array_equal(q2t, g["q2t"])
        assert np.array_equal(bits(pts), bits(g["points"]))
        run_case(eng, orc, "tracks12_full")


def _probe(eng, counts, kp, desc, width, n_views=None, out=True, mo=None):
    cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
    xyz, n = ctypes.c_void_p(), ctypes.c_int64()
    return N.lib.dp_probe_seed_stages(eng.handle, len(cnt) if n_views is None else n_views, N.ptr(cnt), N.ptr(kp),
                                      N.ptr(desc), width, mo, ctypes.byref(xyz) if out else None,
                                      ctypes.byref(n) if out else None, None)


def test_bad_arguments_fail_loudly(orc):
    c = SC.build("half_pixels")
    with dp.Engine() as eng:
        assert _probe(eng, c.counts, c.kp, c.desc, 32) == N.DP_E_STATE  # no views set
        eng.set_views([dp.View(c.P[v], BLANK) for v in range(c.V)])
        bad = [
            _probe(eng, c.counts, c.kp, c.desc, 32, out=False),            # null outputs
            _probe(eng, None, c.kp, c.desc, 32, n_views=2),                # null counts
            _probe(eng, c.counts, None, c.desc, 32),                       # null keypoints
            _probe(eng, c.counts, c.kp, None, 32),                         # null descriptors
            _probe(eng, c.counts, c.kp, c.desc, 16),                       # width
            _probe(eng, c.counts, c.kp, c.desc, 48),
            _probe(eng, c.counts, c.kp, c.desc, 0),
            _probe(eng, [c.counts[0], -1], c.kp, c.desc, 32),              # negative count
            _probe(eng, c.counts + [0], c.kp, c.desc, 32),                 # counts for three views
            _probe(eng, c.counts[:1], c.kp, c.desc, 32),                   # ... for one
        ]
        assert bad == [N.DP_E_ARG] * len(bad)
        assert N.lib.dp_last_error(eng.handle).decode().startswith("dp_probe_seed_stages:")
        # more rows in a view than a kNN key's row field holds: 2^22 at 32 bytes, 2^21 at 64
        for width, rows in ((32, 1 << 22), (64, 1 << 21)):
            kp = np.zeros(rows, dtype=N.KEYPOINT_DTYPE)
            desc = np.zeros((rows, width), dtype=np.uint8)
            assert _probe(eng, [0, rows], kp, desc, width) == N.DP_E_ARG
            assert "keypoints in one view" in N.lib.dp_last_error(eng.handle).decode()
        mo = M.MatcherOptions(nn_match_ratio=float("nan")).to_c()
        assert _probe(eng, c.counts, c.kp, c.desc, 32, mo=ctypes.byref(mo)) == N.DP_E_ARG
        # a failed call leaves no result behind, and the context still works
        with pytest.raises(dp.DensePointsError):
            M.Matcher(eng).t2q(0)
        run_case(eng, orc, "half_pixels")
        # no keypoints at all is a valid, empty run
        m = M.Matcher(eng)
        pts = m.probe_stages([0, 0], c.kp[:0], c.desc[:0])
        assert len(pts) == 0 and m.stats["pairs"] == 1 and m.stats["matches"] == 0 and len(m.t2q(0)) == 0
        with pytest.raises(dp.DensePointsError):
            m.t2q(1)
