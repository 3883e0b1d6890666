"""The oracle's stages after the detector (or_seeds_from_keypoints, which
or_seeds_run also runs) against the numpy restatement tests/seedstage_ref.py on
every planted case of tests/seedcases.py: the pair list, q2t and t2q of every
pair, the counts, the observation list of every point in DLT row order, and the
points bit for bit.  Everything is integer or fixed-order IEEE arithmetic: no
tolerance anywhere."""
import numpy as np
import pytest

import seedcases as SC
import seedstage_ref as SR


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_stages_equal_the_restatement(orc, name):
    case = SC.build(name)
    ref = SC.reference(orc, name)
    got = SC.oracle(orc, name)
    assert got["pairs"] == ref["pairs"] and len(got["pairs"]) == case.V * (case.V - 1) // 2
    for p, pair in enumerate(ref["pairs"]):
        assert np.array_equal(got["q2t"][p], ref["q2t"][p]), f"pair {pair}: q2t differs"
        assert np.array_equal(got["t2q"][p], ref["t2q"][p]), f"pair {pair}: t2q differs"
    c = got["counts"]
    assert {k: c[k] for k in ref["counts"]} == ref["counts"]
    assert (c["views"], c["keypoints"], c["detected"]) == (case.V, case.size, case.size)
    assert len(got["tracks"]) == len(ref["tracks"])
    for i, (g, r) in enumerate(zip(got["tracks"], ref["tracks"])):
        assert g.tolist() == [[o[0], o[1]] for o in r], f"point {i}: observation lists differ"
    assert np.array_equal(bits(got["points"]), bits(ref["points"]))
    # the planted keypoints and descriptors come back as they went in
    off = case.offsets
    for v in range(case.V):
        assert np.array_equal(bits(got["keypoints"][v]), bits(case.kp[off[v]:off[v + 1]]))
        assert np.array_equal(got["descriptors"][v], case.desc[off[v]:off[v + 1]])


def test_restatement_top2_orders_ties_by_index():
    t = np.zeros((5, 32), dtype=np.uint8)
    t[0, 0] = 1
    q = np.zeros((2, 32), dtype=np.uint8)
    q[1, 0] = 3
    idx, dist = SR.top2(q, t)
    assert idx.tolist() == [[1, 2], [0, 1]] and dist.tolist() == [[0, 0], [1, 2]]
    idx, dist = SR.top2(q, t[:1])
    assert idx.tolist() == [[0, -1], [0, -1]] and dist.tolist() == [[1, -1], [1, -1]]
    assert SR.top2(q, t[:0])[0].tolist() == [[-1, -1], [-1, -1]]


def test_restatement_distance_is_the_oracles(orc):
    """or_epipolar_distance (pinned in tests/test_seeds_cpu.py) on random and
    degenerate lines, bit for bit, NaN for NaN"""
    rng = np.random.default_rng(3)
    Fs = [orc.fundamental_matrix(P1, P2) for P1, P2 in
          [(SC.horizontal_rig(2)[0], SC.horizontal_rig(2)[1]), (SC.ring_rig(5)[0], SC.ring_rig(5)[2]),
           (SC.build("nan_line_knn").P[0], SC.build("nan_line_knn").P[1])]]
    for F in Fs:
        xy = rng.uniform(-50, 1500, size=(200, 4)).astype(np.float32)
        xy[:50] = np.rint(xy[:50]) + np.float32(0.5)
        got = SR.epipolar_distance(F, xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3])
        want = np.array([orc.epipolar_distance(F, *map(float, r)) for r in xy], dtype=np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
