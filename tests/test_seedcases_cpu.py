"""The premises of tests/seedcases.py, on the numpy restatement alone
(tests/seedstage_ref.py): each case reaches the edge it is built for.  A case
that silently stopped doing so would leave tests/test_gpu_seed_stages.py green
and blind; it fails here instead.  These are conditions, not measurements."""
import numpy as np
import pytest

import seedcases as SC


def pair_index(ref, a, b):
    return ref["pairs"].index((a, b))


def test_sizes_and_order():
    sizes = [SC.build(n).size for n in SC.NAMES]
    assert sizes == sorted(sizes), "NAMES runs small -> large"
    for n in SC.NAMES:
        c = SC.build(n)
        assert c.V <= 12
        if n not in ("contended_t2q", "epipolar_direct"):  # these two say otherwise
            assert max(c.counts) <= 700
    assert SC.build("epipolar_direct").counts == [606, 606]
    assert SC.build("contended_t2q").counts == [3300, 40]


# ---- 1. tracks12 -----------------------------------------------------------
@pytest.mark.parametrize("name,width", [("tracks12", 32), ("tracks12_wide", 64)])
def test_tracks12(orc, name, width):
    c, ref = SC.build(name), SC.reference(orc, name)
    assert c.counts == [300, 257, 129, 0, 300, 33, 2, 1, 300, 31, 300, 0] and c.desc.shape[1] == width
    if width == 64:
        assert not SC.unpack(c.desc)[:, 486:].any() and SC.unpack(c.desc)[:, :486].any(axis=0).all()
    # jobs that share an output offset (the binary search of the match kernels) and
    # a view's first keypoint (the scan of the triangulation kernel)
    nq = [c.counts[a] for a, _ in ref["pairs"]]
    nt = [c.counts[b] for _, b in ref["pairs"]]
    assert nq.count(0) == 8 and nt.count(0) == 14 and nt[-1] == 0 and {1, 2} <= set(nq) & set(nt)
    # knnMatch needs two train rows: nothing matches into the one-row view, though its descriptor is there
    for p, (a, b) in enumerate(ref["pairs"]):
        if b == 7:
            assert (ref["q2t"][p] < 0).all() and (c.counts[a] == 0 or ref["info"][p]["dist2"][:, 0].min() <= 20)
        if b == 6 and c.counts[a] >= 200:
            assert (ref["q2t"][p] >= 0).sum() >= 1  # ... and into the two-row view something does
    # Ten views have keypoints, so a track holds ten observations at most (a
    # keypoint and one match per pair with another view); tracks12_full has twelve.
    longest = max(len(t) for t in ref["tracks"])
    assert longest == 10
    # a long track's rows mix both tables: t2q for earlier views, q2t for later ones
    assert any(len(t) >= 8 and any(o[0] < t[0][0] for o in t[1:]) and any(o[0] > t[0][0] for o in t[1:])
               for t in ref["tracks"])
    # keypoints of the last view with keypoints have train-side matches only
    last = [t for t in ref["tracks"] if t[0][0] == 10]
    assert len(last) >= 100 and all(o[0] < 10 for t in last for o in t[1:])
    # the epipolar filter decides: some ratio matches fall to it, most stay
    cnt = ref["counts"]
    assert cnt["matches"] < cnt["ratio_matches"] and cnt["matches"] > 0.5 * cnt["ratio_matches"] > 1000


def test_tracks12_full(orc):
    c, ref = SC.build("tracks12_full"), SC.reference(orc, "tracks12_full")
    assert c.counts == [40] * 12
    assert max(len(t) for t in ref["tracks"]) == 12
    t = next(t for t in ref["tracks"] if len(t) == 12 and 0 < t[0][0] < 11)
    assert [o[0] for o in t[1:]] == [v for v in range(12) if v != t[0][0]]  # pair-list order


# ---- 2. ratio_edges --------------------------------------------------------
@pytest.mark.parametrize("name", ["ratio_edges_07", "ratio_edges_08", "ratio_edges_07_wide", "ratio_edges_08_wide"])
def test_ratio_edges(orc, name):
    c, ref = SC.build(name), SC.reference(orc, name)
    info = ref["info"][pair_index(ref, 0, 1)]
    r10 = c.meta["ratio10"]
    assert np.float32(c.options["nn_match_ratio"]) == np.float32(r10 / 10)
    on_false = on_true = 0
    for q, t, d0, d1 in c.meta["planted"]:
        assert info["dist2"][q].tolist() == [d0, d1], "the planted rows are the two nearest"
        assert info["idx2"][q, 0] == t, "of equal rows the lower index wins"
        passed = bool(info["ratio_pass"][q])
        if 10 * d0 == r10 * d1:  # exactly on the bound: never a match
            assert not passed
            on_false += d1 > 0
        elif 10 * d0 < r10 * d1 <= 10 * (d0 + 1):  # the last distance inside it
            assert passed
            on_true += 1
        assert (ref["q2t"][0][q] == t) == passed  # every keypoint lies on its line: the ratio test decides
    assert on_false >= 6 and on_true >= 2
    assert any(d0 == d1 == 0 and info["idx2"][q].tolist() == [t, t + SC.TIE_GAP] for q, t, d0, d1 in c.meta["planted"])
    # popcnt(q) = all bits and none; the largest distance there is
    n = c.meta["nbits"]
    ones, zeros = c.meta["extreme_queries"]
    qd = SC.unpack(c.desc[:c.counts[0]])
    assert qd[ones].all() and not qd[zeros].any()
    far = ref["info"][pair_index(ref, 0, 2)]
    assert far["dist2"][ones].tolist() == [77, n] and far["dist2"][zeros].tolist() == [0, n - 77]
    assert ref["q2t"][pair_index(ref, 0, 2)][[ones, zeros]].tolist() == [1, 0]


def test_ratio_bound_needs_float(orc):
    """what the 0.8 cases are for: in double the product stays above the bound"""
    assert np.float32(0.8) * np.float32(10) == np.float32(8) and float(np.float32(0.8)) * 10.0 > 8.0
    assert np.float32(0.7) * np.float32(10) == np.float32(7) and float(np.float32(0.7)) * 10.0 < 7.0


def test_flann_edges(orc):
    c, ref = SC.build("flann_edges"), SC.reference(orc, "flann_edges")
    assert c.counts[2:] == [1, 0] and c.options["matcher_type"] == SC.FLANN
    p01 = pair_index(ref, 0, 1)
    info = ref["info"][p01]
    seen = set()
    for q, t, d0 in c.meta["planted"]:
        assert info["dist2"][q, 0] == d0 and info["idx2"][q, 0] == t
        assert (ref["q2t"][p01][q] == t) == (d0 < 30)
        seen.add(d0)
    assert {29, 30} <= seen
    assert any(info["dist2"][q].tolist() == [29, 29] and info["idx2"][q, 1] == t + SC.TIE_GAP
               for q, t, d0 in c.meta["planted"])
    # the one-row view: match() needs one train row only
    p02 = pair_index(ref, 0, 2)
    for q, d0 in c.meta["lone"]:
        assert ref["info"][p02]["dist2"][q].tolist() == [d0, -1]
        assert ref["q2t"][p02][q] == (0 if d0 < 30 else -1)
    assert sorted(d for _, d in c.meta["lone"]) == [29, 30]
    # the empty view: nothing matches into it or from it
    for a, b in ((0, 3), (1, 3), (2, 3)):
        assert (ref["q2t"][pair_index(ref, a, b)] < 0).all() and len(ref["t2q"][pair_index(ref, a, b)]) == 0


# ---- 3. contended_t2q ------------------------------------------------------
def test_contended_t2q(orc):
    c, ref = SC.build("contended_t2q"), SC.reference(orc, "contended_t2q")
    q2t, t2q = ref["q2t"][0], ref["t2q"][0]
    assert c.counts[0] > 12 * 256 - 256 and c.meta["groups"][0]["count"] >= 11 * 256 + 1  # 12 blocks of queries
    for g in c.meta["groups"]:
        mine = np.arange(g["first"], g["first"] + g["count"])
        assert (q2t[mine[g["off_line"]:]] == g["row"]).all() and (q2t[mine[:g["off_line"]]] == -1).all()
        assert t2q[g["row"]] == g["first"] + g["off_line"] > 0
    assert (q2t == 5).sum() >= 1000 and {g["row"] for g in c.meta["groups"]} == {0, 5, c.counts[1] - 1}
    assert (t2q >= 0).sum() == 3  # every other slot keeps the "no match" value
    assert len(ref["tracks"]) == ref["counts"]["matches"] + 3


# ---- 4. epipolar_edges -----------------------------------------------------
def test_epipolar_edges(orc):
    want = np.array([0.0, 1.5, 1.5 + 2.0 ** -17, 1.5,
                     1.4999924, 1.5000076], dtype=np.float32)  # a float next to 101.5 is 2^-17 away
    assert want[2] == np.float32(1.5000076) and want[4] < 1.5 < want[2]
    accept = [True, True, False, True, True, False]
    # through match_kernel: erased iff dist > max
    c, ref = SC.build("epipolar_knn"), SC.reference(orc, "epipolar_knn")
    info = ref["info"][0]
    assert info["ratio_pass"].all() and info["idx2"][:, 0].tolist() == list(range(6))
    assert np.array_equal(info["dist"], want) and info["accepted"].tolist() == accept
    assert ref["q2t"][0].tolist() == [t if a else -1 for t, a in enumerate(accept)]
    # through epipolar_match_kernel: kept iff dist <= max
    c, ref = SC.build("epipolar_direct"), SC.reference(orc, "epipolar_direct")
    info = ref["info"][0]
    eq, et = c.meta["edge_queries"], c.meta["edge_trains"]
    for q in eq:
        assert np.array_equal(info["dist"][q, et], want) and info["accepted"][q, et].tolist() == accept
    b = c.meta["block"]
    assert ref["counts"]["matches"] == ref["counts"]["ratio_matches"] == b * b + len(eq) * sum(accept) == 360024
    block_t = np.setdiff1d(np.arange(c.counts[1]), et)
    assert (ref["t2q"][0][block_t] == 0).all() and info["accepted"][:, block_t].sum(axis=0).min() == b
    assert (ref["t2q"][0][et] == np.where(accept, eq[0], -1)).all()


# ---- 5. nan_line -----------------------------------------------------------
def test_nan_line(orc):
    c, ref = SC.build("nan_line_knn"), SC.reference(orc, "nan_line_knn")
    info = ref["info"][pair_index(ref, 0, 1)]
    assert len(info["dist"]) >= 30 and np.isnan(info["dist"]).all()
    assert info["accepted"].all() and (ref["q2t"][0] >= 0).sum() == len(info["dist"])  # FilterMatches keeps them
    assert np.isfinite(ref["points"]).all()
    for a, b in ((0, 2), (1, 2)):  # the ordinary view: finite distances, some kept
        i = ref["info"][pair_index(ref, a, b)]
        assert np.isfinite(i["dist"]).all() and i["accepted"].any()
    c, ref = SC.build("nan_line_direct"), SC.reference(orc, "nan_line_direct")
    info = ref["info"][pair_index(ref, 0, 1)]
    assert info["dist"].shape == (40, 40) and np.isnan(info["dist"]).all()
    assert not info["accepted"].any() and (ref["q2t"][0] < 0).all() and (ref["t2q"][0] < 0).all()
    assert ref["counts"]["matches"] > 0 and np.isfinite(ref["points"]).all()


# ---- 6. half_pixels --------------------------------------------------------
def test_half_pixels(orc):
    c, ref = SC.build("half_pixels"), SC.reference(orc, "half_pixels")
    assert (ref["q2t"][0] == np.arange(c.counts[0])).all()
    off = c.offsets
    raw, used = [], []
    for t in ref["tracks"]:
        for v, k, x, y in t:
            for r, u in ((c.kp["x"][off[v] + k], x), (c.kp["y"][off[v] + k], y)):
                raw.append(float(r))
                used.append(u)
    raw, used = np.array(raw), np.array(used)
    half = raw - np.floor(raw) == 0.5
    assert half.sum() >= 20
    assert ((used == np.floor(raw)) & half).any() and ((used == np.floor(raw) + 1) & half).any()  # both tie directions
    assert (used[half] % 2 == 0).all()  # ... each to the even neighbour
    for v in (0.5, 8191.5, -0.5, -1.5):
        assert v in raw
    assert np.isfinite(ref["points"]).all()


# ---- 7. far_points ---------------------------------------------------------
@pytest.mark.parametrize("name,V", [("far_points2", 2), ("far_points3", 3)])
def test_far_points(orc, name, V):
    c, ref = SC.build(name), SC.reference(orc, name)
    n = c.counts[0]
    assert c.V == V and len(ref["points"]) == V * n and np.isfinite(ref["points"]).all()
    assert all(len(t) == V for t in ref["tracks"])
    z = ref["points"][:n, 2]
    depth = c.meta["depth"]
    assert depth.min() == 1e2 and depth.max() == 1e6
    assert np.all(np.abs(z / depth - 1.0) < 0.06)  # the disparity is rounded to a pixel: 2.097 -> 2 at most
