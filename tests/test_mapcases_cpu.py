"""The premises of tests/mapcases.py, on the numpy references alone: what makes
tests/test_gpu_mixed_sizes.py able to fail.  A kernel that read a width, a
pitch or a plane offset of the wrong view is only caught where views of
different sizes really meet: a box clipped at a small view's edge, a window
void by the source's own bound, a projection that one view's bounds admit and
the other's refuse, a voxel that one view sees and another does not."""
import copy

import numpy as np
import pytest

import fuse_ref as FR
import mapcases as MC
import mapref_ref as MR
import tsdf_ref as TR


@pytest.fixture(scope="module")
def mixed(orc):
    return MC.build("mixed"), MC.chain(orc, "mixed")


@pytest.fixture(scope="module")
def tiny(orc):
    return MC.build("tiny"), MC.chain(orc, "tiny")


def pixels(sizes):
    return [w * h for w, h in sizes]


def projections(vw, s, X):
    """(in front, xi, yi) of the points X in view s, before any bounds test
    (steps 1-3 of dp_fuse_maps' observe)"""
    P = vw.P[s]
    with np.errstate(all="ignore"):
        d = FR.row(P, 2, X)
        ok = d > 0.0
        u, v = FR.row(P, 0, X) / d, FR.row(P, 1, X) / d
        ok &= (np.abs(u) < 2e9) & (np.abs(v) < 2e9)
        xi = np.where(ok, np.rint(u), -1.0).astype(np.int64)
        yi = np.where(ok, np.rint(v), -1.0).astype(np.int64)
    return ok, xi, yi


def inside(xi, yi, size):
    return (xi >= 0) & (xi < size[0]) & (yi >= 0) & (yi < size[1])


def test_scenes_are_what_they_are_named_for(orc):
    for name, sizes in (("mixed", MC.MIXED_SIZES), ("tiny", MC.TINY_SIZES)):
        sc = MC.build(name)
        assert sc.sizes == sizes and [(v.width, v.height) for v in sc.views] == sizes
        assert len(set(sizes)) == sc.V == 5
        assert len(sc.seeds) > 100
        assert (np.einsum("vj,nj->nv", sc.P[:, 2, :3], sc.seeds) + sc.P[:, 2, 3] > 0).all()
    assert [MC.gray_pitch(w) for w, _ in MC.MIXED_SIZES] == [128, 128, 192, 64, 64]
    assert 15 * 13 < 256 and 33 < 64 and (33 - 1) % 16 == 0 and (17 - 1) % 16 == 0
    # level 1 of the odd sizes: all different again, none the half of another's level 0
    l1 = MC.build("mixed").level_sizes(orc, 1)
    assert l1 == [(48, 36), (35, 25), (66, 34), (17, 9), (8, 7)]


def test_render_every_view_is_covered_and_a_small_views_edge_clips(mixed):
    sc, ch = mixed
    rd = ch["render"]
    covered = [int((i >= 0).sum()) for i in rd["index"]]
    print("covered pixels per view:", covered, "of", pixels(sc.sizes))
    assert all(c > 0 for c in covered)
    largest = int(np.argmax(pixels(sc.sizes)))
    assert largest == 2
    # B >= 2, so a centre within 3 pixels of the last column (row) has its box cut there
    cut = {}
    for p in rd["pairs"]:
        W, H = sc.sizes[p["view"]]
        if p["clipped"] and ((p["cu"] > W - 3 and p["x1"] == W - 1) or (p["cv"] > H - 3 and p["y1"] == H - 1)):
            cut[p["view"]] = cut.get(p["view"], 0) + 1
    print("pairs cut at the right or bottom edge, per view:", cut)
    assert any(v != largest for v in cut)
    assert 3 in cut or 4 in cut  # one of the two views smaller than a block


def test_refine_mixed_every_view_keeps_moves_and_fills(mixed):
    sc, ch = mixed
    rd, rf = ch["render"], ch["refine"]
    for k in range(sc.V):
        own = FR.is_depth(rd["depth"][k])
        c = rf["choice"][k]
        kept, moved, filled = int((c >= 0).sum()), int((c > 0).sum()), int(((c >= 0) & ~own).sum())
        print("view %d: kept %d moved %d filled %d" % (k, kept, moved, filled))
        assert kept > 0 and moved > 0 and filled > 0
    st = rf["stats"]
    assert st["kept"] == sum(int((c >= 0).sum()) for c in rf["choice"])
    # every size differs, so every valid source of a pixel is a view of another size
    src = MR.default_sources(ch["mvw"], list(range(sc.V)), 4)
    for k in range(sc.V):
        assert all(sc.sizes[s] != sc.sizes[k] for s in src[k])
        assert (rf["valid"][k] > 0).any()
    # the smallest and the largest view score against each other
    assert 4 in src[2] and 2 in src[4]


def one_source(vw, r, s, depth, normal, **kw):
    """candidate 0 of view r against source s alone: the `valid` plane (1 valid, 0
    void in s, -1 void by its plane)"""
    return MR.refine(vw, [depth], [normal], views=[r], sources=[[s]], sweep=0, reach=(0, 0), max_sources=1, top_k=1,
                     **kw)["valid"][0]


def test_refine_mixed_a_window_is_void_by_the_sources_own_bound(mixed):
    """pixels of the largest view whose window leaves the smallest view at its
    right or bottom bound, 32 (W_s - 1) or 32 (H_s - 1), although it is below the
    same bound taken from the reference view: with the source's W and H replaced
    by the reference's (its gray plane padded to match) they are valid"""
    sc, ch = mixed
    rd, vw = ch["render"], ch["mvw"]
    found = 0
    for r, s in ((2, 4), (0, 3), (2, 1)):
        assert sc.sizes[s][0] < sc.sizes[r][0]
        true = one_source(vw, r, s, rd["depth"][r], rd["normal"][r])
        alt = copy.copy(vw)
        alt.W, alt.H, alt.gray = list(vw.W), list(vw.H), list(vw.gray)
        alt.W[s], alt.H[s] = max(vw.W[r], vw.W[s]), max(vw.H[r], vw.H[s])
        alt.gray[s] = np.pad(vw.gray[s], ((0, alt.H[s] - vw.H[s]), (0, alt.W[s] - vw.W[s])), mode="edge")
        wide = one_source(alt, r, s, rd["depth"][r], rd["normal"][r])
        only_bound = int(((true == 0) & (wide == 1)).sum())
        print("reference %d, source %d: %d pixels void by the source's upper bound alone" % (r, s, only_bound))
        assert not ((true == 1) & (wide != 1)).any()
        found += only_bound > 0
    assert found == 3


def test_refine_fewer_sources_than_top_k_is_void_not_an_error(mixed):
    """the header: "With fewer than top_k valid sources the candidate is void."
    Two requested views leave one source; the reference used to index its second
    score and raise."""
    sc, ch = mixed
    views = [0, 4]
    rd = ch["render"]
    out = MR.refine(ch["mvw"], MC.pick(rd["depth"], views), MC.pick(rd["normal"], views), views=views)
    assert out["stats"]["source_scores"] > 0 and out["stats"]["candidates"] == 0 and out["stats"]["kept"] == 0
    assert all((c == -1).all() for c in out["choice"])


TINY_VIEWS = (2, 3, 4)  # 17 x 1, 1 x 19, 5 x 3


def test_refine_tiny_no_window_of_11_fits_a_single_row_or_column(tiny):
    """A window corner must lie in [0, 32 (W - 1)] x [0, 32 (H - 1)] of the source:
    in a view of one row or one column that is a segment, which an 11 x 11
    window of any other view never fits.  In the 5 x 3 view the bound is 128 x 64
    thirty-seconds: the 10-pixel window of the 16 x 16 view and of the smaller
    views spans more than its 2 rows and never fits; the 10 pixels of the 70 x 50
    view span 10 * 5 / 70 = 0.7 of its pixels and do fit, so that view alone
    scores against it."""
    sc, ch = tiny
    rd, vw = ch["render"], ch["mvw"]
    scored = {}
    for r in range(sc.V):
        for s in TINY_VIEWS:
            if s == r:
                continue
            st = MR.refine(vw, [rd["depth"][r]], [rd["normal"][r]], views=[r], sources=[[s]], window=11, max_sources=1,
                           top_k=1)["stats"]
            assert st["depth_pixels_in"] > 0
            scored[(r, s)] = st["source_scores"]
    print("source scores at window 11, (reference, source):", scored)
    for (r, s), n in scored.items():
        if s in (2, 3) or r != 0:
            assert n == 0, (r, s)
    assert scored[(0, 4)] > 0
    # with the default sources, nothing is kept in a view that is itself too small
    rf = MR.refine(vw, rd["depth"], rd["normal"], window=11)
    for k in TINY_VIEWS:
        assert (rf["choice"][k] == -1).all()
    assert (rf["choice"][0] >= 0).any()


def test_refine_tiny_keep_unscored_passes_their_pixels_through(tiny):
    sc, ch = tiny
    rd, vw = ch["render"], ch["mvw"]
    rf = MR.refine(vw, rd["depth"], rd["normal"], window=11, flags=MR.KEEP_UNSCORED)
    for k in TINY_VIEWS:
        own = FR.is_depth(rd["depth"][k])
        c = rf["choice"][k]
        print("view %d (%d x %d): %d depth pixels, %d come out with choice -2" % ((k,) + sc.sizes[k] + (
            int(own.sum()), int((c == -2).sum()))))
        # (a pixel of a small view may itself score against the 70 x 50 view: its window is clamped, not void)
        assert own.any() and (c == -2).any() and ((c == -2) == (own & (rf["ncand"][k] == 0))).all()
        assert MR.same_bytes(rf["depth"][k][c == -2], rd["depth"][k][c == -2])
    assert (rf["choice"][0] >= 0).any() and (rf["choice"][0] == -2).any()


def test_fuse_mixed_every_pair_matches_and_the_bounds_differ(mixed):
    sc, ch = mixed
    vw, maps = ch["fvw"], ch["maps"]
    assert maps is ch["refine"]
    matched = np.zeros((sc.V, sc.V), np.int64)
    s_refuses, r_refuses = [], []
    for r in range(sc.V):
        ys, xs = np.nonzero(FR.is_depth(maps["depth"][r]))
        X = FR.backproject(vw, r, xs, ys, maps["depth"][r][ys, xs])
        for s in range(sc.V):
            if s == r:
                continue
            matched[r, s] = int(FR.observe(vw, s, X, maps["depth"][s], 0.01)[0].sum())
            ok, xi, yi = projections(vw, s, X)
            in_s, in_r = inside(xi, yi, sc.sizes[s]), inside(xi, yi, sc.sizes[r])
            if (ok & ~in_s & in_r).any():
                s_refuses.append((r, s))
            if (ok & in_s & ~in_r).any():
                r_refuses.append((r, s))
    print("matched pairs, [pixel's view][observing view]:\n", matched)
    assert (matched[~np.eye(sc.V, dtype=bool)] > 0).all()
    assert matched.sum() == ch["fuse"]["stats"]["matched_pairs"]
    print("outside s, inside r's bounds:", s_refuses, "\ninside s, outside r's bounds:", r_refuses)
    assert s_refuses and set(r_refuses) - {s_refuses[0]}
    st = ch["fuse"]["stats"]
    loose = FR.fuse(vw, maps["depth"], maps["normal"], flags=FR.NO_SUPPRESS)["stats"]
    print("fusion:", st, "without suppression:", loose["emitted"])
    assert st["emitted"] > 0 and loose["emitted"] > st["emitted"]
    assert len(set(ch["fuse"]["points"]["view"].tolist())) >= 3


def test_fuse_tiny_every_depth_pixel_emits_at_min_views_0(tiny):
    sc, ch = tiny
    maps = ch["maps"]
    assert maps is ch["render"]
    depth_pixels = [int(FR.is_depth(d).sum()) for d in maps["depth"]]
    out = FR.fuse(ch["fvw"], maps["depth"], maps["normal"], min_views=0)
    per_view = np.bincount(out["points"]["view"], minlength=sc.V)
    print("depth pixels per view:", depth_pixels, "emitted at min_views = 0:", per_view.tolist())
    # every depth pixel is fusable; the suppression takes those an earlier view's pixel agrees with
    assert out["stats"]["fusable"] == sum(depth_pixels) and (per_view > 0).all()
    assert 0 < out["stats"]["emitted"] < out["stats"]["fusable"]
    loose = FR.fuse(ch["fvw"], maps["depth"], maps["normal"], min_views=0, flags=FR.NO_SUPPRESS)
    assert np.bincount(loose["points"]["view"], minlength=sc.V).tolist() == depth_pixels
    assert ch["fuse"]["stats"]["matched_pairs"] > 0


def test_tsdf_every_view_contributes_and_the_views_see_different_voxels(mixed, tiny):
    sc, ch = mixed
    vw, maps, full = ch["tvw"], ch["maps"], ch["tsdf"]
    for v in range(sc.V):
        rest = [k for k in range(sc.V) if k != v]
        less = TR.integrate(vw, MC.pick(maps["depth"], rest), rest, **MC.VOLUME)
        diff = int((less["weight"] != full["weight"]).sum())
        print("without view %d the weight differs in %d voxels" % (v, diff))
        assert diff > 0 and diff == int(full["counted"][v].sum())
    x, y, z = TR.voxel_centres(MC.VOLUME["origin"], MC.VOLUME["voxel"], MC.VOLUME["dim"])
    shape = full["weight"].shape
    X = [np.broadcast_to(x[None, None, :], shape), np.broadcast_to(y[None, :, None], shape),
         np.broadcast_to(z[:, None, None], shape)]
    ok2, x2, y2 = projections(vw, 2, X)
    ok4, x4, y4 = projections(vw, 4, X)
    only_largest = ok2 & inside(x2, y2, sc.sizes[2]) & ~(ok4 & inside(x4, y4, sc.sizes[4]))
    print("voxels inside the largest view and outside the smallest:", int(only_largest.sum()))
    assert only_largest.any()
    mesh = TR.mesh(full["tsdf"], full["weight"], full["rgb"], origin=MC.VOLUME["origin"], voxel=MC.VOLUME["voxel"],
                   dim=MC.VOLUME["dim"])
    assert mesh["stats"]["triangles"] > 0
    # tiny: the single row and the single column alone still observe voxels
    sc, ch = tiny
    pair = [3, 2]
    two = TR.integrate(ch["tvw"], MC.pick(ch["maps"]["depth"], pair), pair, **MC.VOLUME)
    print("1 x 19 and 17 x 1 alone:", two["stats"], [int(c.sum()) for c in two["counted"]])
    assert all(c.any() for c in two["counted"])
