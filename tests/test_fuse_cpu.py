"""dp_fuse_maps without a GPU: the CPU reference (tests/fuse_ref.py, restated from
the spec in include/densepoints.h) against analytic geometry, and the host-side
pieces -- bindings, struct layouts, the PLY writer, argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs
from densepoints_amd._native import FUSED_DTYPE, DpFuseOptions, DpFuseStats

import fuse_ref as FR
from test_render_cpu import Plane4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_default_fuse_options", "dp_fuse_maps", "dp_fuse_maps_device")
TOL = 0.01
RECT = (slice(200, 260), slice(280, 360))  # rows, columns of view 1


class PlaneCase:
    """plane4 (4 x 640 x 480, the plane z = 0): analytic ray-plane depth planes
    rounded to f32 and constant normal planes, with their reference fusions
    (computed once, never modified)"""

    def __init__(self, orc):
        p4 = Plane4(orc)
        self.V, self.W, self.H = p4.V, p4.W, p4.H
        self.vw = FR.Views(p4.P, [p4.W] * p4.V, [p4.H] * p4.V)
        self.depth = [p4.analytic_depth(v).astype(np.float32) for v in range(p4.V)]
        self.normal = [np.broadcast_to(np.array([0, 0, 1], np.float32), (p4.H, p4.W, 3)).copy() for _ in range(p4.V)]
        assert all((d > 0).all() for d in self.depth)
        self.base = FR.fuse(self.vw, self.depth, self.normal)
        self.all_views = FR.fuse(self.vw, self.depth, self.normal, min_views=p4.V - 1)


@pytest.fixture(scope="module")
def plane(orc):
    return PlaneCase(orc)


def projects_inside(vw, r, s, depth_r):
    """the pixels of view r whose point lands on a pixel of view s (plain numpy
    matrices, independent of the reference's arithmetic order)"""
    P_r, P_s = np.array(vw.P[r]), np.array(vw.P[s])
    H, W = depth_r.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = depth_r.astype(np.float64)
    b = np.stack([z * x - P_r[0, 3], z * y - P_r[1, 3], z - P_r[2, 3]])
    X = np.einsum("ij,jhw->ihw", np.linalg.inv(P_r[:, :3]), b)
    h = np.einsum("ij,jhw->ihw", P_s[:, :3], X) + P_s[:, 3][:, None, None]
    u, v = h[0] / h[2], h[1] / h[2]
    # half a pixel inside the rounding limits, so that both computations agree
    return (h[2] > 0) & (u > -0.49) & (u < vw.W[s] - 0.51) & (v > -0.49) & (v < vw.H[s] - 0.51), \
        (h[2] > 0) & (u > -0.51) & (u < vw.W[s] - 0.49) & (v > -0.51) & (v < vw.H[s] - 0.49)


def test_header_declares_and_native_binds_the_fuse_calls():
    txt = open(os.path.join(ROOT, "include", "densepoints.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, txt), f"{sym} not declared"
        assert sym in bound and hasattr(N.lib, sym)
    assert len(bound["dp_fuse_maps"]) == 9 and len(bound["dp_fuse_maps_device"]) == 11
    for struct, cls in (("dp_fuse_options", DpFuseOptions), ("dp_fuse_stats", DpFuseStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S)
        assert re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1)) == [name for name, _ in cls._fields_]
    m = re.search(r"typedef struct dp_fused_point \{(.*?)\} dp_fused_point;", txt, flags=re.S)
    assert re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", m.group(1)) == list(FUSED_DTYPE.names)
    assert ctypes.sizeof(DpFuseOptions) == 16 and ctypes.sizeof(DpFuseStats) == 48
    assert FUSED_DTYPE.itemsize == 40 and FUSED_DTYPE == FR.POINT and dp.FUSED_DTYPE is FUSED_DTYPE
    assert re.search(r"#define DP_FUSE_NO_SUPPRESS 1\b", txt) and N.FUSE_NO_SUPPRESS == FR.NO_SUPPRESS == 1
    fo = DpFuseOptions()
    N.lib.dp_default_fuse_options(ctypes.byref(fo))
    assert (fo.depth_tol, fo.min_views, fo.min_normal_cos, fo.flags) == (np.float32(0.01), 2, 0.5, 0)
    assert N.lib.dp_abi_version() == 2
    v, n = np.zeros(1, np.int32), ctypes.c_int64()
    assert N.lib.dp_fuse_maps(None, N.ptr(v), 1, None, None, None, None, ctypes.byref(n), None) == N.DP_E_ARG
    assert N.lib.dp_fuse_maps_device(None, N.ptr(v), 1, None, None, None, None, 0, ctypes.byref(n), None,
                                     None) == N.DP_E_ARG


def test_analytic_plane(plane):
    """every pixel whose point lands inside another view is consistent with it;
    every emitted position lies on z = 0 within 1e-5 of its depth (the render
    test's bound: the planes are f32, 2^-24 relative, and so is the output);
    the normals are the plane's"""
    out, K = plane.base, plane.V
    assert out["stats"]["depth_pixels"] == K * plane.W * plane.H
    assert out["stats"]["matched_pairs"] == out["stats"]["consistent_pairs"] > 0
    for k in range(K):
        for kp in range(K):
            if kp == k:
                continue
            sure, maybe = projects_inside(plane.vw, k, kp, plane.depth[k])
            bit = ((out["mask"][k] >> np.uint64(kp)) & np.uint64(1)).astype(bool)
            assert sure.sum() > 1000 and bit[sure].all() and not bit[~maybe].any(), (k, kp)
    pts = out["points"]
    assert len(pts) == out["stats"]["emitted"] > 100000
    z_own = np.concatenate([plane.depth[k][out["emitted"][k]] for k in range(K)])
    worst = float((np.abs(pts["pos"][:, 2].astype(np.float64)) / z_own).max())
    print("analytic plane: maximum |z| / depth of an emitted position %.3g" % worst)
    assert worst < 1e-5
    assert (pts["normal"] == np.array([0, 0, 1], np.float32)).all()
    # the mean of the agreeing back-projections stays near the pixel's own point:
    # each of them is the point of a pixel within half a pixel of it in its view,
    # so within the largest diagonal pixel footprint on the plane
    foot = 0.0
    for v in range(K):
        y, x = np.mgrid[0:plane.H, 0:plane.W]
        G = np.stack(FR.backproject(plane.vw, v, x.ravel(), y.ravel(), plane.depth[v].ravel()), 1)
        G = G.reshape(plane.H, plane.W, 3)
        foot = max(foot, float(np.linalg.norm(G[1:, 1:] - G[:-1, :-1], axis=2).max()))
    own = np.concatenate([np.stack(FR.backproject(plane.vw, k, *np.nonzero(out["emitted"][k])[::-1],
                                                  plane.depth[k][out["emitted"][k]]), 1) for k in range(K)])
    assert (np.linalg.norm(pts["pos"].astype(np.float64) - own, axis=1) < foot).all()
    assert (pts["n_views"] == [1 + bin(int(m)).count("1") for k in range(K) for m in
                               out["mask"][k][out["emitted"][k]]]).all()


def in_rect(xi, yi):
    return (yi >= RECT[0].start) & (yi < RECT[0].stop) & (xi >= RECT[1].start) & (xi < RECT[1].stop)


def lands_in_rect(plane, k, kr):
    """pixels of view k whose point is matched to a pixel of view kr's rectangle"""
    ys, xs = np.nonzero(FR.is_depth(plane.depth[k]))
    X = FR.backproject(plane.vw, k, xs, ys, plane.depth[k][ys, xs])
    matched, _, xi, yi, _ = FR.observe(plane.vw, kr, X, plane.depth[kr], np.float64(np.float32(TOL)))
    hit = np.zeros(plane.depth[k].shape, bool)
    hit[ys, xs] = matched & in_rect(xi, yi)
    return hit


def test_depth_disagreement_is_rejected(plane):
    K, kr = plane.V, 1
    depth = [d.copy() for d in plane.depth]
    depth[kr][RECT] *= np.float32(1 + 3 * TOL)
    out = FR.fuse(plane.vw, depth, plane.normal, min_views=K - 1, depth_tol=TOL)
    was = plane.all_views["fusable"][kr][RECT]
    assert was.sum() > 1000  # the rectangle was fusable with every view agreeing
    assert not out["fusable"][kr][RECT].any()
    assert np.array_equal(out["fusable"][kr][:RECT[0].start], plane.all_views["fusable"][kr][:RECT[0].start])
    for k in range(K):
        if k == kr:
            continue
        hit = lands_in_rect(plane, k, kr)
        bit = ((out["mask"][k] >> np.uint64(kr)) & np.uint64(1)).astype(bool)
        before = ((plane.base["mask"][k] >> np.uint64(kr)) & np.uint64(1)).astype(bool)
        assert hit.sum() > 1000 and before[hit].all() and not bit[hit].any(), k
        assert np.array_equal(bit[~hit], before[~hit])
    assert out["stats"]["matched_pairs"] > out["stats"]["consistent_pairs"]


def test_normal_disagreement_is_rejected_only_with_normal_planes(plane):
    K, kr = plane.V, 1
    normal = [n.copy() for n in plane.normal]
    normal[kr][RECT] *= -1
    out = FR.fuse(plane.vw, plane.depth, normal, min_views=K - 1)
    assert plane.all_views["fusable"][kr][RECT].sum() > 1000 and not out["fusable"][kr][RECT].any()
    for k in range(K):
        if k == kr:
            continue
        hit = lands_in_rect(plane, k, kr)
        bit = ((out["mask"][k] >> np.uint64(kr)) & np.uint64(1)).astype(bool)
        assert hit.sum() > 1000 and not bit[hit].any(), k
    # the same planes without normals: nothing is rejected, and the normals are zeros
    plain = FR.fuse(plane.vw, plane.depth, None, min_views=K - 1)
    assert all(np.array_equal(plain["mask"][k], plane.all_views["mask"][k]) for k in range(K))
    assert np.array_equal(plain["points"]["pos"], plane.all_views["points"]["pos"])
    assert (plain["points"]["normal"] == 0).all()
    # a zero normal agrees with every normal: c = 0 passes c >= 0 and c*c >= cs^2 * 0
    zero = [n.copy() for n in plane.normal]
    zero[kr][RECT] = 0
    assert FR.fuse(plane.vw, plane.depth, zero, min_views=K - 1)["stats"] == plane.all_views["stats"]


def test_suppression(plane):
    K = plane.V
    base = plane.base
    free = FR.fuse(plane.vw, plane.depth, plane.normal, flags=FR.NO_SUPPRESS)
    assert free["stats"]["emitted"] == free["stats"]["fusable"] == base["stats"]["fusable"]
    assert 0 < base["stats"]["emitted"] < base["stats"]["fusable"]
    assert all(np.array_equal(free["emitted"][k], free["fusable"][k]) for k in range(K))
    tol = np.float64(np.float32(TOL))
    for k in range(K):
        ys, xs = np.nonzero(base["fusable"][k])
        X = FR.backproject(plane.vw, k, xs, ys, plane.depth[k][ys, xs])
        has_lower = np.zeros(len(xs), bool)
        for kp in range(k):
            _, good, xi, yi, _ = FR.observe(plane.vw, kp, X, plane.depth[kp], tol)
            has_lower |= good & base["fusable"][kp][yi, xi]
        assert np.array_equal(base["emitted"][k][ys, xs], ~has_lower), k
        assert not base["emitted"][k][~base["fusable"][k]].any()
    assert np.array_equal(base["emitted"][0], base["fusable"][0])  # nothing precedes the first view
    # the order of `views` decides which view emits a shared point
    order = [1, 0, 2, 3]
    swap = FR.fuse(plane.vw, [plane.depth[v] for v in order], [plane.normal[v] for v in order], views=order)
    assert swap["stats"]["fusable"] == base["stats"]["fusable"]
    assert np.array_equal(swap["emitted"][0], swap["fusable"][0]) and np.array_equal(swap["fusable"][0], base["fusable"][1])
    assert (swap["points"]["view"] == 1).sum() > (base["points"]["view"] == 1).sum()
    assert (swap["points"]["view"] == 0).sum() < (base["points"]["view"] == 0).sum()
    assert swap["points"]["view"][0] == 1


def test_small_cases(plane):
    vw = plane.vw
    # min_views = 0 emits every depth pixel that no earlier view holds; without
    # suppression all of them, at the pixel's own back-projection when alone
    depth = [plane.depth[0][:, :].copy(), plane.depth[1].copy()]
    bad = np.array([np.nan, -1.0, np.inf, -np.inf, 0.0, -0.0], np.float32)
    depth[0][240, 300:306] = bad
    depth[1][250, 320:326] = bad
    out = FR.fuse(vw, depth, None, views=[0, 1], min_views=0, flags=FR.NO_SUPPRESS)
    n_depth = 2 * plane.W * plane.H - 12
    assert out["stats"]["depth_pixels"] == out["stats"]["fusable"] == out["stats"]["emitted"] == n_depth
    assert not out["emitted"][0][240, 300:306].any() and not out["emitted"][1][250, 320:326].any()
    assert np.isfinite(out["points"]["pos"]).all()
    # K = 1: no other view, every mask is empty, pos == (float)backproject
    one = FR.fuse(vw, [depth[0]], None, views=[0], min_views=0)
    assert one["stats"] == dict(depth_pixels=plane.W * plane.H - 6, matched_pairs=0, consistent_pairs=0,
                                fusable=plane.W * plane.H - 6, emitted=plane.W * plane.H - 6)
    p = one["points"]
    X = FR.backproject(vw, 0, p["x"], p["y"], depth[0][p["y"], p["x"]])
    assert FR.same_bytes(p["pos"], np.stack(X, 1).astype(np.float32)) and (p["n_views"] == 1).all()
    assert not one["mask"][0].any()
    assert FR.fuse(vw, [depth[0]], None, views=[0], min_views=1)["stats"]["emitted"] == 0
    # the non-depths are not matched targets either: a pixel of view 1 landing on them sees nothing
    two = FR.fuse(vw, depth, None, views=[0, 1])
    ys, xs = np.nonzero(FR.is_depth(depth[1]))
    Xb = FR.backproject(vw, 1, xs, ys, depth[1][ys, xs])
    _, _, xi, yi, _ = FR.observe(vw, 0, Xb, depth[0], np.float64(np.float32(TOL)))
    on_bad = (yi == 240) & (xi >= 300) & (xi < 306)
    assert on_bad.sum() > 0 and not two["mask"][1][ys[on_bad], xs[on_bad]].any()


def test_output_order_and_ply(plane, tmp_path):
    pts = plane.base["points"]
    key = (pts["view"].astype(np.int64) * plane.H + pts["y"]) * plane.W + pts["x"]
    assert (np.diff(key) > 0).all()  # views = 0..V-1: k is the view id
    order = [2, 0]
    sub = FR.fuse(plane.vw, [plane.depth[v] for v in order], None, views=order, min_views=1)["points"]
    rank = np.where(sub["view"] == 2, 0, 1)
    assert set(sub["view"]) == {0, 2} and (np.diff((rank.astype(np.int64) * plane.H + sub["y"]) * plane.W + sub["x"]) > 0).all()
    # write_ply takes a fused array unchanged
    some = pts[::5000].astype(FUSED_DTYPE)
    some["rgb"] = (np.arange(len(some) * 3).reshape(-1, 3) % 256).astype(np.uint8)
    path = tmp_path / "fused.ply"
    dp.write_ply(str(path), some)
    lines = path.read_text().splitlines()
    assert lines[2] == "element vertex %d" % len(some) and lines[12] == "end_header" and len(lines) == 13 + len(some)
    rows = np.array([[float(t) for t in ln.split()] for ln in lines[13:]])
    assert np.allclose(rows[:, :3], some["pos"], rtol=1e-5) and np.array_equal(rows[:, 3:6], some["rgb"])
    assert np.allclose(rows[:, 6:], some["normal"], rtol=1e-5)
    as_patches = dp.empty_patches(len(some))
    for f in ("pos", "rgb", "normal"):
        as_patches[f] = some[f]
    ref = tmp_path / "ref.ply"
    dp.write_ply(str(ref), as_patches)
    assert ref.read_bytes() == path.read_bytes()


def test_python_argument_validation_raises_before_any_device_call():
    ok = dict(V=4, views=None, depth_tol=0.01, min_views=2, min_normal_cos=0.5, suppress=True)
    fo, vid = pmvs.check_fuse_args(**ok)
    assert vid.tolist() == [0, 1, 2, 3] and vid.dtype == np.int32
    assert (fo.depth_tol, fo.min_views, fo.min_normal_cos, fo.flags) == (np.float32(0.01), 2, 0.5, 0)
    assert pmvs.check_fuse_args(**dict(ok, suppress=False, views=[2, 0]))[0].flags == N.FUSE_NO_SUPPRESS
    assert pmvs.check_fuse_args(**dict(ok, depth_tol=0, min_views=0, min_normal_cos=1))[0].min_views == 0
    assert pmvs.check_fuse_args(**dict(ok, V=64, min_views=63))[0].min_views == 63
    bad = [dict(views=[0, 0]), dict(views=[4]), dict(views=[-1]), dict(views=[]), dict(V=65), dict(depth_tol=-0.1),
           dict(depth_tol=float("nan")), dict(depth_tol=float("inf")), dict(min_views=-1), dict(min_views=64),
           dict(min_views=1.5), dict(min_normal_cos=-0.1), dict(min_normal_cos=1.1), dict(min_normal_cos=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            pmvs.check_fuse_args(**dict(ok, **kw))

    class NoDevice(dp.Engine):  # an engine that must not be reached
        def __init__(self):
            self._ctx, self._V, self._level, self.views = None, 4, 0, []

        def _check(self, rc):
            raise AssertionError("device call")

        def level_info(self, level, view):
            raise AssertionError("device call")

    eng = NoDevice()
    planes = [np.zeros((4, 4), np.float32)] * 4
    for kw in bad:
        if "V" in kw:
            continue
        with pytest.raises(ValueError):
            eng.fuse_maps(planes, **kw)
        with pytest.raises(ValueError):
            eng.fuse_maps_device(kw.get("views", range(4)), [1] * 4, None, 1, 1,
                                 **{k: v for k, v in kw.items() if k != "views"})
    for args in (([0, 1], [1], None, 1, 1), ([0, 1], [1, 0], None, 1, 1), ([0, 1], [1, 1], [1], 1, 1),
                 ([0, 1], [1, 1], None, 0, 1), ([0, 1], [1, 1], None, 1, -1), ([0, 1], None, None, 1, 1)):
        with pytest.raises(ValueError):
            eng.fuse_maps_device(*args)
    with pytest.raises(ValueError):
        dp.PMVS().fused_cloud()  # nothing has run

    class Sized(NoDevice):  # shapes are checked against view_sizes, before the fusion is called
        def view_sizes(self, views=None):
            return [(6, 4)] * len(views)

    eng = Sized()
    good = [np.zeros((4, 6), np.float32)] * 2
    for depth, normal in ((good[:1], None), ([np.zeros((6, 4), np.float32)] * 2, None),
                          (good, [np.zeros((4, 6), np.float32)] * 2), (good, [np.zeros((4, 6, 3), np.float32)])):
        with pytest.raises(ValueError):
            eng.fuse_maps(depth, normal, views=[0, 1])
    with pytest.raises(AssertionError, match="device call"):
        eng.fuse_maps(good, [np.zeros((4, 6, 3), np.float32)] * 2, views=[0, 1])
