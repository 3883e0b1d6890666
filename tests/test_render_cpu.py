"""dp_render_maps without a GPU: the CPU reference (tests/render_ref.py, restated
from the spec in include/densepoints.h) against analytic geometry, and the
host-side pieces -- bindings, PFM files, argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs, synth

import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_default_render_options", "dp_render_maps", "dp_render_maps_device")


class Plane4:
    """scene plane4 (4 x 640 x 480, the plane z = 0) without its images: the
    render reads cameras only"""

    def __init__(self, orc, V=4, W=640, H=480):
        self.cfg = synth.config(V, W, H, 0, depth_noise=0.0)
        self.P = synth.cameras(self.cfg)
        self.cams = RR.Cameras(orc, self.P, [W] * V, [H] * V)
        self.V, self.W, self.H = V, W, H

    def analytic_depth(self, v):
        """ray-plane depth of every pixel of view v: the X on z = 0 with
        P [X; 1] ~ (x, y, 1) has depth 1 / (M^-1 (x, y, 1))_2, M = P[:, (0, 1, 3)]"""
        Mi = np.linalg.inv(self.P[v][:, [0, 1, 3]])
        y, x = np.mgrid[0:self.H, 0:self.W].astype(np.float64)
        return 1.0 / (Mi[2, 0] * x + Mi[2, 1] * y + Mi[2, 2])

    def patches_on_grid(self, pitch_px=8.0, view=0, margin=0):
        """one patch per organizer cell centre of `view`, on the true surface,
        visible everywhere, ref = view: spacing rho by construction"""
        Mi = np.linalg.inv(self.P[view][:, [0, 1, 3]])
        cx = np.arange(margin, self.W // int(pitch_px) - margin) * pitch_px + pitch_px / 2
        cy = np.arange(margin, self.H // int(pitch_px) - margin) * pitch_px + pitch_px / 2
        gx, gy = np.meshgrid(cx, cy)
        h = Mi @ np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)])
        xy = (h[:2] / h[2]).T
        z, nrm = synth.surface(self.cfg, xy)
        assert (z == 0).all()
        pat = dp.empty_patches(len(xy))
        pat["pos"] = np.column_stack([xy, z]).astype(np.float32)
        pat["normal"] = nrm.astype(np.float32)
        pat["ref"] = view
        pat["vis"][:, 0] = (1 << self.V) - 1
        pat["score"] = 0.9
        return pat, (cx, cy)


@pytest.fixture(scope="module")
def plane(orc):
    return Plane4(orc)


def one_patch(plane, xy=(0.0, 0.0), dz=0.0, **fields):
    z, nrm = synth.surface(plane.cfg, np.array([xy]))
    p = dp.empty_patches(1)
    p["pos"] = np.array([xy[0], xy[1], z[0] + dz], np.float32)
    p["normal"] = nrm.astype(np.float32)
    p["vis"][:, 0] = (1 << plane.V) - 1
    p["score"] = 0.5
    for k, v in fields.items():
        p[k] = v
    return p


def wide_patches(cfg):
    """three patches of a 2 x 64 x 48 plane scene whose boxes exceed 64 pixels at
    splat_scale >= 4 (tests/test_gpu_render.py renders them on the device)"""
    xy = np.array([[0.0, 0.0], [0.05, -0.03], [-0.04, 0.04]])
    z, nrm = synth.surface(cfg, xy)
    pat = dp.empty_patches(3)
    pat["pos"] = np.column_stack([xy, z]).astype(np.float32)
    pat["normal"] = nrm.astype(np.float32)
    pat["vis"][:, 0] = 3
    pat["score"] = [0.9, 0.8, 0.7]
    # a tilted disc: its plane crosses z = 0, in front on one side of the line
    pat["normal"][1] = (np.array([0.3, 0.1, 1.0]) / np.linalg.norm([0.3, 0.1, 1.0])).astype(np.float32)
    return pat


WIDE_CASES = (dict(splat_scale=4.0, max_radius_px=32), dict(splat_scale=40.0, max_radius_px=255))


def test_header_declares_and_native_binds_the_render_calls():
    txt = open(os.path.join(ROOT, "include", "densepoints.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, txt), f"{sym} not declared"
        assert sym in bound and hasattr(N.lib, sym)
    assert len(bound["dp_render_maps"]) == 12 and len(bound["dp_render_maps_device"]) == 13
    for struct, cls in (("dp_render_options", N.DpRenderOptions), ("dp_render_stats", N.DpRenderStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S)
        assert re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1)) == [name for name, _ in cls._fields_]
    assert ctypes.sizeof(N.DpRenderOptions) == 12 and ctypes.sizeof(N.DpRenderStats) == 40
    ro = N.DpRenderOptions()
    N.lib.dp_default_render_options(ctypes.byref(ro))
    assert (ro.splat_scale, ro.max_radius_px, ro.flags) == (1.0, 32, 0)
    assert N.lib.dp_abi_version() == 2
    v = np.zeros(1, np.int32)
    assert N.lib.dp_render_maps(None, None, 0, None, N.ptr(v), 1, None, None, None, None, None, None) == N.DP_E_ARG
    assert N.lib.dp_render_maps_device(None, None, 0, None, N.ptr(v), 1, None, None, None, None, None, None,
                                       None) == N.DP_E_ARG


def test_analytic_plane_depth(plane):
    """patches on the true surface: every covered pixel's depth is the analytic
    ray-plane depth within relative 1e-5 (pos and normal are f32, 2^-24 relative
    each, so the disc's plane moves ~1e-7 of the scene scale; the output is f32)"""
    pat, _ = plane.patches_on_grid(pitch_px=8.0)
    out = RR.render(plane.cams, pat)
    worst = 0.0
    for k, v in enumerate(out["views"]):
        hit = out["index"][k] >= 0
        assert hit.sum() > 1000
        want = plane.analytic_depth(v)
        rel = np.abs(out["depth"][k].astype(np.float64)[hit] - want[hit]) / want[hit]
        worst = max(worst, float(rel.max()))
    print("analytic plane: maximum relative depth error %.3g" % worst)
    assert worst < 1e-5
    assert out["stats"]["patches"] == len(pat) and out["stats"]["pairs"] > len(pat)


def test_coverage_of_a_grid_of_pitch_rho(plane):
    """discs of radius rho on a grid of pitch rho cover the plane: every pixel of
    view 0 inside the patch grid shrunk by one cell is non-empty"""
    pat, (cx, cy) = plane.patches_on_grid(pitch_px=8.0, view=0, margin=4)
    rho = np.array([RR.rho_of(plane.cams, p) for p in pat])
    # the covering condition: no point of a grid cell is farther than rho from
    # its corners, i.e. the cell's world half-diagonal is below every rho (the
    # plane is oblique to view 0, so 8 px span up to ~1.2 rho on it, not rho)
    X = pat["pos"].astype(np.float64).reshape(len(cy), len(cx), 3)
    diag = np.maximum(np.linalg.norm(X[1:, 1:] - X[:-1, :-1], axis=2), np.linalg.norm(X[1:, :-1] - X[:-1, 1:], axis=2))
    R = rho.reshape(len(cy), len(cx))
    corner_rho = np.minimum(np.minimum(R[1:, 1:], R[:-1, :-1]), np.minimum(R[1:, :-1], R[:-1, 1:]))
    assert (0.5 * diag < 0.9 * corner_rho).all()
    out = RR.render(plane.cams, pat, views=[0])
    x0, x1 = int(np.ceil(cx[1])), int(np.floor(cx[-2]))
    y0, y1 = int(np.ceil(cy[1])), int(np.floor(cy[-2]))
    inner = out["index"][0][y0:y1 + 1, x0:x1 + 1]
    assert inner.size > 100000 and (inner >= 0).all()
    assert out["stats"]["covered_pixels"] < plane.W * plane.H  # the margin stays empty


def test_occlusion_and_ties(plane):
    C0 = np.array(plane.cams.C[0])
    far = one_patch(plane, ref=0)
    near = far.copy()
    near["pos"] = (C0 + 0.8 * (far["pos"][0].astype(np.float64) - C0)).astype(np.float32)  # same ray, in front
    out = RR.render(plane.cams, np.concatenate([far, near]), views=[0])
    idx = out["index"][0]
    assert set(np.unique(idx)) == {-1, 0, 1}
    both = [p for p in out["pairs"]]
    ys, xs = np.nonzero(idx == 0)
    # the overlap (pixels the near disc covers) shows the near index everywhere
    only_near = RR.render(plane.cams, near, views=[0])["index"][0] >= 0
    assert only_near.sum() > 10 and (idx[only_near] == 1).all()
    assert (out["depth"][0][only_near] < RR.render(plane.cams, far, views=[0])["depth"][0].max()).all()
    assert len(both) == 2 and len(ys) > 0
    # two identical patches: the lower index everywhere
    twin = RR.render(plane.cams, np.concatenate([far, far, far])[[0, 1, 2]], views=[0, 2])
    for k in range(2):
        assert set(np.unique(twin["index"][k])) == {-1, 0}
    assert twin["stats"]["pairs"] == 6


def test_skips_write_no_pixel(plane):
    cams, V = plane.cams, plane.V
    C0, xr0 = np.array(cams.C[0]), np.array(cams.xr[0])
    base = one_patch(plane, ref=0)
    assert RR.render(cams, base)["stats"]["covered_pixels"] > 0
    behind = base.copy()
    behind["pos"] = (C0 - 0.5 * (base["pos"][0].astype(np.float64) - C0)).astype(np.float32)
    assert RR.row(cams.P[0], 2, [float(c) for c in behind["pos"][0]]) < 0
    cases = {"behind the camera": (behind, dict(views=[0])),
             "ref >= V": (one_patch(plane, ref=V), {}),
             "NaN position": (one_patch(plane, ref=0, pos=np.array([np.nan, 0, 0], np.float32)), {}),
             "infinite normal": (one_patch(plane, ref=0, normal=np.array([0, np.inf, 1], np.float32)), {}),
             "edge-on to the x-axis": (one_patch(plane, ref=1, normal=xr0.astype(np.float32)), dict(views=[0])),
             "not in vis": (one_patch(plane, ref=0, vis=np.array([0b1110, 0], np.uint64)), dict(views=[0])),
             "keep == 0": (base, dict(keep=np.zeros(1, np.uint8)))}
    for name, (p, kw) in cases.items():
        out = RR.render(cams, p, **kw)
        assert out["stats"]["covered_pixels"] == 0 and out["stats"]["pairs"] == 0, name
        assert all((i == -1).all() for i in out["index"]) and all((d == 0).all() for d in out["depth"]), name
    # the edge-on patch: s < 1e-12 in view 0 although the patch takes part
    edge = cases["edge-on to the x-axis"][0]
    n = [float(c) for c in edge["normal"][0]]
    t = RR.dot(cams.xr[0], n)
    e1 = [cams.xr[0][k] - t * n[k] for k in range(3)]
    assert RR.dot(e1, e1) < 1e-12 and RR.takes_part(cams, edge[0])
    # ALL_FACING renders the patch that is not in vis into the views it faces:
    # a stored normal points away from the cameras that see the patch
    back = cases["not in vis"][0]  # the surface normal points at the cameras
    assert RR.render(cams, back, all_facing=True)["stats"]["pairs"] == 0
    hidden = back.copy()
    hidden["normal"] = -hidden["normal"]
    assert RR.render(cams, hidden, views=[0])["stats"]["pairs"] == 0
    assert RR.render(cams, hidden, views=[0], all_facing=True)["stats"]["covered_pixels"] > 0
    assert RR.render(cams, hidden, all_facing=True)["stats"]["pairs"] == V


def test_box_clamp(plane):
    p = one_patch(plane, ref=0)
    out = RR.render(plane.cams, p, splat_scale=50.0, max_radius_px=3)
    assert out["stats"]["pairs"] == plane.V
    for pr in out["pairs"]:
        assert 7 <= pr["x1"] - pr["x0"] + 1 <= 8 and 7 <= pr["y1"] - pr["y0"] + 1 <= 8
        assert pr["hits"] == (pr["x1"] - pr["x0"] + 1) * (pr["y1"] - pr["y0"] + 1)  # the disc exceeds the box
    # unclamped, the box holds the whole disc: a wider clamp changes nothing
    a = RR.render(plane.cams, p, max_radius_px=32)
    b = RR.render(plane.cams, p, max_radius_px=255)
    assert all(RR.same_bits(x, y) for x, y in zip(a["index"], b["index"]))
    assert all(pr["hits"] < (pr["x1"] - pr["x0"] + 1) * (pr["y1"] - pr["y0"] + 1) for pr in a["pairs"])


def test_wide_case_premises(orc):
    """the hand-made patches of the GPU test's wide-box case: boxes above 64
    pixels, a 64-pixel row, an occlusion"""
    cfg = synth.config(2, 64, 48, 0)
    cams = RR.Cameras(orc, synth.cameras(cfg), [64, 64], [48, 48])
    pat = wide_patches(cfg)
    for kw in WIDE_CASES:
        out = RR.render(cams, pat, **kw)
        assert out["stats"]["pairs"] == 6 and out["stats"]["covered_pixels"] > 64
        assert all((p["x1"] - p["x0"] + 1) * (p["y1"] - p["y0"] + 1) > 64 for p in out["pairs"])
        assert len(set(np.unique(out["index"][0]).tolist()) - {-1}) >= 2
    assert any(p["x1"] - p["x0"] + 1 == 64 for p in out["pairs"])


@pytest.mark.parametrize("shape", [(5, 7), (4, 3, 3), (1, 1), (6, 2, 1)])
def test_pfm_round_trip(tmp_path, shape):
    rng = np.random.default_rng(3)
    a = rng.normal(size=shape).astype(np.float32)
    a.flat[0] = 0.0
    path = str(tmp_path / "a.pfm")
    dp.write_pfm(path, a)
    b = dp.read_pfm(path)
    want = a[:, :, 0] if len(shape) == 3 and shape[2] == 1 else a
    assert RR.same_bits(b, want)
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n-1.0\n" % (b"PF" if want.ndim == 3 else b"Pf", shape[1], shape[0])
    assert raw.startswith(head) and len(raw) == len(head) + 4 * want.size
    # bottom-up: the file's first row is the array's last, little-endian
    first = np.frombuffer(raw, "<f4", count=want[0].size, offset=len(head))
    assert np.array_equal(first, want[-1].ravel())


def test_pfm_rejects_other_shapes(tmp_path):
    for bad in (np.zeros(3), np.zeros((2, 2, 2)), np.zeros((1, 2, 3, 4))):
        with pytest.raises(ValueError):
            dp.write_pfm(str(tmp_path / "bad.pfm"), bad)
    (tmp_path / "x.pfm").write_bytes(b"P6\n1 1\n255\nabc")
    with pytest.raises(ValueError):
        dp.read_pfm(str(tmp_path / "x.pfm"))


def test_python_argument_validation_raises_before_any_device_call():
    ok = dict(n=3, V=4, views=None, keep=None, splat_scale=1.0, max_radius_px=32, all_facing=False)
    ro, vid, keep = pmvs.check_render_args(**ok)
    assert vid.tolist() == [0, 1, 2, 3] and vid.dtype == np.int32 and keep is None
    assert (ro.splat_scale, ro.max_radius_px, ro.flags) == (1.0, 32, 0)
    assert pmvs.check_render_args(**dict(ok, all_facing=True, views=[2, 0]))[0].flags == N.RENDER_ALL_FACING
    bad = [dict(views=[0, 0]), dict(views=[4]), dict(views=[-1]), dict(views=[]), dict(splat_scale=0.0),
           dict(splat_scale=-1.0), dict(splat_scale=float("nan")), dict(max_radius_px=0), dict(max_radius_px=256),
           dict(max_radius_px=2.5), dict(n=2**31), dict(keep=np.ones(2, np.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            pmvs.check_render_args(**dict(ok, **kw))

    class NoDevice(dp.Engine):  # an engine that must not be reached
        def __init__(self):
            self._ctx, self._V, self._level, self.views = None, 4, 0, []

        def _check(self, rc):
            raise AssertionError("device call")

        def level_info(self, level, view):
            raise AssertionError("device call")

    eng = NoDevice()
    pat = dp.empty_patches(3)
    for kw in bad:
        if "n" in kw:
            continue
        with pytest.raises(ValueError):
            eng.render_maps(pat, **kw)
    with pytest.raises(ValueError):
        eng.render_maps_device(0, 3, None, [1, 1])
    with pytest.raises(ValueError):
        eng.render_maps_device(0, 3, None, [0, 1], d_depth=[0])
    with pytest.raises(ValueError):
        dp.PMVS().depth_maps()  # nothing has run
