"""dp_refine_maps without a GPU: the bindings and the argument validation, and
the CPU reference (tests/mapref_ref.py, restated from the spec in
include/densepoints.h) on the analytic plane4 scene -- exact depths, the true
normal -- restricted to crops of two reference views so that it runs in seconds."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs, synth

import mapref_ref as MR
import render_ref as RR
from test_render_cpu import Plane4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_default_mapref_options", "dp_refine_maps", "dp_refine_maps_device")
CROP = (slice(200, 248), slice(280, 344))    # rows, columns: well inside every view
CORNER = (slice(0, 24), slice(0, 40))        # windows and projections leave the images here
OFF = dict(sweep=0, reach=(0, 0))


class PlaneCase:
    """plane4 with its images: analytic ray-plane depths rounded to f32 and the
    constant true normal; the crops of views 0 and 1 are refined, views 2 and 3
    serve as sources only"""

    def __init__(self, orc):
        p4 = Plane4(orc)
        cfg = synth.config(p4.V, p4.W, p4.H, 0)
        P, imgs, _ = synth.scene_host(cfg)
        assert np.array_equal(P, p4.P)
        self.p4, self.V, self.W, self.H = p4, p4.V, p4.W, p4.H
        self.vw = MR.Views(orc, P, imgs)
        self.depth = [p4.analytic_depth(v).astype(np.float32) for v in range(p4.V)]
        self.normal = [np.broadcast_to(np.array([0, 0, 1], np.float32), (p4.H, p4.W, 3)).copy() for _ in range(p4.V)]

    def only(self, *regions):
        out = []
        for k in range(self.V):
            m = np.zeros((self.H, self.W), bool)
            if k < 2:
                for reg in regions:
                    m[reg] = True
            out.append(m)
        return out

    def moved_along_rays(self, v, feet):
        """the depth plane of view v with every true point moved along its ray by
        `feet` pixel footprints (plain numpy: independent of the reference), and
        the depth of one footprint"""
        Pv = np.array(self.vw.P[v])
        y, x = np.mgrid[0:self.H, 0:self.W].astype(np.float64)
        z = self.depth[v].astype(np.float64)
        X = np.einsum("ij,jhw->ihw", np.linalg.inv(Pv[:, :3]), np.stack([z * x, z * y, z]) - Pv[:, 3][:, None, None])
        ray = X - np.array(self.vw.C[v])[:, None, None]
        ray /= np.linalg.norm(ray, axis=0)

        def proj(Y):
            h = np.einsum("ij,jhw->ihw", Pv[:, :3], Y) + Pv[:, 3][:, None, None]
            return h[:2] / h[2], h[2]

        dx = np.linalg.norm(proj(X + np.array(self.vw.xr[v])[:, None, None])[0] - proj(X)[0], axis=0)
        one = proj(X + ray / dx)[1] - z
        return proj(X + feet * ray / dx)[1].astype(np.float32), one


@pytest.fixture(scope="module")
def plane(orc):
    return PlaneCase(orc)


def test_header_declares_and_native_binds_the_mapref_calls():
    txt = open(os.path.join(ROOT, "include", "densepoints.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, txt), f"{sym} not declared"
        assert sym in bound and hasattr(N.lib, sym)
    assert len(bound["dp_refine_maps"]) == 12 and len(bound["dp_refine_maps_device"]) == 13
    for struct, cls in (("dp_mapref_options", N.DpMaprefOptions), ("dp_mapref_stats", N.DpMaprefStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S)
        assert re.findall(r"\b([a-z_]+)(?:\[2\])?\s*[,;]", m.group(1)) == [name for name, _ in cls._fields_]
    assert ctypes.sizeof(N.DpMaprefOptions) == 36 and ctypes.sizeof(N.DpMaprefStats) == 56
    assert re.search(r"#define DP_MAPREF_KEEP_UNSCORED 1\b", txt) and N.MAPREF_KEEP_UNSCORED == MR.KEEP_UNSCORED == 1
    mo = N.DpMaprefOptions()
    N.lib.dp_default_mapref_options(ctypes.byref(mo))
    assert (mo.window, mo.sweep, mo.step_px, list(mo.reach), mo.max_sources, mo.top_k, mo.min_ncc, mo.flags) == \
        (7, 2, 1.0, [1, 4], 4, 2, 0.5, 0)
    d = pmvs.MAPREF_DEFAULTS
    assert bytes(pmvs.check_mapref_args(4)[0]) == bytes(mo) and d["reach"] == (1, 4) and d["window"] == 7
    assert N.lib.dp_abi_version() == 2
    v = np.zeros(1, np.int32)
    assert N.lib.dp_refine_maps(None, N.ptr(v), 1, None, None, None, None, None, None, None, None, None) == N.DP_E_ARG
    assert N.lib.dp_refine_maps_device(None, N.ptr(v), 1, None, None, None, None, None, None, None, None, None,
                                       None) == N.DP_E_ARG
    assert [name for name, _ in N.DpMaprefStats._fields_][:6] == list(MR.COUNTS)


def test_python_argument_validation_raises_before_any_device_call():
    mo, vid, src = pmvs.check_mapref_args(4)
    assert vid.tolist() == [0, 1, 2, 3] and vid.dtype == np.int32 and src is None
    mo, vid, src = pmvs.check_mapref_args(6, [4, 1, 2], [[1, 2], [4], []], window=11, sweep=8, reach=(16, 0),
                                          max_sources=3, top_k=3, min_ncc=-1, keep_unscored=True, step_px=0.5)
    assert src.tolist() == [[1, 2, -1], [4, -1, -1], [-1, -1, -1]] and src.dtype == np.int32
    assert (mo.window, mo.sweep, mo.step_px, list(mo.reach), mo.max_sources, mo.top_k, mo.min_ncc, mo.flags) == \
        (11, 8, 0.5, [16, 0], 3, 3, -1.0, 1)
    bad = [dict(window=2), dict(window=4), dict(window=13), dict(window=7.5), dict(sweep=-1), dict(sweep=9),
           dict(step_px=0), dict(step_px=-1.0), dict(step_px=float("nan")), dict(step_px=float("inf")),
           dict(reach=(17, 0)), dict(reach=(0, -1)), dict(reach=(1,)), dict(reach=3), dict(max_sources=0),
           dict(max_sources=9), dict(top_k=0), dict(top_k=5), dict(max_sources=2, top_k=3), dict(min_ncc=1.5),
           dict(min_ncc=-1.01), dict(min_ncc=float("nan")), dict(no_such_option=1),
           dict(views=[0, 0]), dict(views=[4]), dict(views=[-1]), dict(views=[]),
           dict(sources=[[1]]), dict(sources=[[0], [0], [0], [0]]), dict(sources=[[1, 1], [0], [0], [0]]),
           dict(sources=[[5], [0], [0], [0]]), dict(sources=[[1, 2, 3, 1, 2], [0], [0], [0]]),
           dict(views=[0, 1], sources=[[2], [0]])]
    for kw in bad:
        with pytest.raises(ValueError):
            pmvs.check_mapref_args(4, **kw)
    with pytest.raises(ValueError):
        pmvs.check_mapref_args(65)

    class NoDevice(dp.Engine):  # an engine that must not be reached
        def __init__(self):
            self._ctx, self._V, self._level, self.views = None, 4, 0, []

        def _check(self, rc):
            raise AssertionError("device call")

        def level_info(self, level, view):
            raise AssertionError("device call")

    eng = NoDevice()
    planes, normals = [np.zeros((4, 4), np.float32)] * 4, [np.zeros((4, 4, 3), np.float32)] * 4
    for kw in bad:
        with pytest.raises(ValueError):
            eng.refine_maps(planes, normals, **kw)
        with pytest.raises(ValueError):
            eng.refine_maps_device(kw.get("views", range(4)), [1] * 4, [2] * 4, [3] * 4,
                                   **{k: v for k, v in kw.items() if k != "views"})
    for args in (([0, 1], [1], [2, 2]), ([0, 1], [1, 0], [2, 2]), ([0, 1], [1, 1], [2]), ([0, 1], None, [2, 2]),
                 ([0, 1], [1, 1], None), ([0, 1], [1, 1], [2, 2], [3]), ([0, 1], [1, 5], [2, 2], [3, 5]),
                 ([0, 1], [1, 5], [2, 6], None, None, None, [7, 6])):
        with pytest.raises(ValueError):
            eng.refine_maps_device(*args)
    p = dp.PMVS()
    with pytest.raises(ValueError):
        p.depth_maps(refine=1)  # nothing has run
    p._ran = True
    for kw in (dict(refine=-1), dict(refine=1.5), dict(window=5), dict(refine=0, min_ncc=0.2)):
        with pytest.raises(ValueError):
            p.depth_maps(**kw)
        with pytest.raises(ValueError):
            p.fused_cloud(**kw)
    with pytest.raises(ValueError):
        p.fused_cloud(refine=1, normals=False)

    class Sized(NoDevice):  # shapes are checked against view_sizes, before the call
        def view_sizes(self, views=None):
            return [(6, 4)] * len(views)

    eng = Sized()
    good, gn = [np.zeros((4, 6), np.float32)] * 2, [np.zeros((4, 6, 3), np.float32)] * 2
    for depth, normal in ((good[:1], gn), ([np.zeros((6, 4), np.float32)] * 2, gn), (good, good), (good, gn[:1]),
                          (good, None)):
        with pytest.raises(ValueError):
            eng.refine_maps(depth, normal, views=[0, 1])
    with pytest.raises(AssertionError, match="device call"):
        eng.refine_maps(good, gn, views=[0, 1])


def test_identity(plane):
    """sweep 0, reach off, min_ncc -1: the only candidate is the pixel's own
    plane, so every input depth pixel with >= top_k valid sources comes out with
    choice 0 and its input depth bit for bit; the rest are empty, or kept under
    the flag"""
    only = plane.only(CROP, CORNER)
    out = MR.refine(plane.vw, plane.depth, plane.normal, min_ncc=-1.0, only=only, **OFF)
    kept = MR.refine(plane.vw, plane.depth, plane.normal, min_ncc=-1.0, only=only, flags=MR.KEEP_UNSCORED, **OFF)
    n_valid = n_void = 0
    for k in range(2):
        m = only[k]
        has = out["valid"][k] >= 2
        assert (out["valid"][k][m] >= 0).all()
        assert has[CROP].all()  # the crop is inside every view's image
        assert np.array_equal(out["choice"][k][m], np.where(has[m], 0, -1))
        assert MR.same_bytes(out["depth"][k][m], np.where(has[m], plane.depth[k][m], np.float32(0)))
        assert MR.same_bytes(out["normal"][k][m & has], plane.normal[k][m & has]) and not out["normal"][k][m & ~has].any()
        assert (np.abs(out["score"][k][m & has]) <= 1.0).all() and not out["score"][k][m & ~has].any()
        assert np.median(out["score"][k][CROP]) > 0.5  # exact geometry on a textured plane
        assert np.array_equal(kept["choice"][k][m], np.where(has[m], 0, -2))
        assert MR.same_bytes(kept["depth"][k][m], plane.depth[k][m])
        assert MR.same_bytes(kept["score"][k], out["score"][k])
        n_valid, n_void = n_valid + int(has[m].sum()), n_void + int((m & ~has).sum())
    assert n_valid > 6000 and n_void > 100
    st = out["stats"]
    assert st["kept"] == st["candidates"] == n_valid and st["moved"] == st["filled"] == 0
    assert st["depth_pixels_in"] == n_valid + n_void and kept["stats"] == st


@pytest.mark.parametrize("k", [1, 2])
def test_sweep_recovers_a_planted_offset(plane, k):
    """every true point moved along its ray by exactly -k footprints; with
    step_px 1 and sweep 2 the hypothesis h = +k is the truth.  Measured with the
    reference on the crops of views 0 and 1: k = 1 / 2: share choosing h = +k
    1.000 / 1.000, median |depth - truth| 3.5e-3 -> 6.8e-6 and 7.0e-3 -> 2.7e-5
    with one step 3.5e-3 (the printed line); the assertion is the ordering of
    the medians."""
    only = plane.only(CROP)
    depth, steps = [], []
    for v in range(plane.V):
        d, one = plane.moved_along_rays(v, -float(k))
        depth.append(d if v < 2 else plane.depth[v])
        steps.append(one)
    out = MR.refine(plane.vw, depth, plane.normal, sweep=2, step_px=1.0, reach=(0, 0), min_ncc=-1.0, only=only)
    before, after, share, step = [], [], [], []
    for v in range(2):
        assert (out["choice"][v][CROP] >= 0).all()
        before.append(np.abs(depth[v][CROP].astype(np.float64) - plane.depth[v][CROP]))
        after.append(np.abs(out["depth"][v][CROP].astype(np.float64) - plane.depth[v][CROP]))
        share.append(out["choice"][v][CROP] == 2 + k)
        step.append(np.abs(steps[v][CROP]))
    before, after, step = (float(np.median(np.concatenate([a.ravel() for a in x]))) for x in (before, after, step))
    print("planted offset -%d footprints: median |depth - truth| %.4g -> %.4g (one step %.4g), share choosing h = +%d: "
          "%.3f" % (k, before, after, step, k, float(np.mean(share))))
    assert after < before and after < 0.5 * step


def test_hole_filling(plane):
    """a blanked rectangle, min_ncc -1: after one pass the filled pixels are
    exactly the blank pixels with a depth pixel at one of the reach offsets (all
    of them see >= top_k valid sources here, by the reference's own rule: the
    identity test's crop), at the analytic ray-plane depth within 1e-5 relative
    (the render test's bound; observed maximum 6.8e-8, printed)"""
    hole = (slice(212, 236), slice(296, 328))  # 24 x 32, inside CROP
    depth = [d.copy() for d in plane.depth]
    blank = np.zeros((plane.H, plane.W), bool)
    blank[hole] = True
    for v in range(2):
        depth[v][hole] = 0
    out = MR.refine(plane.vw, depth, plane.normal, sweep=0, reach=(1, 4), min_ncc=-1.0, only=plane.only(CROP))
    near = np.zeros_like(blank)
    for d in (1, 4):
        for oy, ox in ((0, -d), (0, d), (-d, 0), (d, 0)):
            near |= np.roll(~blank, (-oy, -ox), (0, 1))
    want = blank & near
    assert 0 < want.sum() < blank.sum()
    worst = 0.0
    for v in range(2):
        filled = blank & (out["choice"][v] >= 0)
        assert np.array_equal(filled, want)
        assert (out["ncand"][v][want] > 0).all() and not out["ncand"][v][blank & ~want].any()
        assert (out["choice"][v][filled] >= 1).all()
        rel = np.abs(out["depth"][v][filled].astype(np.float64) / plane.depth[v][filled] - 1.0)
        worst = max(worst, float(rel.max()))
        assert MR.same_bytes(out["normal"][v][filled], plane.normal[v][filled])
        # outside the hole nothing is lost
        assert (out["choice"][v][CROP][~blank[CROP]] >= 0).all()
    print("hole filling: maximum relative depth error of a filled pixel %.3g" % worst)
    assert worst < 1e-5
    assert out["stats"]["filled"] == 2 * int(want.sum())


def test_photometric_rejection(plane):
    """a rectangle of view 1's depths scaled by 1.2, sweep 0 and reach off: its
    median score is below the rest's, and a min_ncc between the two medians (taken
    from the reference's own medians) removes more of it than of the rest"""
    rect = (slice(212, 236), slice(296, 328))
    depth = [d.copy() for d in plane.depth]
    depth[1][rect] *= np.float32(1.2)
    inside = np.zeros((plane.H, plane.W), bool)
    inside[rect] = True
    crop = np.zeros_like(inside)
    crop[CROP] = True
    only = [np.zeros_like(inside), crop, np.zeros_like(inside), np.zeros_like(inside)]
    free = MR.refine(plane.vw, depth, plane.normal, min_ncc=-1.0, only=only, **OFF)
    assert (free["choice"][1][crop] == 0).all()
    m_in, m_out = float(np.median(free["score"][1][inside])), float(np.median(free["score"][1][crop & ~inside]))
    print("photometric rejection (depths x 1.2): median score inside %.3f, outside %.3f" % (m_in, m_out))
    assert m_in < m_out
    thr = 0.5 * (m_in + m_out)
    out = MR.refine(plane.vw, depth, plane.normal, min_ncc=thr, only=only, **OFF)
    lost = out["choice"][1] < 0
    assert lost[inside].mean() > lost[crop & ~inside].mean()
    assert MR.same_bytes(out["depth"][1][~lost], free["depth"][1][~lost])
