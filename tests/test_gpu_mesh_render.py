"""dp_mesh_render on the GPU against the CPU reference (tests/meshrender_ref.py,
restated from the header's spec): every byte of the depth, index and normal
planes and every integer statistic, in the host and the device form, with and
without culling."""
import os
import subprocess
import sys

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

import meshrender_ref as MR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
FORMS = ["host", "device"]


def views_of(P, W, H):
    return [dp.View(np.asarray(P[v], np.float64), np.zeros((H[v], W[v], 3), np.uint8)) for v in range(len(P))]


def render(eng, form, verts, tris, sizes, views=None, cull_back=False, want=("depth", "index", "normal")):
    """mesh_render in either form as the dict Engine.mesh_render returns; the
    device form renders into sentinel-filled buffers with slack behind every plane
    and checks that nothing beyond the planes, no plane that was not asked for,
    and no input was written"""
    verts, tris = np.ascontiguousarray(verts, dtype=dp.MESH_VERTEX_DTYPE), np.ascontiguousarray(tris, dtype=np.int32)
    vid = list(range(len(sizes))) if views is None else list(views)
    if form == "host":
        assert set(want) >= {"depth", "index"}
        return eng.mesh_render(verts, tris, views=views, cull_back=cull_back, normals="normal" in want)
    import torch

    nv, nt = len(verts), len(tris)
    dv, dt = (to_device(verts) if nv else None), (to_device(tris) if nt else None)
    width = {"depth": 4, "index": 4, "normal": 12}
    bufs = {k: [torch.full((sizes[v][0] * sizes[v][1] * width[k] + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
                for v in vid] for k in width}
    torch.cuda.synchronize()
    st = eng.mesh_render_device(dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt, vid,
                                *[[b.data_ptr() for b in bufs[k]] if k in want else None for k in width],
                                cull_back=cull_back)
    torch.cuda.synchronize()
    out = {"views": vid, "stats": st}
    for k, dtype in (("depth", np.float32), ("index", np.int32), ("normal", np.float32)):
        planes = []
        for j, v in enumerate(vid):
            raw = bufs[k][j].cpu().numpy()
            w, h = sizes[v]
            n = w * h * width[k] if k in want else 0
            assert (raw[n:] == SENTINEL).all(), (k, v)
            planes.append(raw[:n].view(dtype).reshape((h, w, 3) if k == "normal" else (h, w)).copy() if n else None)
        if k in want:
            out[k] = planes
    if nv:
        assert dv.cpu().numpy().tobytes() == verts.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == tris.tobytes()
    return out


def assert_equal(got, want, planes=("depth", "index", "normal")):
    assert got["views"] == want["views"]
    for name in planes:
        for k, v in enumerate(want["views"]):
            assert MR.same_bits(got[name][k], want[name][k]), (name, v)
    assert {c: got["stats"][c] for c in MR.COUNTS} == want["stats"]


@pytest.fixture(scope="module")
def sphere(orc):
    """the TSDF sphere, its cameras on level 0 and 1, an engine with the views and
    a pyramid, and the reference renders (computed once, never modified)"""
    verts, tris, centre, _ = MR.tsdf_sphere()
    P = MR.sphere_cameras(centre)
    W, H = [s[0] for s in MR.SPHERE_SIZES], [s[1] for s in MR.SPHERE_SIZES]
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in MR.SPHERE_SIZES]
    P1, imgs1 = orc.level_scene(np.asarray(P), imgs, 1)
    cams = {0: MR.Cameras(P, W, H), 1: MR.Cameras(P1, [im.shape[1] for im in imgs1], [im.shape[0] for im in imgs1])}
    want = {(lv, cull): MR.render(cams[lv], verts, tris, cull_back=cull) for lv in (0, 1) for cull in (False, True)}
    with dp.Engine(device=0) as eng:
        eng.set_views(views_of(P, W, H))
        eng.build_pyramid(2)
        yield dict(verts=verts, tris=tris, cams=cams, want=want, eng=eng)
        eng.set_level(0)


@pytest.fixture(scope="module")
def planted():
    P, W, H = MR.planted_cameras()
    verts, tris, names = MR.planted_mesh()
    cams = MR.Cameras(P, W, H)
    with dp.Engine(device=0) as eng:
        eng.set_views(views_of(P, W, H))
        yield dict(verts=verts, tris=tris, names=names, cams=cams, eng=eng, sizes=list(zip(W, H)))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("level", [0, 1])
def test_sphere_equals_reference_bit_for_bit(sphere, level, cull, form):
    eng, cams, want = sphere["eng"], sphere["cams"][level], sphere["want"][(level, cull)]
    eng.set_level(level)
    got = render(eng, form, sphere["verts"], sphere["tris"], list(zip(cams.W, cams.H)), cull_back=cull)
    assert_equal(got, want)
    # not vacuous: about a thousand triangles, every view sees the sphere, half
    # of the pairs face away and are culled without changing a depth
    assert 500 < want["stats"]["triangles"] == len(sphere["tris"]) and want["stats"]["invalid_triangles"] == 0
    assert all((d > 0).sum() > d.size // 8 for d in want["depth"])
    if cull:
        assert want["stats"]["culled_pairs"] > want["stats"]["pairs"] // 2
        assert all(MR.same_bits(a, b) for a, b in zip(want["depth"], sphere["want"][(level, False)]["depth"]))


def test_sphere_subset_order_and_null_planes(sphere):
    eng, cams = sphere["eng"], sphere["cams"][0]
    eng.set_level(0)
    sizes = list(zip(cams.W, cams.H))
    want = MR.render(cams, sphere["verts"], sphere["tris"], views=[4, 1])
    assert_equal(render(eng, "host", sphere["verts"], sphere["tris"], sizes, views=[4, 1]), want)
    assert_equal(render(eng, "device", sphere["verts"], sphere["tris"], sizes, views=[4, 1]), want)
    # NULL arrays: only the depth, only the normal
    for only in ("depth", "normal"):
        got = render(eng, "device", sphere["verts"], sphere["tris"], sizes, views=[4, 1], want=(only,))
        assert_equal(got, want, planes=(only,))
    # NULL entries inside an array, and no statistics: no plane of view 1 is written
    import torch

    w, h = sizes[4]
    d4 = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert eng.mesh_render_device(to_device(sphere["verts"]).data_ptr(), len(sphere["verts"]),
                                  to_device(sphere["tris"]).data_ptr(), len(sphere["tris"]), [4, 1],
                                  [d4.data_ptr(), 0], None, None, stats=False) is None
    torch.cuda.synchronize()
    assert MR.same_bits(d4.cpu().numpy(), want["depth"][0])
    # the whole set again after the smaller z-buffer
    assert_equal(eng.mesh_render(sphere["verts"], sphere["tris"], normals=True), sphere["want"][(0, False)])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cull", [False, True])
def test_planted_mesh(planted, cull, form):
    want = MR.render(planted["cams"], planted["verts"], planted["tris"], cull_back=cull)
    got = render(planted["eng"], form, planted["verts"], planted["tris"], planted["sizes"], cull_back=cull)
    assert_equal(got, want)
    # what the planted cases state (tests/test_mesh_render_cpu.py checks the
    # reference's side of each); here on the device's planes
    names, idx = planted["names"], got["index"][0]
    q0, q1 = names["quad"]
    assert all(idx[k, k] == q0 for k in range(8, 25)) and idx[8, 24] == q1 and idx[24, 8] == q0
    c0, c1 = names["coincident"]
    assert (idx == c0).sum() > 0 and (idx == c1).sum() == 0
    assert (idx == names["edge_on"][0]).sum() == 0
    assert got["stats"]["invalid_triangles"] == 4 and got["stats"]["clipped_pairs"] == 2 * 3
    b = names["back"][0]
    assert ((idx == b).sum() == 0) == cull
    assert got["stats"]["culled_pairs"] == (3 if cull else 0)


@pytest.mark.parametrize("form", FORMS)
def test_full_view_triangle_is_split_into_bands(planted, form):
    """one triangle covers the whole 96 x 64 view: its box exceeds the band budget,
    so several work items (the last one shorter) raster it; alone, and behind the
    planted mesh"""
    fv, ft = MR.full_view_triangle()
    want = MR.render(planted["cams"], fv, ft, views=[0, 1])
    assert (want["depth"][0] > 0).all() and (want["depth"][1] > 0).all()
    assert want["stats"]["pixel_tests"] == 96 * 64 + 67 * 45
    assert_equal(render(planted["eng"], form, fv, ft, planted["sizes"], views=[0, 1]), want)
    verts = np.concatenate([planted["verts"], fv])
    tris = np.concatenate([planted["tris"], ft + len(planted["verts"])]).astype(np.int32)
    want = MR.render(planted["cams"], verts, tris)
    assert (want["index"][0] == len(tris) - 1).sum() > 96 * 64 // 2
    assert_equal(render(planted["eng"], form, verts, tris, planted["sizes"]), want)


def test_no_triangles_and_no_vertices(planted):
    eng, sizes = planted["eng"], planted["sizes"]
    for form in FORMS:
        got = render(eng, form, planted["verts"], np.zeros((0, 3), np.int32), sizes)
        assert all((d == 0).all() for d in got["depth"]) and all((i == -1).all() for i in got["index"])
        assert all((n == 0).all() for n in got["normal"])
        assert {c: got["stats"][c] for c in MR.COUNTS} == dict.fromkeys(MR.COUNTS, 0)
        # without vertices every triangle is invalid
        got = render(eng, form, planted["verts"][:0], planted["tris"], sizes)
        assert got["stats"]["invalid_triangles"] == len(planted["tris"]) and got["stats"]["covered_pixels"] == 0
        assert all((i == -1).all() for i in got["index"])


CHUNK_CHILD = """
import os, sys
import numpy as np
os.environ["DP_MESH_RENDER_ITEM_CAP"] = sys.argv[1]
sys.path.insert(0, sys.argv[2])
import densepoints_amd as dp
import meshrender_ref as MR
from test_gpu_mesh_render import views_of
verts, tris, centre, _ = MR.tsdf_sphere()
P = MR.sphere_cameras(centre)
W, H = [s[0] for s in MR.SPHERE_SIZES], [s[1] for s in MR.SPHERE_SIZES]
with dp.Engine(device=0) as eng:
    eng.set_views(views_of(P, W, H))
    out = eng.mesh_render(verts, tris, normals=True)
np.savez(sys.argv[3], stats=np.array([out["stats"][c] for c in MR.COUNTS]),
         **{"%s%d" % (k, v): out[k][v] for k in ("depth", "index", "normal") for v in range(len(P))})
"""


def test_several_chunks_of_the_item_list(sphere, tmp_path):
    """DP_MESH_RENDER_ITEM_CAP = 500 with 5 views: 100 triangles per chunk, ten or
    more chunks, each raster sized from its own device-held counter.  The variable
    is set before the library is loaded, in a fresh child process; the planes equal
    those of the unchunked run."""
    out = str(tmp_path / "chunks.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    subprocess.run([sys.executable, "-c", CHUNK_CHILD, "500", os.path.join(ROOT, "tests"), out], check=True, env=env,
                   cwd=ROOT, timeout=300)
    got, want = np.load(out), sphere["want"][(0, False)]
    assert len(sphere["tris"]) > 1000
    for k in ("depth", "index", "normal"):
        for v in range(5):
            assert MR.same_bits(got["%s%d" % (k, v)], want[k][v]), (k, v)
    assert got["stats"].tolist() == [want["stats"][c] for c in MR.COUNTS]


def test_refusals(planted):
    import ctypes

    eng, verts, tris = planted["eng"], planted["verts"], planted["tris"]
    lib, ctx = N.lib, eng._ctx
    nv, nt = len(verts), len(tris)
    vid = np.array([0, 1, 2], np.int32)

    def call(vp=N.ptr(verts), n_v=nv, tp=N.ptr(tris), n_t=nt, views=vid, n_views=3, flags=0, device=False):
        mro = N.DpMeshRenderOptions(flags)
        args = [ctx, vp, n_v, tp, n_t, N.ptr(views) if views is not None else None, n_views, ctypes.byref(mro), None,
                None, None, None]
        return lib.dp_mesh_render_device(*args, None) if device else lib.dp_mesh_render(*args)

    for device in (False, True):
        assert call(n_v=-1, device=device) == N.DP_E_ARG
        assert call(n_t=-1, device=device) == N.DP_E_ARG
        assert call(n_v=2**31, device=device) == N.DP_E_ARG
        assert call(n_t=2**31, device=device) == N.DP_E_ARG
        assert call(vp=None, device=device) == N.DP_E_ARG
        assert call(tp=None, device=device) == N.DP_E_ARG
        assert call(views=None, device=device) == N.DP_E_ARG
        assert call(n_views=0, device=device) == N.DP_E_ARG
        assert call(n_views=4, views=np.array([0, 1, 2, 0], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, 1, 1], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, 1, 3], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, -1, 2], np.int32), device=device) == N.DP_E_ARG
        assert call(flags=2, device=device) == N.DP_E_ARG
        assert call(flags=-2**31, device=device) == N.DP_E_ARG
        with pytest.raises(Exception, match="dp_mesh_render"):
            N.check(call(flags=2, device=device), ctx)
    # NULL inputs with zero counts and NULL options are legal
    assert lib.dp_mesh_render(ctx, None, 0, None, 0, N.ptr(vid), 3, None, None, None, None, None) == N.DP_OK
    # no views set
    with dp.Engine(device=0) as bare:
        mro = N.DpMeshRenderOptions(0)
        assert lib.dp_mesh_render(bare._ctx, N.ptr(verts), nv, N.ptr(tris), nt, N.ptr(vid), 3, ctypes.byref(mro), None,
                                  None, None, None) == N.DP_E_STATE
        # a projection whose left 3x3 is singular never becomes a view: dp_set_views
        # refuses it, so dp_mesh_render's own m_v check is a second line
        flat = np.array([[32.0, 0, 32, 0], [0, 32, 32, 0], [32.0, 32, 64, 1]])
        with pytest.raises(Exception):
            bare.set_views(views_of([flat], [16], [16]))
    # the Python layer refuses the same before the library is called
    with pytest.raises(ValueError):
        eng.mesh_render(verts, tris, views=[0, 0])
    with pytest.raises(ValueError):
        eng.mesh_render(verts, tris, cull_back=1)
    with pytest.raises(ValueError):
        eng.mesh_render_device(0, 3, 0, 1, [0])
