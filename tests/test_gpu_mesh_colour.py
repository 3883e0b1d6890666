"""dp_mesh_colour on the GPU against the CPU reference (tests/meshcolour_ref.py,
restated from the header's spec): every byte of vertices_out, seen and best and
every integer statistic, in the host and the device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import synth

import meshcolour_ref as CR
import meshrender_ref as MR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
PLANTED = dict(depth_tol=0.25, min_cos=0.0)


def views_of(P, images):
    return [dp.View(np.asarray(P[v], np.float64), images[v]) for v in range(len(P))]


def colour(eng, form, verts, depth, views=None, normals=None, want=("seen", "best"), **kw):
    """mesh_colour in either form as the dict Engine.mesh_colour returns; the
    device form writes into sentinel-filled buffers with slack behind them and
    checks that nothing beyond the results, no output that was not asked for and
    no input was written"""
    verts = np.ascontiguousarray(verts, dtype=dp.MESH_VERTEX_DTYPE)
    nv = len(verts)
    vid = list(range(eng.num_views())) if views is None else list(views)
    if form == "host":
        return eng.mesh_colour(verts, views=views, depth=depth, normals=normals, **kw)
    import torch

    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
    dv = to_device(verts) if nv else None
    dn = to_device(nrm) if nrm is not None and nv else None
    dd = [to_device(p) for p in depth]
    width = {"vertices": 16, "seen": 8, "best": 4}
    bufs = {k: torch.full((nv * width[k] + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for k in width}
    torch.cuda.synchronize()
    st = eng.mesh_colour_device(dv.data_ptr() if nv else None, nv, vid, [t.data_ptr() for t in dd],
                                bufs["vertices"].data_ptr(), d_normals=dn.data_ptr() if dn is not None else None,
                                d_seen=bufs["seen"].data_ptr() if "seen" in want else None,
                                d_best=bufs["best"].data_ptr() if "best" in want else None, **kw)
    torch.cuda.synchronize()
    out = {"views": vid, "stats": st}
    for k, dtype in (("vertices", dp.MESH_VERTEX_DTYPE), ("seen", np.uint64), ("best", np.int32)):
        raw = bufs[k].cpu().numpy()
        n = nv * width[k] if k == "vertices" or k in want else 0
        assert (raw[n:] == SENTINEL).all(), k
        if k == "vertices" or k in want:
            out[k] = raw[:n].view(dtype).copy()
    if nv:
        assert dv.cpu().numpy().tobytes() == verts.tobytes()
    if dn is not None:
        assert dn.cpu().numpy().tobytes() == nrm.tobytes()
    for t, p in zip(dd, depth):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(p).tobytes()
    return out


def assert_equal(got, want, outputs=("vertices", "seen", "best")):
    assert got["views"] == want["views"]
    for name in outputs:
        assert CR.same_bits(got[name], want[name]), name
    assert {c: got["stats"][c] for c in CR.COUNTS} == want["stats"]
    assert got["stats"]["colour_ms"] >= 0


@pytest.fixture(scope="module")
def sphere(orc):
    """the TSDF sphere, hashed images of its cameras on level 0 and 1, the
    reference's depth planes of the mesh, analytic normals, an engine with the
    views and a pyramid, and the reference colours (computed once, never
    modified)"""
    verts, tris, centre, _ = MR.tsdf_sphere()
    verts = verts.copy()
    verts["rgb"] = [200, 100, 50]
    P = MR.sphere_cameras(centre)
    imgs = [CR.hash_image(v, w, h) for v, (w, h) in enumerate(MR.SPHERE_SIZES)]
    P1, imgs1 = orc.level_scene(np.asarray(P), imgs, 1)
    scene = {0: (P, imgs), 1: (P1, imgs1)}
    nrm = verts["pos"].astype(np.float64) - centre
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    depth, want = {}, {}
    for lv, (Pl, il) in scene.items():
        cams = MR.Cameras(Pl, [im.shape[1] for im in il], [im.shape[0] for im in il])
        depth[lv] = MR.render(cams, verts, tris)["depth"]
        for normals in (False, True):
            for bilinear in (False, True):
                want[(lv, normals, bilinear)] = CR.colour(Pl, il, verts, depth[lv], normals=nrm if normals else None,
                                                          bilinear=bilinear)
    with dp.Engine(device=0) as eng:
        eng.set_views(views_of(P, imgs))
        eng.build_pyramid(2)
        yield dict(verts=verts, tris=tris, normals=nrm, depth=depth, want=want, scene=scene, eng=eng)
        eng.set_level(0)


@pytest.fixture(scope="module")
def planted():
    s = CR.planted()
    with dp.Engine(device=0) as eng:
        eng.set_views(views_of(s["P"], s["images"]))
        yield dict(s, eng=eng)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("level", [0, 1])
def test_sphere_equals_reference_bit_for_bit(sphere, level, normals, bilinear, form):
    eng, want = sphere["eng"], sphere["want"][(level, normals, bilinear)]
    eng.set_level(level)
    got = colour(eng, form, sphere["verts"], sphere["depth"][level], normals=sphere["normals"] if normals else None,
                 bilinear=bilinear)
    assert_equal(got, want)
    # not vacuous: every view contributes, every view leaves vertices unseen (the
    # far side), and most vertices are coloured
    st, nv = want["stats"], len(sphere["verts"])
    for k in range(5):
        sees = ((want["seen"] >> np.uint64(k)) & np.uint64(1)).sum()
        assert 0 < sees < nv, k
        assert not normals or (want["best"] == k).any(), k
    assert st["vertices"] == nv and st["coloured_vertices"] > nv // 2 and st["occluded_pairs"] > nv // 2
    assert (st["grazing_pairs"] > 0) == normals
    assert (want["vertices"]["rgb"][want["seen"] != 0] != [200, 100, 50]).any()
    assert (want["vertices"]["rgb"][want["seen"] == 0] == [200, 100, 50]).all()


def test_sphere_subset_order_and_unwanted_outputs(sphere):
    eng = sphere["eng"]
    eng.set_level(0)
    P, imgs = sphere["scene"][0]
    depth = [sphere["depth"][0][4], sphere["depth"][0][1]]
    want = CR.colour(P, imgs, sphere["verts"], depth, views=[4, 1], normals=sphere["normals"], clear_unseen=True)
    for form in FORMS:
        assert_equal(colour(eng, form, sphere["verts"], depth, views=[4, 1], normals=sphere["normals"],
                            clear_unseen=True), want)
    assert (want["vertices"]["rgb"][want["seen"] == 0] == 0).all() and (want["seen"] == 0).any()
    # without seen and best: the same vertices, nothing else written
    got = colour(eng, "device", sphere["verts"], depth, views=[4, 1], normals=sphere["normals"], clear_unseen=True,
                 want=())
    assert_equal(got, want, outputs=("vertices",))
    assert "seen" not in got and "best" not in got
    # the planes the engine renders itself are the reference's
    own = eng.mesh_colour(sphere["verts"], triangles=sphere["tris"], normals=sphere["normals"])
    assert_equal(own, sphere["want"][(0, True, False)])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("clear_unseen", [False, True])
@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_planted_planes(planted, normals, clear_unseen, form):
    s, eng = planted, planted["eng"]
    nrm = s["normals"] if normals else None
    want = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], normals=nrm, clear_unseen=clear_unseen, **PLANTED)
    got = colour(eng, form, s["vertices"], s["depth"], normals=nrm, clear_unseen=clear_unseen, **PLANTED)
    assert_equal(got, want)

    def seen(label):
        return int(got["seen"][s["names"][label]])

    def rgb(label):
        return list(got["vertices"]["rgb"][s["names"][label]])

    unseen = [0, 0, 0] if clear_unseen else [9, 8, 7]
    assert seen("tol_edge") == 0b101 and seen("tol_over") == 0 and seen("behind_surface") == 0b101
    assert seen("half_even_down") == 1 and rgb("half_even_down") == list(s["images"][0][10, 20, ::-1])
    assert seen("half_even_up") == 1 and rgb("half_even_up") == list(s["images"][0][10, 22, ::-1])
    for label in ("outside", "behind_camera", "empty_pixel", "tol_over"):
        assert seen(label) == 0 and rgb(label) == unseen and got["best"][s["names"][label]] == -1
    for label in ("nan", "inf"):  # copied, not counted, not cleared
        assert seen(label) == 0 and rgb(label) == [9, 8, 7] and got["best"][s["names"][label]] == -1
    assert got["stats"]["vertices"] == len(s["vertices"]) - 2
    assert seen("two_views") == 0b011 and rgb("two_views") == [2, 2, 2]
    assert seen("zero_normal") == 0b101 and seen("corner_8x8") == 0b0010 and seen("wide_last_column") == 0b1000
    assert seen("right_angle") == (0 if normals else 0b101) and seen("facing_away") == (0 if normals else 0b101)
    assert got["stats"]["grazing_pairs"] == (4 if normals else 0)


@pytest.mark.parametrize("form", FORMS)
def test_planted_bilinear_and_subset(planted, form):
    s, eng = planted, planted["eng"]
    depth = [s["depth"][2], s["depth"][0], s["depth"][3]]
    want = CR.colour(s["P"], s["images"], s["vertices"], depth, views=[2, 0, 3], normals=s["normals"], bilinear=True,
                     **PLANTED)
    assert_equal(colour(eng, form, s["vertices"], depth, views=[2, 0, 3], normals=s["normals"], bilinear=True,
                        **PLANTED), want)
    assert int(want["seen"][s["names"]["tol_edge"]]) == 0b011 and want["best"][s["names"]["wide_last_column"]] == 2


@pytest.mark.parametrize("form", FORMS)
def test_last_of_64_views(form):
    s = CR.last_of_64()
    want = CR.colour(s["P"], s["images"], s["vertices"], s["depth"])
    with dp.Engine(device=0) as eng:
        eng.set_views(views_of(s["P"], s["images"]))
        got = colour(eng, form, s["vertices"], s["depth"])
    assert_equal(got, want)
    assert int(got["seen"][0]) == 1 << 63 and got["best"][0] == 63 and got["stats"]["visible_pairs"] == 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 257])
def test_block_tail(planted, n, form):
    s, eng = planted, planted["eng"]
    idx = np.arange(n) % len(s["vertices"])
    verts, nrm = s["vertices"][idx], s["normals"][idx]
    want = CR.colour(s["P"], s["images"], verts, s["depth"], normals=nrm, **PLANTED)
    got = colour(eng, form, verts, s["depth"], normals=nrm, **PLANTED)
    assert_equal(got, want)
    assert len(got["vertices"]) == n and (n == 0 or got["stats"]["visible_pairs"] > 0)


def test_refusals(planted):
    s, eng = planted, planted["eng"]
    lib, ctx = N.lib, eng._ctx
    verts, nv = s["vertices"], len(s["vertices"])
    vid = np.array([0, 1, 2, 3], np.int32)
    planes = [np.ascontiguousarray(p) for p in s["depth"]]
    seen, best = np.zeros(nv, np.uint64), np.zeros(nv, np.int32)

    def call(vp=N.ptr(verts), n_v=nv, views=vid, n_views=4, tol=0.01, min_cos=0.2, flags=0, depth=planes,
             out=True, seen_p=None, device=False):
        mco = N.DpMeshColourOptions(tol, min_cos, flags)
        tab = None if depth is None else (ctypes.c_void_p * len(depth))(*[p.ctypes.data if p is not None else None
                                                                          for p in depth])
        pv = ctypes.c_void_p()
        args = [ctx, vp, n_v, None, N.ptr(views) if views is not None else None, n_views, ctypes.byref(mco), tab]
        if device:  # refused before any address is used
            return lib.dp_mesh_colour_device(*args, vp if out else None, seen_p, None, None, None)
        return lib.dp_mesh_colour(*args, ctypes.byref(pv) if out else None, seen_p, None, None)

    for device in (False, True):
        assert call(n_v=-1, device=device) == N.DP_E_ARG
        assert call(n_v=2**31, device=device) == N.DP_E_ARG
        assert call(vp=None, device=device) == N.DP_E_ARG
        assert call(views=None, device=device) == N.DP_E_ARG
        assert call(n_views=0, device=device) == N.DP_E_ARG
        assert call(n_views=5, views=np.array([0, 1, 2, 3, 0], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, 1, 1, 2], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, 1, 4, 2], np.int32), device=device) == N.DP_E_ARG
        assert call(views=np.array([0, -1, 3, 2], np.int32), device=device) == N.DP_E_ARG
        assert call(depth=None, device=device) == N.DP_E_ARG
        assert call(depth=planes[:2] + [None] + planes[3:], device=device) == N.DP_E_ARG
        for tol in (-0.5, float("inf"), float("nan")):
            assert call(tol=tol, device=device) == N.DP_E_ARG
        for mc in (-0.1, 1.5, float("nan")):
            assert call(min_cos=mc, device=device) == N.DP_E_ARG
        assert call(flags=4, device=device) == N.DP_E_ARG
        assert call(flags=-2**31, device=device) == N.DP_E_ARG
        assert call(out=False, device=device) == N.DP_E_ARG
        with pytest.raises(Exception, match="dp_mesh_colour"):
            N.check(call(flags=4, device=device), ctx)
    # an output that equals an input: the vertices (device form), a plane
    assert call(device=True) == N.DP_E_ARG
    assert call(seen_p=ctypes.c_void_p(planes[1].ctypes.data)) == N.DP_E_ARG
    # n_vertices = 0 with NULL vertices and NULL options is legal
    pv = ctypes.c_void_p(1)
    tab = (ctypes.c_void_p * 4)(*[p.ctypes.data for p in planes])
    assert lib.dp_mesh_colour(ctx, None, 0, None, N.ptr(vid), 4, None, tab, ctypes.byref(pv), None, None,
                              None) == N.DP_OK and pv.value is None
    # no views set
    with dp.Engine(device=0) as bare:
        assert lib.dp_mesh_colour(bare._ctx, N.ptr(verts), nv, None, N.ptr(vid), 4, None, tab, ctypes.byref(pv),
                                  N.ptr(seen), N.ptr(best), None) == N.DP_E_STATE
    # the Python layer refuses the same before the library is called
    with pytest.raises(ValueError):
        eng.mesh_colour(verts, views=[0, 0], depth=planes[:2])
    with pytest.raises(ValueError):
        eng.mesh_colour(verts, depth=planes[:3])
    with pytest.raises(ValueError):
        eng.mesh_colour(verts)  # neither planes nor triangles
    with pytest.raises(ValueError):
        eng.mesh_colour(verts, depth=planes, normals=s["normals"][:3])
    with pytest.raises(ValueError):
        eng.mesh_colour(verts, depth=[p[:-1] for p in planes])
    with pytest.raises(ValueError):
        eng.mesh_colour_device(64, 3, [0], [128], 64)


@pytest.fixture(scope="module")
def pm():
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    pm = dp.PMVS()
    for v in range(4):
        pm.add_camera(dp.View(P[v], synth.render_host(cfg, P, v)))
    assert pm.run(synth.seeds(cfg, P))
    return pm


def test_pmvs_mesh_colour(pm):
    v0, t0, n0 = pm.mesh(dim=40, smooth=dict(iterations=2), normals=True)
    opts = dict(bilinear=True, min_cos=0.1)
    v1, t1, n1 = pm.mesh(dim=40, smooth=dict(iterations=2), normals=True, colour=opts)
    assert len(t0) > 0 and CR.same_bits(t0, t1) and CR.same_bits(n0, n1)
    assert CR.same_bits(v0["pos"], v1["pos"]) and CR.same_bits(v0["pad"], v1["pad"])
    with dp.Engine(device=0) as eng:
        eng.set_views(pm.views)
        want = eng.mesh_colour(v0, triangles=t0, normals=n0, **opts)
        plain = eng.mesh_colour(v0, triangles=t0)
    assert CR.same_bits(v1, want["vertices"])
    assert {c: pm.stats["mesh_colour"][c] for c in CR.COUNTS} == {c: want["stats"][c] for c in CR.COUNTS}
    assert want["stats"]["coloured_vertices"] > len(v0) // 2 and not CR.same_bits(v1["rgb"], v0["rgb"])
    # without normals=True the weights are 1
    v2, t2 = pm.mesh(dim=40, smooth=dict(iterations=2), colour={})
    assert CR.same_bits(t2, t0) and CR.same_bits(v2, plain["vertices"])
    with pytest.raises(ValueError):
        pm.mesh(dim=40, colour=dict(min_cos=2.0))
