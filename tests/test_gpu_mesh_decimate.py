"""dp_mesh_decimate on the GPU against the CPU reference
(tests/meshdecimate_ref.py, restated from the header's spec): every byte of the
vertices, the triangles and the maps and every integer statistic, in the host
and the device form and in both modes."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import MESH_VERTEX_DTYPE
from densepoints_amd import _native as N

import meshdecimate_ref as DR
import meshsmooth_ref as SR
import tsdf_ref as TR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
MODES = [False, True]


@pytest.fixture(scope="module")
def eng():
    # no views are set: the call reads none
    with dp.Engine(device=0) as e:
        yield e


def device_buffer(records, size):
    import torch

    return torch.full(((records + 3) * size,), SENTINEL, dtype=torch.uint8, device="cuda")


def pick(stats):
    return {c: stats[c] for c in DR.COUNTS}


def decimate(eng, form, verts, tris, cell, origin=(0.0, 0.0, 0.0), quadric=False, vcap=None, tcap=None, maps=True,
             stats=True):
    """mesh_decimate in either form as dict(vertices, triangles, vertex_map,
    triangle_map, stats, counts); the device form checks the sentinels beyond
    min(cap, count) records and beyond the maps, and that the inputs are unchanged"""
    verts, tris = np.ascontiguousarray(verts, dtype=MESH_VERTEX_DTYPE), DR.as_triangles(tris)
    nv, nt = len(verts), len(tris)
    if form == "host":
        vo, to, st, vm, tm = eng.mesh_decimate(verts, tris, cell, origin, quadric, maps=True)
        return dict(vertices=vo, triangles=to, vertex_map=vm, triangle_map=tm, stats=st, counts=(len(vo), len(to)))
    import torch

    vcap, tcap = nv if vcap is None else vcap, nt if tcap is None else tcap
    dv, dt = (to_device(verts) if nv else None), (to_device(tris) if nt else None)
    vb, tb, vmb, tmb = device_buffer(vcap, 16), device_buffer(tcap, 12), device_buffer(nv, 4), device_buffer(nt, 4)
    torch.cuda.synchronize()
    no, to_, st = eng.mesh_decimate_device(dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt,
                                           vb.data_ptr() if vcap else None, vcap, tb.data_ptr() if tcap else None, tcap,
                                           cell, origin, quadric, vmb.data_ptr() if maps else None,
                                           tmb.data_ptr() if maps else None, stats=stats)
    torch.cuda.synchronize()
    rv, rt, rvm, rtm = (b.cpu().numpy() for b in (vb, tb, vmb, tmb))
    wv, wt = min(no, vcap), min(to_, tcap)
    assert (rv[wv * 16:] == SENTINEL).all() and (rt[wt * 12:] == SENTINEL).all()
    assert (rvm[(nv * 4 if maps else 0):] == SENTINEL).all() and (rtm[(nt * 4 if maps else 0):] == SENTINEL).all()
    if nv:
        assert dv.cpu().numpy().tobytes() == verts.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == tris.tobytes()
    return dict(vertices=rv[:wv * 16].view(MESH_VERTEX_DTYPE).copy(), triangles=rt[:wt * 12].view(np.int32).reshape(-1, 3).copy(),
                vertex_map=rvm[:nv * 4].view(np.int32).copy() if maps else None,
                triangle_map=rtm[:nt * 4].view(np.int32).copy() if maps else None, stats=st, counts=(no, to_))


def assert_equal(got, want):
    assert pick(got["stats"]) == want["stats"]
    assert got["counts"] == (len(want["vertices"]), len(want["triangles"]))
    for k in ("vertices", "triangles", "vertex_map", "triangle_map"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def tsdf_sphere():
    """the sphere of a 16^3 volume (the size test_gpu_mesh_smooth.py uses) with its volume"""
    vol, _ = SR.sphere_volume(16)
    m = TR.mesh(vol["tsdf"], vol["weight"], None, origin=vol["origin"], voxel=vol["voxel"], dim=vol["dim"])
    verts = m["vertices"].astype(MESH_VERTEX_DTYPE)
    verts["rgb"] = DR.colours(len(verts), 7)
    return verts, SR.as_triangles(m["triangles"]), vol


def wide_mesh():
    """more than 2^21 vertices, nearly all unused: the canonical triple no longer
    fits one key and is sorted in two passes.  The planted triangles on the first
    vertices, again (moved by 8 cells) on the last, and three triangles that name
    both ends, two of them in the same three cells."""
    pv, pt = DR.planted_mesh()
    nv = 2**21 + 40
    verts = np.zeros(nv, MESH_VERTEX_DTYPE)
    top = nv - len(pv)
    verts[:len(pv)], verts[top:] = pv, pv
    verts["pos"][top:] += np.float32(8.0)
    shifted = np.where((pt >= 0) & (pt < len(pv)), pt + top, pt)
    mixed = np.array([(0, top + 1, top + 2), (3, top + 4, top + 5), (top + 6, 8, 7)], np.int32)
    return verts, np.concatenate([pt, shifted, mixed]).astype(np.int32)


def cases():
    sphere, cube, planted = DR.uv_sphere(24, 48), DR.cube(8), DR.planted_mesh()
    tv, tt, vol = tsdf_sphere()
    return {
        "sphere": (sphere, dict(cell=0.5)),
        "cube": (cube, dict(cell=0.25, origin=(-0.0625,) * 3)),
        "planted": (planted, DR.PLANTED),
        "sphere_fine": (sphere, dict(cell=0.1)),      # 872 clusters, 9 blocks of triangles
        "sphere_coarse": (sphere, dict(cell=1.0)),    # clusters of ~150 members: the long sequential sums
        "tsdf_sphere": ((tv, tt), dict(cell=float(np.float32(2.0 * float(np.float32(vol["voxel"])))), origin=vol["origin"])),
        "wide": (wide_mesh(), DR.PLANTED),
    }


@pytest.fixture(scope="module")
def wanted():
    """the reference's result of every case in both modes, computed once"""
    out = {}
    for name, ((verts, tris), opts) in cases().items():
        for quadric in MODES:
            out[name, quadric] = (verts, tris, opts, DR.decimate(verts, tris, quadric=quadric, **opts))
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("quadric", MODES, ids=["mean", "quadric"])
@pytest.mark.parametrize("name", ["sphere", "cube", "planted", "sphere_fine", "sphere_coarse", "tsdf_sphere", "wide"])
def test_against_the_reference(eng, wanted, name, quadric, form):
    verts, tris, opts, want = wanted[name, quadric]
    got = decimate(eng, form, verts, tris, quadric=quadric, **opts)
    assert_equal(got, want)
    assert got["stats"]["decimate_ms"] > 0
    st = want["stats"]
    if name == "sphere_fine":
        assert st["clusters"] > 256 and len(tris) > 8 * 256
    if name == "sphere_coarse":
        assert st["max_cluster"] >= 150
    if name == "tsdf_sphere":
        assert 0 < st["triangles_out"] < len(tris) and len(verts) > 256
    if name == "wide":
        assert len(verts) > 2**21 and st["duplicate_triangles"] >= 2 and st["triangles_out"] >= 6
    if quadric and name in ("sphere", "sphere_fine", "planted"):
        assert "outside" in want["placement"] and "quadric" in want["placement"]
    if quadric and name == "cube":
        assert want["placement"].count("unsolvable") == 90


@pytest.mark.parametrize("form", FORMS)
def test_empty_inputs(eng, form):
    for nv, tris in ((0, []), (5, []), (0, [(0, 0, 0), (0, 1, 2)]), (4, [(0, 1, 4), (-1, 2, 3)]), (4, [(0, 0, 1), (1, 1, 1)])):
        verts = DR.random_vertices(nv, 4)
        for quadric in MODES:
            want = DR.decimate(verts, tris, 0.5, quadric=quadric)
            assert want["stats"]["vertices_out"] == 0 and want["stats"]["unused_vertices"] == nv
            assert_equal(decimate(eng, form, verts, tris, 0.5, quadric=quadric), want)
    if form == "host":  # the context-owned results of an empty call are NULL
        pv, pt, no, to = ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_int64(9), ctypes.c_int64(9)
        o = dp.check_mesh_decimate_args(1.0)
        N.check(N.lib.dp_mesh_decimate(eng._ctx, ctypes.byref(o), None, 0, None, 0, ctypes.byref(pv), ctypes.byref(no),
                                       ctypes.byref(pt), ctypes.byref(to), None, None, None), eng._ctx)
        assert (pv.value, pt.value, no.value, to.value) == (None, None, 0, 0)


@pytest.mark.parametrize("quadric", MODES, ids=["mean", "quadric"])
def test_caps_null_maps_and_no_stats(eng, wanted, quadric):
    """caps of 0, of count - 1 and of count: the full counts, the first min(cap,
    count) records and nothing beyond them; the maps left out; stats = None"""
    verts, tris, opts, want = wanted["cube", quadric]
    VO, TO = len(want["vertices"]), len(want["triangles"])
    for vcap, tcap in ((0, 0), (VO - 1, TO - 1), (VO, TO), (VO - 1, TO), (VO, 0)):
        got = decimate(eng, "device", verts, tris, quadric=quadric, vcap=vcap, tcap=tcap, **opts)
        assert got["counts"] == (VO, TO) and pick(got["stats"]) == want["stats"]
        assert got["vertices"].tobytes() == want["vertices"][:vcap].tobytes()
        assert got["triangles"].tobytes() == want["triangles"][:tcap].tobytes()
        assert got["vertex_map"].tobytes() == want["vertex_map"].tobytes()
        assert got["triangle_map"].tobytes() == want["triangle_map"].tobytes()
    got = decimate(eng, "device", verts, tris, quadric=quadric, maps=False, stats=False, **opts)
    assert got["stats"] is None and got["counts"] == (VO, TO) and got["vertex_map"] is None
    assert got["vertices"].tobytes() == want["vertices"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_twice_gives_identical_bytes(eng, wanted, form):
    verts, tris, opts, want = wanted["sphere_fine", True]
    a = decimate(eng, form, verts, tris, quadric=True, **opts)
    b = decimate(eng, form, verts, tris, quadric=True, **opts)
    for k in ("vertices", "triangles", "vertex_map", "triangle_map"):
        assert a[k].tobytes() == b[k].tobytes() == want[k].tobytes(), k
    assert pick(a["stats"]) == pick(b["stats"])


@pytest.mark.parametrize("quadric", MODES, ids=["mean", "quadric"])
def test_orientation_survives(eng, quadric):
    """the normals of the decimated closed sphere point away from its centre"""
    verts, tris, vol = tsdf_sphere()
    _, centre = SR.sphere_volume(16)
    vo, to, st = eng.mesh_decimate(verts, tris, 2.0 * vol["voxel"], vol["origin"], quadric)
    assert 0 < len(to) < len(tris) and st["duplicate_triangles"] == 0
    edges = {(int(a), int(b)) for t in to for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert len(edges) == 3 * len(to) and edges == {(b, a) for a, b in edges}  # closed
    nrm, nst = eng.mesh_normals(vo, to)
    assert nst["zero_normals"] == 0
    dots = np.einsum("ij,ij->i", nrm.astype(np.float64), vo["pos"].astype(np.float64) - centre)
    assert (dots > 0).all()


def test_refusals(eng):
    """every argument error: DP_E_ARG with a message, nothing written"""
    import torch

    verts, tris = DR.cube(4)
    nv, nt = len(verts), len(tris)
    dv, dt = to_device(verts), to_device(tris)
    vb, tb, vmb, tmb = device_buffer(nv, 16), device_buffer(nt, 12), device_buffer(nv, 4), device_buffer(nt, 4)
    torch.cuda.synchronize()
    lib, ctx = N.lib, eng._ctx
    good = dp.check_mesh_decimate_args(0.25)
    no, to = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def call(o=good, v=dv.data_ptr(), n_v=nv, t=dt.data_ptr(), n_t=nt, vo=vb.data_ptr(), vcap=nv, p_no=ctypes.byref(no),
             to_=tb.data_ptr(), tcap=nt, p_to=ctypes.byref(to), vm=vmb.data_ptr(), tm=tmb.data_ptr()):
        return lib.dp_mesh_decimate_device(ctx, ctypes.byref(o) if o is not None else None, v, n_v, t, n_t, vo, vcap, p_no,
                                           to_, tcap, p_to, vm, tm, None, None)

    def opt(cell=0.25, origin=(0.0, 0.0, 0.0), mode=0, flags=0):
        return N.DpMeshDecimateOptions((ctypes.c_float * 3)(*origin), cell, mode, flags, 0)

    big = (2**31 - 1) // 3 + 1
    bad = [(dict(o=None), b"opts"), (dict(o=opt(cell=0.0)), b"cell"), (dict(o=opt(cell=-1.0)), b"cell"),
           (dict(o=opt(cell=float("nan"))), b"cell"), (dict(o=opt(cell=float("inf"))), b"cell"),
           (dict(o=opt(origin=(0.0, float("nan"), 0.0))), b"origin"), (dict(o=opt(origin=(float("inf"), 0.0, 0.0))), b"origin"),
           (dict(o=opt(mode=2)), b"mode"), (dict(o=opt(mode=-1)), b"mode"), (dict(o=opt(flags=1)), b"flag"),
           (dict(n_v=-1), b"counts"), (dict(n_t=-1), b"counts"), (dict(n_v=2**31), b"counts"),
           (dict(n_t=big, t=None), b"3 * n_triangles"), (dict(t=None), b"triangles must be given"),
           (dict(v=None), b"vertices must be given"), (dict(p_no=None), b"n_vertices_out"), (dict(p_to=None), b"n_vertices_out"),
           (dict(vcap=-1), b"cap"), (dict(tcap=-1), b"cap"), (dict(vo=None), b"cap"), (dict(to_=None), b"cap"),
           (dict(vo=dv.data_ptr()), b"equals an input"), (dict(to_=dt.data_ptr()), b"equals an input"),
           (dict(vm=dt.data_ptr()), b"equals an input"), (dict(tm=dv.data_ptr()), b"equals an input")]
    for kw, word in bad:
        assert call(**kw) == N.DP_E_ARG, kw
        assert word in lib.dp_last_error(ctx), (kw, lib.dp_last_error(ctx))
    # one below the 3T limit passes the count check and stops at the missing triangles
    assert call(n_t=big - 1, t=None) == N.DP_E_ARG and b"triangles must be given" in lib.dp_last_error(ctx)
    torch.cuda.synchronize()
    for b in (vb, tb, vmb, tmb):
        assert (b.cpu().numpy() == SENTINEL).all()
    assert (no.value, to.value) == (-7, -7)
    assert dv.cpu().numpy().tobytes() == verts.tobytes() and dt.cpu().numpy().tobytes() == tris.tobytes()
    # the host form: the same checks, and its result pointers
    pv, pt = ctypes.c_void_p(), ctypes.c_void_p()
    vm, tm = np.full(nv, 77, np.int32), np.full(nt, 77, np.int32)

    def host(o=good, v=N.ptr(verts), t=N.ptr(tris), p_pv=ctypes.byref(pv), p_no=ctypes.byref(no), p_pt=ctypes.byref(pt),
             p_to=ctypes.byref(to), vmap=N.ptr(vm), tmap=N.ptr(tm)):
        return lib.dp_mesh_decimate(ctx, ctypes.byref(o) if o is not None else None, v, nv, t, nt, p_pv, p_no, p_pt, p_to,
                                    vmap, tmap, None)

    for kw in (dict(o=None), dict(o=opt(cell=0.0)), dict(o=opt(mode=3)), dict(v=None), dict(t=None), dict(p_pv=None),
               dict(p_no=None), dict(p_pt=None), dict(p_to=None), dict(vmap=N.ptr(tris)), dict(tmap=N.ptr(verts))):
        assert host(**kw) == N.DP_E_ARG, kw
        assert lib.dp_last_error(ctx)
    assert (vm == 77).all() and (tm == 77).all() and (no.value, to.value) == (-7, -7)
    assert call() == N.DP_OK and host() == N.DP_OK and no.value == nv and to.value == nt  # one vertex per cell
    # the Python layer refuses before the library
    with pytest.raises(ValueError):
        eng.mesh_decimate(verts, tris, 0.0)
    with pytest.raises(ValueError):
        eng.mesh_decimate_device(dv.data_ptr(), nv, dt.data_ptr(), nt, None, 4, None, 0, 0.25)
