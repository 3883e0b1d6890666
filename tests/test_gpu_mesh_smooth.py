"""dp_mesh_adjacency, dp_mesh_smooth and dp_mesh_normals on the GPU against the
CPU reference (tests/meshsmooth_ref.py, restated from the header's spec): every
byte of the CSR arrays, the flags, the smoothed records and the normals, the
counts and the integer statistics, in the host and the device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import MESH_VERTEX_DTYPE
from densepoints_amd import _native as N

import meshsmooth_ref as SR
import tsdf_ref as TR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]


@pytest.fixture(scope="module")
def eng():
    # no views are set: none of the calls reads one
    with dp.Engine(device=0) as e:
        yield e


def device_buffer(records, size):
    import torch

    return torch.full(((records + 3) * size,), SENTINEL, dtype=torch.uint8, device="cuda")


def pick(stats, names):
    return {c: stats[c] for c in names}


def adjacency(eng, form, tris, nv, cap=None, skip=()):
    """mesh_adjacency in either form; the device form checks the sentinels
    beyond min(cap, E) entries and beyond the arrays, and leaves out the
    outputs named in `skip` (they must stay untouched)"""
    tris = SR.as_triangles(tris)
    if form == "host":
        got = eng.mesh_adjacency(tris, nv)
        return dict(got, n_entries=len(got["neighbours"]))
    import torch

    nt = len(tris)
    cap = 6 * nt if cap is None else cap
    dt = to_device(tris) if nt else None
    bufs = dict(offsets=device_buffer(nv + 1, 4), neighbours=device_buffer(cap, 4), edge_triangles=device_buffer(cap, 4),
                vertex_flags=device_buffer(nv, 1))
    torch.cuda.synchronize()
    arg = {k: (None if k in skip else b.data_ptr()) for k, b in bufs.items()}
    E, st = eng.mesh_adjacency_device(dt.data_ptr() if nt else None, nt, nv, arg["offsets"], arg["neighbours"],
                                      arg["edge_triangles"], cap, arg["vertex_flags"])
    raw = {k: b.cpu().numpy() for k, b in bufs.items()}
    n = min(E, cap)
    used = dict(offsets=(nv + 1) * 4, neighbours=n * 4, edge_triangles=n * 4, vertex_flags=nv)
    for k in raw:
        assert (raw[k][(0 if k in skip else used[k]):] == SENTINEL).all(), k
    return dict(offsets=raw["offsets"][:used["offsets"]].view(np.int32).copy(),
                neighbours=raw["neighbours"][:n * 4].view(np.int32).copy(),
                edge_triangles=raw["edge_triangles"][:n * 4].view(np.int32).copy(),
                vertex_flags=raw["vertex_flags"][:nv].copy(), stats=st, n_entries=E)


def smooth(eng, form, verts, tris, stats=True, **opts):
    verts, tris = np.ascontiguousarray(verts, dtype=MESH_VERTEX_DTYPE), SR.as_triangles(tris)
    nv, nt = len(verts), len(tris)
    if form == "host":
        out, st = eng.mesh_smooth(verts, tris, **opts)
        return dict(vertices=out, stats=st)
    import torch

    dv, dt = (to_device(verts) if nv else None), (to_device(tris) if nt else None)
    ob = device_buffer(nv, 16)
    torch.cuda.synchronize()
    st = eng.mesh_smooth_device(dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt,
                                ob.data_ptr() if nv else None, stats=stats, **opts)
    torch.cuda.synchronize()
    raw = ob.cpu().numpy()
    assert (raw[nv * 16:] == SENTINEL).all()
    if nv:  # the input is read only
        assert dv.cpu().numpy().tobytes() == verts.tobytes()
    return dict(vertices=raw[:nv * 16].view(MESH_VERTEX_DTYPE).copy(), stats=st)


def normals(eng, form, verts, tris, stats=True):
    verts, tris = np.ascontiguousarray(verts, dtype=MESH_VERTEX_DTYPE), SR.as_triangles(tris)
    nv, nt = len(verts), len(tris)
    if form == "host":
        out, st = eng.mesh_normals(verts, tris)
        return dict(normals=out, stats=st)
    import torch

    dv, dt = (to_device(verts) if nv else None), (to_device(tris) if nt else None)
    ob = device_buffer(nv, 12)
    torch.cuda.synchronize()
    st = eng.mesh_normals_device(dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt,
                                 ob.data_ptr() if nv else None, stats=stats)
    torch.cuda.synchronize()
    raw = ob.cpu().numpy()
    assert (raw[nv * 12:] == SENTINEL).all()
    return dict(normals=raw[:nv * 12].view(np.float32).reshape(-1, 3).copy(), stats=st)


def assert_adjacency(got, want):
    assert pick(got["stats"], SR.ADJ_COUNTS) == want["stats"]
    assert got["n_entries"] == len(want["neighbours"])
    for k in ("offsets", "neighbours", "edge_triangles", "vertex_flags"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def check_all(eng, form, verts, tris, **opts):
    """the three calls against the reference on one mesh; returns (got, want) of the smoothing"""
    assert_adjacency(adjacency(eng, form, tris, len(verts)), SR.adjacency(tris, len(verts)))
    got, want = smooth(eng, form, verts, tris, **opts), SR.smooth(verts, tris, **opts)
    assert pick(got["stats"], SR.SMOOTH_COUNTS) == want["stats"]
    assert got["vertices"].tobytes() == want["vertices"].tobytes()
    gn, wn = normals(eng, form, verts, tris), SR.normals(verts, tris)
    assert pick(gn["stats"], SR.NORMAL_COUNTS) == wn["stats"]
    assert gn["normals"].tobytes() == wn["normals"].tobytes()
    return got, want


HAND = {
    "triangle": ([(0, 1, 2)], 3),
    "shared_edge": ([(0, 1, 2), (2, 1, 3)], 4),
    "tetrahedron": ([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], 4),
    "bow_tie": ([(0, 1, 2), (2, 3, 4)], 5),
    "three_on_an_edge": ([(0, 1, 2), (0, 1, 3), (1, 0, 4)], 5),
    "mixed": ([(0, 1, 1), (2, 2, 2), (-1, 0, 1), (0, 1, 6), (3, 4, 5), (3, 4, 5), (5, 3, 4)], 6),
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_meshes(eng, form, name):
    tris, nv = HAND[name]
    got, _ = check_all(eng, form, SR.random_vertices(nv, 21), tris, iterations=2)
    assert got["stats"]["adjacency_ms"] > 0 and got["stats"]["smooth_ms"] > 0


@pytest.mark.parametrize("form", FORMS)
def test_empty_and_all_refused(eng, form):
    """n_triangles = 0, n_vertices = 0, and meshes whose triangles are all invalid or degenerate"""
    for nv, tris in ((0, []), (5, []), (0, [(0, 0, 0), (0, 1, 2)]), (4, [(0, 1, 4), (-1, 2, 3)]),
                     (4, [(0, 0, 1), (2, 3, 3), (1, 1, 1)])):
        verts = SR.random_vertices(nv, 4)
        got, want = check_all(eng, form, verts, tris, iterations=1)
        assert want["stats"]["isolated_vertices"] == nv and want["stats"]["edges"] == 0
        assert got["vertices"].tobytes() == verts.tobytes()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [65, 130])
def test_fans(eng, form, n):
    """a row longer than a wave, and one longer than two: the step's loop"""
    tris, nv = SR.fan(n)
    _, want = check_all(eng, form, SR.random_vertices(nv, n), tris, iterations=2, free_boundary=True)
    assert want["stats"]["max_valence"] == n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("free", [False, True])
def test_grid_sheet(eng, form, free):
    """a 17 x 17 sheet: 64 pinned border vertices, or none with FREE_BOUNDARY"""
    tris, nv = SR.grid_sheet(17)
    verts = SR.grid_vertices(17, 8)
    got, want = check_all(eng, form, verts, tris, iterations=3, free_boundary=free)
    assert want["stats"]["pinned_vertices"] == (0 if free else 64) and want["stats"]["boundary_vertices"] == 64
    border = SR.adjacency(tris, nv)["vertex_flags"] & 1 != 0
    assert (got["vertices"][border].tobytes() == verts[border].tobytes()) == (not free)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nv", [44, 45, 255, 256, 257])
def test_block_edges(eng, form, nv):
    """strips of 255, 256 and 257 vertices (the vertex kernels' block edge), and
    of 44 and 45 vertices: 42 and 43 triangles, 252 and 258 keys around the block
    of the count / scan / emit"""
    tris, _ = SR.strip(nv)
    assert nv > 45 or 6 * len(tris) in (252, 258)
    check_all(eng, form, SR.random_vertices(nv, nv), tris, iterations=1)


@pytest.fixture(scope="module")
def sphere():
    """the sphere of a 16^3 volume with vertex noise of a fifth of a voxel (some
    triangle names the index n_vertices - 1), in the extracted triangle order and
    shuffled"""
    vol, _ = SR.sphere_volume(16)
    m = TR.mesh(vol["tsdf"], vol["weight"], None, origin=vol["origin"], voxel=vol["voxel"], dim=vol["dim"])
    verts = SR.noisy(m["vertices"].astype(MESH_VERTEX_DTYPE), 0.2 * vol["voxel"], 16)
    tris = SR.as_triangles(m["triangles"])
    assert (tris == len(verts) - 1).any()
    rng = np.random.default_rng(5)
    return verts, tris, tris[rng.permutation(len(tris))]


@pytest.fixture(scope="module")
def sphere_want(sphere):
    verts, tris, shuffled = sphere
    return {k: (SR.smooth(verts, t, iterations=3), SR.normals(verts, t), SR.adjacency(t, len(verts)))
            for k, t in (("ordered", tris), ("shuffled", shuffled))}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ["ordered", "shuffled"])
def test_noisy_sphere(eng, form, sphere, sphere_want, order):
    """the closed sphere, its highest vertex index named, in the extracted and
    in a shuffled triangle order.  The adjacency and the smoothed positions do not
    depend on the triangle order (rows are sorted sets); the normals may, by design:
    their sum follows the triangle index, so each order has its own reference."""
    verts, tris, shuffled = sphere
    t = tris if order == "ordered" else shuffled
    ws, wn, wa = sphere_want[order]
    assert wa["stats"]["boundary_edges"] == 0 and wa["stats"]["isolated_vertices"] == 0
    assert_adjacency(adjacency(eng, form, t, len(verts)), wa)
    got = smooth(eng, form, verts, t, iterations=3)
    assert pick(got["stats"], SR.SMOOTH_COUNTS) == ws["stats"]
    assert got["vertices"].tobytes() == ws["vertices"].tobytes()
    assert got["vertices"].tobytes() == sphere_want["ordered"][0]["vertices"].tobytes()
    gn = normals(eng, form, verts, t)
    assert pick(gn["stats"], SR.NORMAL_COUNTS) == wn["stats"]
    assert gn["normals"].tobytes() == wn["normals"].tobytes()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("opts", [dict(iterations=0), dict(iterations=1), dict(iterations=3), dict(iterations=2, mu=0.0),
                                  dict(iterations=2, lam=1.0), dict(iterations=2, lam=0.33, mu=-0.34)],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_smooth_options(eng, form, opts):
    tris, nv = SR.grid_sheet(6)
    verts = SR.grid_vertices(6, 9)
    got, want = smooth(eng, form, verts, tris, free_boundary=True, **opts), SR.smooth(verts, tris, free_boundary=True, **opts)
    assert pick(got["stats"], SR.SMOOTH_COUNTS) == want["stats"]
    assert got["vertices"].tobytes() == want["vertices"].tobytes()
    if opts["iterations"] == 0:
        assert got["vertices"].tobytes() == verts.tobytes() and want["stats"]["steps"] == 0


def test_entry_cap_overflow(eng):
    """a neighbour cap below the entries: the full count is reported, the first
    cap entries are written and nothing beyond them"""
    tris, nv = SR.grid_sheet(5)
    want = SR.adjacency(tris, nv)
    E = len(want["neighbours"])
    for cap in (0, 1, E - 1, E, E + 5):
        got = adjacency(eng, "device", tris, nv, cap=cap)
        assert got["n_entries"] == E and pick(got["stats"], SR.ADJ_COUNTS) == want["stats"]
        n = min(cap, E)
        assert got["neighbours"].tobytes() == want["neighbours"][:n].tobytes()
        assert got["edge_triangles"].tobytes() == want["edge_triangles"][:n].tobytes()
        assert got["offsets"].tobytes() == want["offsets"].tobytes()
        assert got["vertex_flags"].tobytes() == want["vertex_flags"].tobytes()


@pytest.mark.parametrize("skip", ["offsets", "neighbours", "edge_triangles", "vertex_flags"])
def test_outputs_null_one_at_a_time(eng, skip):
    tris, nv = SR.grid_sheet(5)
    want = SR.adjacency(tris, nv)
    got = adjacency(eng, "device", tris, nv, skip=(skip,))
    assert got["n_entries"] == len(want["neighbours"]) and pick(got["stats"], SR.ADJ_COUNTS) == want["stats"]
    for k in ("offsets", "neighbours", "edge_triangles", "vertex_flags"):
        if k != skip:
            assert got[k].tobytes() == want[k].tobytes(), k


def test_host_outputs_null_and_stats_null(eng):
    """the host form with every result pointer NULL but the count; stats NULL in every call"""
    tris, nv = SR.grid_sheet(5)
    verts = SR.grid_vertices(5, 3)
    ne = ctypes.c_int64()
    N.check(N.lib.dp_mesh_adjacency(eng._ctx, N.ptr(tris), len(tris), nv, None, None, None, None, ctypes.byref(ne), None),
            eng._ctx)
    assert ne.value == len(SR.adjacency(tris, nv)["neighbours"])
    for form in ("device",):
        got = smooth(eng, form, verts, tris, stats=False, iterations=2)
        assert got["stats"] is None and got["vertices"].tobytes() == SR.smooth(verts, tris, iterations=2)["vertices"].tobytes()
        gn = normals(eng, form, verts, tris, stats=False)
        assert gn["stats"] is None and gn["normals"].tobytes() == SR.normals(verts, tris)["normals"].tobytes()
    pv = ctypes.c_void_p()
    N.check(N.lib.dp_mesh_smooth(eng._ctx, None, N.ptr(verts), nv, N.ptr(tris), len(tris), ctypes.byref(pv), None), eng._ctx)
    out = np.zeros(nv, MESH_VERTEX_DTYPE)
    ctypes.memmove(out.ctypes.data, pv.value, out.nbytes)
    assert out.tobytes() == SR.smooth(verts, tris)["vertices"].tobytes()  # NULL options: the defaults


def test_refusals(eng):
    import torch

    tris, nv = SR.grid_sheet(4)
    dv, dt = to_device(SR.grid_vertices(4, 1)), to_device(tris)
    torch.cuda.synchronize()
    lib, ctx = N.lib, eng._ctx
    # equal in and out pointers
    assert lib.dp_mesh_smooth_device(ctx, None, dv.data_ptr(), nv, dt.data_ptr(), len(tris), dv.data_ptr(), None,
                                     None) == N.DP_E_ARG
    assert b"output pointer equals an input pointer" in lib.dp_last_error(ctx)
    assert lib.dp_mesh_normals_device(ctx, dv.data_ptr(), nv, dt.data_ptr(), len(tris), dv.data_ptr(), None,
                                      None) == N.DP_E_ARG
    ne = ctypes.c_int64()
    assert lib.dp_mesh_adjacency_device(ctx, dt.data_ptr(), len(tris), nv, dt.data_ptr(), None, None, 0, None,
                                        ctypes.byref(ne), None, None) == N.DP_E_ARG
    # the 6T limit, by count only: the argument check precedes the pointer check
    big = (2**31 - 1) // 6 + 1
    assert lib.dp_mesh_adjacency_device(ctx, None, big, nv, None, None, None, 0, None, ctypes.byref(ne), None,
                                        None) == N.DP_E_ARG
    assert b"6 * n_triangles" in lib.dp_last_error(ctx)
    assert lib.dp_mesh_adjacency(ctx, None, big, nv, None, None, None, None, ctypes.byref(ne), None) == N.DP_E_ARG
    assert b"6 * n_triangles" in lib.dp_last_error(ctx)
    assert lib.dp_mesh_smooth_device(ctx, None, None, nv, None, big, None, None, None) == N.DP_E_ARG
    assert b"6 * n_triangles" in lib.dp_last_error(ctx)
    # one below the limit passes the count check and stops at the missing triangles
    assert lib.dp_mesh_adjacency_device(ctx, None, big - 1, nv, None, None, None, 0, None, ctypes.byref(ne), None,
                                        None) == N.DP_E_ARG
    assert b"triangles must be given" in lib.dp_last_error(ctx)
    # options the Python check would stop: through the struct
    ob = device_buffer(nv, 16)
    for o in (N.DpMeshSmoothOptions(-1, 0.5, -0.53, 0, 0), N.DpMeshSmoothOptions(1001, 0.5, -0.53, 0, 0),
              N.DpMeshSmoothOptions(1, 0.0, -0.53, 0, 0), N.DpMeshSmoothOptions(1, float("nan"), -0.53, 0, 0),
              N.DpMeshSmoothOptions(1, 0.5, 0.1, 0, 0), N.DpMeshSmoothOptions(1, 0.5, float("nan"), 0, 0),
              N.DpMeshSmoothOptions(1, 0.5, -0.53, 2, 0)):
        assert lib.dp_mesh_smooth_device(ctx, ctypes.byref(o), dv.data_ptr(), nv, dt.data_ptr(), len(tris),
                                         ob.data_ptr(), None, None) == N.DP_E_ARG
    torch.cuda.synchronize()
    assert (ob.cpu().numpy() == SENTINEL).all()
    assert lib.dp_mesh_adjacency_device(ctx, dt.data_ptr(), len(tris), nv, None, None, None, -1, None, ctypes.byref(ne),
                                        None, None) == N.DP_E_ARG
    assert lib.dp_mesh_adjacency_device(ctx, dt.data_ptr(), len(tris), nv, None, None, None, 0, None, None, None,
                                        None) == N.DP_E_ARG


def test_device_chain_equals_host_pipeline(eng):
    """tsdf_mesh_device -> mesh_clean_device -> mesh_smooth_device -> mesh_normals_device
    on the 16^3 sphere, the mesh never leaving the device, against the host calls"""
    import torch

    vol, _ = SR.sphere_volume(16)
    hv, ht, _ = eng.tsdf_mesh(dict(vol, rgb=None), 1)
    hv, ht, _ = eng.mesh_clean(hv, ht)
    hs, hst = eng.mesh_smooth(hv, ht, iterations=3)
    hn, hnst = eng.mesh_normals(hs, ht)
    assert len(hv) > 256 and hst["boundary_edges"] == 0

    cap_v, cap_t = len(hv) + 8, len(ht) + 8
    d_tsdf, d_w = to_device(vol["tsdf"]), to_device(vol["weight"])
    v0, t0, v1, t1 = device_buffer(cap_v, 16), device_buffer(cap_t, 12), device_buffer(cap_v, 16), device_buffer(cap_t, 12)
    v2, nb = device_buffer(cap_v, 16), device_buffer(cap_v, 12)
    torch.cuda.synchronize()
    nv, nt, _ = eng.tsdf_mesh_device(d_tsdf.data_ptr(), d_w.data_ptr(), None, v0.data_ptr(), cap_v, t0.data_ptr(), cap_t,
                                     origin=vol["origin"], voxel=vol["voxel"], dim=vol["dim"], trunc=vol["trunc"],
                                     min_weight=1)
    nv, nt, _ = eng.mesh_clean_device(v0.data_ptr(), nv, t0.data_ptr(), nt, v1.data_ptr(), cap_v, t1.data_ptr(), cap_t)
    assert (nv, nt) == (len(hv), len(ht))
    st = eng.mesh_smooth_device(v1.data_ptr(), nv, t1.data_ptr(), nt, v2.data_ptr(), iterations=3)
    nst = eng.mesh_normals_device(v2.data_ptr(), nv, t1.data_ptr(), nt, nb.data_ptr())
    torch.cuda.synchronize()
    assert pick(st, SR.SMOOTH_COUNTS) == pick(hst, SR.SMOOTH_COUNTS) and pick(nst, SR.NORMAL_COUNTS) == pick(hnst, SR.NORMAL_COUNTS)
    assert v2.cpu().numpy()[:nv * 16].tobytes() == hs.tobytes()
    assert nb.cpu().numpy()[:nv * 12].tobytes() == hn.tobytes()
    assert (v2.cpu().numpy()[nv * 16:] == SENTINEL).all() and (nb.cpu().numpy()[nv * 12:] == SENTINEL).all()
