"""dp_mesh_nearest on the GPU against the brute-force CPU reference
(tests/meshnearest_ref.py, restated from the header's spec): index, dist,
closest, hist and every integer statistic bit for bit, in the host and the
device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import meshnearest_ref as MR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
CELL_CAP = 1 << 24  # the most cells the header lets the grid have


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


def search(eng, form, queries, vertices, triangles, max_dist, hist_bins=0, closest=True, want_hist=True):
    """mesh_nearest in either form as the dict Engine.mesh_nearest returns; the
    device form writes into sentinel-filled buffers with slack behind them and
    checks that nothing beyond the results and no input was written"""
    if form == "host":
        return eng.mesh_nearest(queries, vertices, triangles, max_dist, hist_bins, closest=closest)
    import torch

    qa, qp, nq, qs = pmvs._cloud_points("test", queries)
    verts = pmvs._mesh_vertices("test", vertices)
    tris = pmvs._mesh_triangles("test", triangles)
    nv, nt = len(verts), len(tris)
    dq = to_device(qa.reshape(-1)) if nq else None
    dv = to_device(verts) if nv else None
    dt = to_device(tris.reshape(-1)) if nt else None
    width = {"index": 4 * nq, "dist": 4 * nq, "closest": 12 * nq, "hist": 8 * hist_bins}
    bufs = {k: torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for k, n in width.items()}
    torch.cuda.synchronize()
    st = eng.mesh_nearest_device(dq.data_ptr() + (qp - qa.ctypes.data) if nq else None, nq, qs,
                                 dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt, max_dist,
                                 bufs["index"].data_ptr(), bufs["dist"].data_ptr(),
                                 bufs["closest"].data_ptr() if closest else None,
                                 bufs["hist"].data_ptr() if want_hist else None, hist_bins)
    torch.cuda.synchronize()
    out = {"stats": st, "hist": None, "closest": None}
    wanted = {"index": True, "dist": True, "closest": closest, "hist": bool(hist_bins) and want_hist}
    for k, dtype in (("index", np.int32), ("dist", np.float32), ("closest", np.float32), ("hist", np.uint64)):
        raw = bufs[k].cpu().numpy()
        n = width[k] if wanted[k] else 0
        assert (raw[n:] == SENTINEL).all(), k
        if wanted[k]:
            out[k] = raw[:n].view(dtype).copy()
    if closest:
        out["closest"] = out["closest"].reshape(-1, 3)
    if nq:
        assert dq.cpu().numpy().tobytes() == qa.tobytes()
    if nv:
        assert dv.cpu().numpy().tobytes() == verts.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == tris.tobytes()
    return out


def assert_equal(got, want, closest=True):
    assert MR.same_bits(got["index"], want["index"])
    assert MR.same_bits(got["dist"], want["dist"])
    if closest:
        assert MR.same_bits(got["closest"], want["closest"])
    else:
        assert got["closest"] is None
    assert (got["hist"] is None) == (want["hist"] is None)
    assert want["hist"] is None or MR.same_bits(got["hist"], want["hist"])
    st = got["stats"]
    assert {c: st[c] for c in MR.COUNTS} == want["stats"]
    part = want["stats"]["triangles"]
    assert 1 <= st["grid_cells"] <= CELL_CAP
    assert part <= st["grid_entries"] <= max(8 * (part + want["stats"]["invalid_triangles"]
                                                  + want["stats"]["degenerate_triangles"]
                                                  + want["stats"]["nonfinite_triangles"]), 0)
    assert 0 <= st["max_cell_entries"] <= part and (st["max_cell_entries"] > 0) == (part > 0)
    assert st["build_ms"] >= 0 and st["query_ms"] >= 0


def check(eng, queries, vertices, triangles, max_dist, hist_bins=0):
    """both forms against the reference (computed once); returns it and the last form's statistics"""
    want = MR.nearest(queries, vertices, triangles, max_dist, hist_bins)
    for form in FORMS:
        got = search(eng, form, queries, vertices, triangles, max_dist, hist_bins)
        assert_equal(got, want)
    return want, got["stats"]


def small_triangles(rng, n, size, lo=0.0, hi=1.0):
    """n triangles of about `size` across; every triangle has its own three vertices"""
    centre = rng.random((n, 1, 3)) * (hi - lo) + lo
    v = (centre + (rng.random((n, 3, 3)) - 0.5) * size).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


# ---- 1. random ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def unit_cube():
    rng = np.random.default_rng(20261022)
    v, t = small_triangles(rng, 2000, 0.06)
    q = rng.random((3000, 3), dtype=np.float32)
    return q, v, t, MR.nearest(q, v, t, 0.05, 16)


def test_random_unit_cube(eng, unit_cube):
    q, v, t, want = unit_cube
    for form in FORMS:
        assert_equal(search(eng, form, q, v, t, 0.05, 16), want)
        # without the closest points, and without the histogram
        assert_equal(search(eng, form, q, v, t, 0.05, 16, closest=False), want, closest=False)
    got = search(eng, "device", q, v, t, 0.05, 16, want_hist=False)
    assert got["hist"] is None and MR.same_bits(got["index"], want["index"])
    assert_equal(search(eng, "host", q, v, t, 0.05, 0), dict(want, hist=None))
    assert 1000 < want["stats"]["matched"] < 3000 and len(set(want["index"].tolist())) > 500
    assert set(want["label"][want["index"] >= 0].tolist()) == set(range(7))
    assert (want["hist"] > 0).sum() > 8 and int(want["hist"].sum()) == want["stats"]["matched"]


# ---- 2. the seven regions ----------------------------------------------------------

def test_every_region_of_a_triangle(eng):
    q, v, t, R, labels = MR.seven_region_case()
    want, _ = check(eng, q, v, t, R, 4)
    assert want["label"].tolist() == labels.tolist() and (want["index"] == 0).all()


# ---- 3. the inclusive radius across cell borders -----------------------------------

def border_case(beyond):
    """343 axis-aligned right triangles with legs of max_dist = 2^-3 in planes at
    multiples of 2^-10, five max_dist apart with up to one max_dist of jitter, so
    the extent stays under 40 max_dist and the grid keeps its smallest cells,
    whose borders (multiples of max_dist * (1 + 2^-19) from the box's corner) fall
    everywhere among them.  Three queries per triangle stand exactly max_dist from
    its face, from an edge and from a vertex -- or, with `beyond`, one float32
    step further."""
    R, step = np.float32(2.0 ** -3), 2.0 ** -10
    k = np.arange(343)
    base = np.stack([k % 7, (k // 7) % 7, k // 49], axis=1) * (5.0 * float(R))
    jitter = np.stack([(k * 37) % 128, (k * 91) % 128, (k * 53) % 128], axis=1) * step
    B = base + jitter + float(R) + 3 * step  # no query coordinate is 0: a float32 step from 0 is lost in fp64
    a, b, c = B.copy(), B + [float(R), 0, 0], B + [0, float(R), 0]
    face = B + [float(R) / 4, float(R) / 4, 0]
    edge = B + [float(R) / 2, 0, 0]
    vert = B.copy()
    sign = np.where(k % 2 == 0, 1.0, -1.0)
    face[:, 2] += sign * float(R)   # above or below the face
    edge[:, 1] -= float(R)          # beside the edge (a, b)
    vert[:, 0] -= float(R)          # beyond the vertex a, along the edge's line
    roll = k % 3                    # the plane's normal along z, x or y
    def turned(p):
        return np.stack([np.roll(p[i], roll[i]) for i in range(len(p))])
    tri = np.stack([turned(a), turned(b), turned(c)], axis=1)
    v = tri.reshape(-1, 3).astype(np.float32)
    assert (v.astype(np.float64) == tri.reshape(-1, 3)).all()
    q64 = np.concatenate([turned(face), turned(edge), turned(vert)])
    q = q64.astype(np.float32)
    assert (q.astype(np.float64) == q64).all()
    if beyond:
        moved = np.concatenate([(2 + roll) % 3, (1 + roll) % 3, (0 + roll) % 3])
        away = np.concatenate([sign, -np.ones(343), -np.ones(343)]).astype(np.float32)
        rows = np.arange(len(q))
        q[rows, moved] = np.nextafter(q[rows, moved], away * np.float32(np.inf))
    return q, v, np.arange(3 * 343, dtype=np.int32).reshape(343, 3), R


def test_inclusive_radius_across_cell_borders(eng):
    q, v, t, R = border_case(False)
    want, st = check(eng, q, v, t, R, 4)
    own = np.tile(np.arange(343), 3)
    # the reference says: everyone matched with its own triangle at exactly max_dist
    assert (want["index"] == own).all() and (want["d2"] == float(R) * float(R)).all() and (want["dist"] == R).all()
    assert want["label"].tolist() == [0] * 343 + [1] * 343 + [4] * 343
    assert want["hist"].tolist() == [0, 0, 0, 1029]
    # the cells are the smallest the grid makes: about 32 to an axis
    assert 31 ** 3 <= st["grid_cells"] <= 33 ** 3
    q, v, t, R = border_case(True)
    want, _ = check(eng, q, v, t, R, 4)
    assert (want["index"] == -1).all() and want["stats"]["unmatched"] == 1029


# ---- 4. one triangle across the whole box ------------------------------------------

@pytest.mark.parametrize("n_small", [10000, 200])
def test_one_triangle_spanning_the_box(eng, n_small):
    rng = np.random.default_rng(4)
    R = 0.005  # the cube is 200 smallest cells to an axis
    v, t = small_triangles(rng, n_small, 0.01)
    big = np.float32([[0, 0, 0], [1, 1, 0.25], [0, 1, 1]])
    at = n_small // 2
    v = np.concatenate([v, big])
    t = np.concatenate([t[:at], np.int32([[len(v) - 3, len(v) - 2, len(v) - 1]]), t[at:]])
    w = rng.dirichlet([1, 1, 1], 600)
    near = w @ big.astype(np.float64) + (rng.random((600, 3)) - 0.5) * R
    q = np.concatenate([rng.random((2000, 3)), near]).astype(np.float32)
    want, st = check(eng, q, v, t, R, 8)
    assert (want["index"] == at).sum() > 100 and (want["index"][:2000] >= 0).sum() > 10
    assert st["grid_entries"] <= 8 * len(t) and st["grid_cells"] <= CELL_CAP
    if n_small == 200:
        # the big triangle's own registrations are what bounds the level
        assert st["grid_cells"] <= 8 * len(t)


# ---- 5. extents much larger than the radius ------------------------------------------

def test_two_clusters_far_apart(eng):
    rng = np.random.default_rng(8)
    va, ta = small_triangles(rng, 400, 2e-3, 0.0, 0.01)
    vb, tb = small_triangles(rng, 400, 0.5, 0.0, 4.0)
    vb = (vb.astype(np.float64) + [1e6, 0, 0]).astype(np.float32)
    v, t = np.concatenate([va, vb]), np.concatenate([ta, tb + len(va)])
    t = t[rng.permutation(len(t))]
    between = np.stack([np.linspace(0.02, 1e6 - 1, 200), np.full(200, 0.005), np.full(200, 0.005)], axis=1)
    q = np.concatenate([(rng.random((400, 3)) * 0.012).astype(np.float32),
                        vb[rng.integers(0, len(vb), 400)] + (rng.random((400, 3)) * [0, 5e-4, 5e-4]).astype(np.float32),
                        between.astype(np.float32)])
    want, st = check(eng, q, v, t, 1e-3, 16)
    assert (want["index"][:400] >= 0).sum() > 100 and (want["index"][400:800] >= 0).sum() > 20
    assert (want["index"][800:] == -1).all() and st["grid_cells"] <= CELL_CAP
    # and far wider still: 3e38 apart at a radius of 1e-30
    tiny, tt = small_triangles(rng, 300, 2e-30, 0.0, 1e-29)
    v2 = np.concatenate([tiny, tiny + np.float32([0, 3e38, 0]), tiny - np.float32([0, 0, 3e38])])
    t2 = np.concatenate([tt, tt + len(tiny), tt + 2 * len(tiny)])
    q1 = (rng.random((400, 3)) * 1e-29).astype(np.float32)
    q2 = np.concatenate([q1, q1 + np.float32([0, 3e38, 0])])
    want, st = check(eng, q2, v2, t2, 1e-30)
    assert (want["index"][:400] >= 0).sum() > 50 and (want["index"][400:] >= 0).sum() > 50
    assert st["grid_cells"] <= CELL_CAP and st["grid_entries"] <= 8 * len(t2)


# ---- 6. a dense cell -----------------------------------------------------------------

def ball(rng, n, radius):
    p = rng.standard_normal((n, 3))
    p *= (rng.random((n, 1)) ** (1 / 3) * radius) / np.linalg.norm(p, axis=1, keepdims=True)
    return p


def test_dense_cell(eng):
    rng = np.random.default_rng(9)
    R = 0.05
    v = np.concatenate([ball(rng, 3000, R / 4) + 0.5, rng.random((300, 3))]).astype(np.float32)
    t = np.concatenate([rng.integers(0, 3000, (5000, 3)), rng.integers(3000, 3300, (100, 3))]).astype(np.int32)
    q = np.concatenate([ball(rng, 300, R / 4) + 0.5, rng.random((300, 3))]).astype(np.float32)
    want, st = check(eng, q, v, t[rng.permutation(len(t))], R, 64)
    assert st["max_cell_entries"] >= 4000 // 8 and (want["index"][:300] >= 0).all()


# ---- 7. triangles and queries that take no part ---------------------------------------

def test_mixed_classes_and_empty_sets(eng, unit_cube):
    q, v, t, _ = unit_cube
    rng = np.random.default_rng(12)
    v, t, q = v.copy(), t.copy(), q[:800].copy()
    nv = len(v)
    v[rng.choice(nv, 60, replace=False), rng.integers(0, 3, 60)] = np.float32([np.nan, np.inf, -np.inf])[np.arange(60) % 3]
    t[0:40, 1] = t[0:40, 0]                                   # degenerate
    t[40:80, 2] = np.int32([-1, nv, 2**31 - 1, -2**31])[np.arange(40) % 4]  # invalid
    t[80:120] = t[80:120, :1]                                 # all three equal
    # slivers: 1e-7 radians wide, and triangles whose positions coincide or are collinear
    for k in range(120, 160):
        a = v[t[k, 0]] = rng.random(3, dtype=np.float32) * np.float32([1, 0, 1])  # y = 0: 5e-9 is not lost beside it
        v[t[k, 1]] = a + np.float32([0.05, 0, 0])
        v[t[k, 2]] = a + np.float32([0.05, 5e-9, 0])
    for k in range(160, 180):
        v[t[k, 1]] = v[t[k, 2]] = v[t[k, 0]] = rng.random(3, dtype=np.float32)
    for k in range(180, 200):
        a = v[t[k, 0]] = rng.random(3, dtype=np.float32)
        v[t[k, 1]], v[t[k, 2]] = a + np.float32([0.01, 0.02, 0.03]), a + np.float32([0.02, 0.04, 0.06])
    q[100:140] = v[t[120:160, 0]] + np.float32([0.02, 0.001, 0.001])  # beside the slivers
    q[200 + rng.choice(600, 30, replace=False), rng.integers(0, 3, 30)] = \
        np.float32([np.nan, np.inf, -np.inf])[np.arange(30) % 3]
    want, _ = check(eng, q, v, t, 0.05, 16)
    s = want["stats"]
    assert s["skipped_queries"] == 30 and s["invalid_triangles"] == 40 and s["degenerate_triangles"] == 80
    assert s["nonfinite_triangles"] > 20 and s["triangles"] == 2000 - 120 - s["nonfinite_triangles"]
    assert len(set(range(120, 200)) & set(want["index"].tolist())) > 20
    assert np.isfinite(want["dist"][want["index"] >= 0]).all() and np.isfinite(want["closest"][want["index"] >= 0]).all()
    # nothing takes part; no triangles; no queries
    want, st = check(eng, q, v, t[:80], 0.05, 4)
    assert want["stats"]["triangles"] + want["stats"]["nonfinite_triangles"] == 0 and st["grid_entries"] == 0
    assert want["stats"]["unmatched"] == 770 and want["hist"].tolist() == [0] * 4
    empty_v, empty_t = np.zeros(0, dp.MESH_VERTEX_DTYPE), np.zeros((0, 3), np.int32)
    want, st = check(eng, q, empty_v, empty_t, 0.05, 4)
    assert want["stats"]["unmatched"] == 770 and st["max_cell_entries"] == 0
    want, _ = check(eng, np.zeros((0, 3), np.float32), v, t, 0.05, 4)
    assert len(want["index"]) == 0 and want["stats"]["triangles"] > 0
    check(eng, np.zeros((0, 3), np.float32), empty_v, empty_t, 0.05)
    check(eng, q, v, np.int32([[0, 1, 2]]), 0.05)  # vertices that no triangle names


# ---- 8. strides ----------------------------------------------------------------------

def test_strides(eng, unit_cube):
    q, v, t, want = unit_cube
    rng = np.random.default_rng(10)

    def noisy(dtype, pos):
        a = np.frombuffer(rng.integers(0, 256, len(pos) * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()
        a["pos"] = pos
        return a

    vr = noisy(dp.MESH_VERTEX_DTYPE, v)  # the colours are noise: only pos is read
    for qdtype, stride in ((dp.PATCH_DTYPE, 80), (dp.FUSED_DTYPE, 40), (dp.MESH_VERTEX_DTYPE, 16)):
        qr = noisy(qdtype, q)
        assert qr.dtype.itemsize == stride
        for form in FORMS:
            assert_equal(search(eng, form, qr, vr, t, 0.05, 16), want)
    for form in FORMS:
        assert_equal(search(eng, form, q, vr, t, 0.05, 16), want)  # packed xyz


# ---- 9. a permutation of the triangles -----------------------------------------------

def test_a_permutation_of_the_triangles_permutes_the_index(eng, unit_cube):
    q, v, t, want = unit_cube
    # no two candidates of a query tie in the reference, so the winner does not depend on the order
    hit = want["index"] >= 0
    perm = np.random.default_rng(11).permutation(len(t))
    again = MR.nearest(q, v, t[perm], 0.05, 16)
    assert MR.same_bits(again["d2"], want["d2"]) and (perm[again["index"][hit]] == want["index"][hit]).all()
    for form in FORMS:
        b = search(eng, form, q, v, t[perm], 0.05, 16)
        assert MR.same_bits(hit, b["index"] >= 0)
        assert (perm[b["index"][hit]] == want["index"][hit]).all()
        assert MR.same_bits(b["dist"], want["dist"]) and MR.same_bits(b["closest"], want["closest"])
        assert MR.same_bits(b["hist"], want["hist"])


# ---- 10. never farther than the nearest vertex ---------------------------------------

def assert_not_above_the_vertices(eng, q, v, t, max_dist):
    verts = pmvs._mesh_vertices("test", v)
    assert np.isfinite(verts["pos"]).all()
    cls = MR.classify(verts, t)
    named = np.unique(np.asarray(t)[cls == 0])
    mesh = eng.mesh_nearest(q, verts, t, max_dist)
    cloud = eng.cloud_nearest(q, verts[named], max_dist)
    assert (mesh["dist"] <= cloud["dist"]).all()
    assert (mesh["dist"] < cloud["dist"]).sum() > 0 and (cloud["index"] >= 0).sum() > 0
    return mesh, cloud


def test_never_farther_than_the_nearest_vertex(eng, unit_cube):
    q, v, t, _ = unit_cube
    assert_not_above_the_vertices(eng, q, v, t, 0.05)


def test_never_farther_than_the_nearest_vertex_of_a_tsdf_mesh(eng):
    from densepoints_amd import synth

    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    pm = dp.PMVS()
    for k in range(4):
        pm.add_camera(dp.View(P[k], synth.render_host(cfg, P, k)))
    seeds = synth.seeds(cfg, P)
    assert pm.run(seeds)
    v, t = pm.mesh(dim=40)
    assert len(t) > 1000
    voxel = float(pm.stats["mesh"]["voxel"])
    q = pm.patches["pos"]
    mesh, cloud = assert_not_above_the_vertices(eng, q, v, t, 4 * voxel)
    assert (mesh["index"] >= 0).sum() > len(q) // 2
    # mesh_compare and PMVS.evaluate agree, and the surface is never less complete than its vertices
    truth = np.ascontiguousarray(q[::3])
    got = dp.mesh_compare(eng, v, t, truth, voxel)
    assert pm.evaluate(truth, voxel, mesh=(v, t)) == got
    plain = dp.cloud_compare(eng, v, truth, voxel)
    assert got["accuracy"] == plain["accuracy"]
    assert got["completeness"]["within_tau"] >= plain["completeness"]["within_tau"] > 0
    dv, dt = pm.mesh(dim=40, decimate=dict(factor=2))
    dev = dp.mesh_deviation(eng, (v, t), (dv, dt), 4 * voxel)
    assert dev["a_to_b"]["n"] == len(v) and dev["b_to_a"]["n"] == len(dv)
    assert 0 < dev["b_to_a"]["mean"] <= dev["b_to_a"]["max"] <= dev["max"] <= 4 * voxel


# ---- 11. errors ------------------------------------------------------------------------

PTS = np.zeros((4, 3), np.float32)
VERTS = np.zeros(4, dp.MESH_VERTEX_DTYPE)
TRIS = np.int32([[0, 1, 2]])


def call(eng, q=PTS.ctypes.data, nq=4, qs=12, v=VERTS.ctypes.data, nv=4, t=TRIS.ctypes.data, nt=1, max_dist=0.5, bins=0,
         flags=0, opts=True, index=True, dist=True, closest=None, hist=None, device=False):
    """the raw library call; the device form is refused before any address is used"""
    mno = N.DpMeshNearestOptions(max_dist, bins, flags)
    pi, pd = ctypes.c_void_p(), ctypes.c_void_p()
    args = [eng._ctx, q, nq, qs, v, nv, t, nt, ctypes.byref(mno) if opts else None]
    if device:
        return N.lib.dp_mesh_nearest_device(*args, ctypes.c_void_p(4096) if index is True else index,
                                            ctypes.c_void_p(8192) if dist is True else dist, closest, hist, None, None)
    return N.lib.dp_mesh_nearest(*args, ctypes.byref(pi) if index else None, ctypes.byref(pd) if dist else None,
                                 closest, hist, None)


@pytest.mark.parametrize("device", [False, True], ids=FORMS)
def test_refusals_name_the_argument(eng, device):
    cases = [
        (dict(nq=-1), "n_queries"), (dict(nq=2**31), "n_queries"), (dict(nv=-1), "n_vertices"),
        (dict(nv=2**31), "n_vertices"), (dict(nt=-1), "n_triangles"), (dict(nt=2**31), "n_triangles"),
        (dict(q=None), "queries"), (dict(v=None), "vertices"), (dict(t=None), "triangles"),
        (dict(qs=8), "query_stride"), (dict(qs=10), "query_stride"), (dict(qs=0), "query_stride"),
        (dict(opts=False), "opts"), (dict(max_dist=0.0), "max_dist"), (dict(max_dist=-1.0), "max_dist"),
        (dict(max_dist=float("inf")), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
        (dict(bins=-1), "hist_bins"), (dict(bins=65537), "hist_bins"), (dict(flags=1), "flags"),
        (dict(index=None), "index"), (dict(dist=None), "dist"),
    ]
    for kw, name in cases:
        assert call(eng, device=device, **kw) == N.DP_E_ARG, kw
        msg = N.lib.dp_last_error(eng._ctx).decode()
        assert msg.startswith("dp_mesh_nearest_device:" if device else "dp_mesh_nearest:") and name in msg, (kw, msg)
    for same in (PTS.ctypes.data, VERTS.ctypes.data, TRIS.ctypes.data):
        same = ctypes.c_void_p(same)
        if device:
            assert call(eng, device=True, index=same) == N.DP_E_ARG
        assert call(eng, device=device, closest=same) == N.DP_E_ARG
        assert call(eng, device=device, hist=same, bins=4) == N.DP_E_ARG
        assert "output" in N.lib.dp_last_error(eng._ctx).decode()
    # zero counts with NULL arrays are legal
    assert call(eng, device=device, q=None, nq=0, v=None, nv=0, t=None, nt=0, index=None if device else True,
                dist=None if device else True) == N.DP_OK


def test_python_layer_refuses_before_the_library(eng):
    for kw in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(hist_bins=-1), dict(hist_bins=65537)):
        with pytest.raises(ValueError):
            eng.mesh_nearest(PTS, VERTS, TRIS, **dict(dict(max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.mesh_nearest(np.zeros((4, 2), np.float32), VERTS, TRIS, 0.5)
    with pytest.raises(ValueError):
        eng.mesh_nearest(PTS, VERTS, np.zeros((2, 2), np.int32), 0.5)
    with pytest.raises(ValueError):
        eng.mesh_nearest_device(64, 3, 12, 128, 3, 256, 1, 0.5, 128, 512)  # an output equals an input
    with pytest.raises(ValueError):
        eng.mesh_nearest_device(64, 3, 12, 128, 3, 256, 1, 0.5, 0, 512)  # no d_index
    with pytest.raises(ValueError):
        eng.mesh_nearest_device(64, 3, 12, 0, 3, 256, 1, 0.5, 1024, 512)  # no vertices
