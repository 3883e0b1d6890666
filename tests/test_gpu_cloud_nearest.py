"""dp_cloud_nearest on the GPU against the brute-force CPU reference
(tests/cloudnearest_ref.py, restated from the header's spec): index, dist, hist
and every integer statistic bit for bit, in the host and the device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudnearest_ref as CR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
CELL_CAP = 1 << 24  # the most cells the header lets the grid have
F32_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


def search(eng, form, queries, targets, max_dist, hist_bins=0, want_hist=True):
    """cloud_nearest in either form as the dict Engine.cloud_nearest returns;
    the device form writes into sentinel-filled buffers with slack behind them
    and checks that nothing beyond the results and no input was written"""
    if form == "host":
        return eng.cloud_nearest(queries, targets, max_dist, hist_bins)
    import torch

    qa, qp, nq, qs = pmvs._cloud_points("test", queries)
    ta, tp, nt, ts = pmvs._cloud_points("test", targets)
    dq = to_device(qa.reshape(-1)) if nq else None
    dt = to_device(ta.reshape(-1)) if nt else None
    width = {"index": 4 * nq, "dist": 4 * nq, "hist": 8 * hist_bins}
    bufs = {k: torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for k, n in width.items()}
    torch.cuda.synchronize()
    st = eng.cloud_nearest_device(dq.data_ptr() + (qp - qa.ctypes.data) if nq else None, nq, qs,
                                  dt.data_ptr() + (tp - ta.ctypes.data) if nt else None, nt, ts, max_dist,
                                  bufs["index"].data_ptr(), bufs["dist"].data_ptr(),
                                  bufs["hist"].data_ptr() if want_hist else None, hist_bins)
    torch.cuda.synchronize()
    out = {"stats": st, "hist": None}
    for k, dtype in (("index", np.int32), ("dist", np.float32), ("hist", np.uint64)):
        raw = bufs[k].cpu().numpy()
        n = width[k] if k != "hist" or want_hist else 0
        assert (raw[n:] == SENTINEL).all(), k
        if k != "hist" or (hist_bins and want_hist):
            out[k] = raw[:n].view(dtype).copy()
    if nq:
        assert dq.cpu().numpy().tobytes() == qa.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == ta.tobytes()
    return out


def assert_equal(got, want):
    assert CR.same_bits(got["index"], want["index"])
    assert CR.same_bits(got["dist"], want["dist"])
    assert (got["hist"] is None) == (want["hist"] is None)
    assert want["hist"] is None or CR.same_bits(got["hist"], want["hist"])
    st = got["stats"]
    assert {c: st[c] for c in CR.COUNTS} == want["stats"]
    assert 1 <= st["grid_cells"] <= CELL_CAP and 0 <= st["max_cell_targets"] <= want["stats"]["targets"]
    assert (st["max_cell_targets"] > 0) == (want["stats"]["targets"] > 0)
    assert st["build_ms"] >= 0 and st["query_ms"] >= 0


def check(eng, queries, targets, max_dist, hist_bins=0):
    """both forms against the reference (computed once); returns it and the host form's statistics"""
    want = CR.nearest(queries, targets, max_dist, hist_bins)
    for form in FORMS:
        got = search(eng, form, queries, targets, max_dist, hist_bins)
        assert_equal(got, want)
    return want, got["stats"]


# ---- 1. random ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def unit_cube():
    rng = np.random.default_rng(20261021)
    return rng.random((3000, 3), dtype=np.float32), rng.random((2500, 3), dtype=np.float32)


def test_random_unit_cube(eng, unit_cube):
    q, t = unit_cube
    want, st = check(eng, q, t, 0.1, 32)
    assert want["stats"]["matched"] > 2900 and 27 < st["grid_cells"] <= 11 ** 3 and st["max_cell_targets"] < 50
    assert len(set(want["index"].tolist())) > 1000
    assert (want["hist"] > 0).sum() > 16 and int(want["hist"].sum()) == want["stats"]["matched"]


def test_random_one_cell(eng, unit_cube):
    q, t = unit_cube
    want, st = check(eng, q, t, 2.0, 32)
    assert want["stats"]["matched"] == 3000 and st["grid_cells"] == 1 and st["max_cell_targets"] == 2500


# ---- 2. ties -----------------------------------------------------------------------

def lattice(n, step, origin=0.0):
    g = np.arange(n, dtype=np.float64) * step + origin
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def test_ties_go_to_the_lowest_index(eng):
    rng = np.random.default_rng(7)
    base = lattice(8, 2.0 ** -4)  # 512 targets, every one twice
    order = rng.permutation(1024)
    t = np.concatenate([base, base])[order]
    # the midpoints of x-neighbours: two pairs of duplicates at the same distance
    q = base[base[:, 0] < 7 * 2.0 ** -4] + np.float32([2.0 ** -5, 0, 0])
    want, _ = check(eng, q, t, 0.25, 8)
    first = {}
    for i, p in enumerate(map(tuple, t)):
        first.setdefault(p, i)
    for qi, p in enumerate(q):
        a, b = (p[0] - 2.0 ** -5, p[1], p[2]), (p[0] + 2.0 ** -5, p[1], p[2])
        assert want["index"][qi] == min(first[a], first[b]) and want["dist"][qi] == np.float32(2.0 ** -5)


def test_a_permutation_of_the_targets_permutes_the_index(eng, unit_cube):
    q, t = unit_cube  # random floats: no two d2 tie
    perm = np.random.default_rng(11).permutation(len(t))
    a = search(eng, "host", q, t, 0.1, 16)
    for form in FORMS:
        b = search(eng, form, q, t[perm], 0.1, 16)
        hit = a["index"] >= 0
        assert CR.same_bits(hit, b["index"] >= 0)
        assert (perm[b["index"][hit]] == a["index"][hit]).all()
        assert CR.same_bits(a["dist"], b["dist"]) and CR.same_bits(a["hist"], b["hist"])


# ---- 3. the inclusive radius across cell borders -----------------------------------

def border_pairs(beyond):
    """4,096 queries at multiples of 2^-10 from an origin that is no multiple of
    max_dist = 2^-3, each with one partner exactly max_dist away along +-x, y or
    z -- or, with `beyond`, one float32 step further.  The queries stand 2.5
    max_dist apart with less than 0.25 max_dist of jitter, so a partner is more
    than max_dist from every query but its own, and the extent is under 40
    max_dist: the grid keeps its smallest cells."""
    step, R = 2.0 ** -10, np.float32(2.0 ** -3)
    k = np.arange(4096)
    axis, sign = k % 3, np.where((k // 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    base = np.stack([k % 16, (k // 16) % 16, k // 256], axis=1).astype(np.float64) * (320 * step)
    jitter = np.stack([(k * 37) % 32, (k * 91) % 32, (k * 53) % 32], axis=1) * step
    q = (base + jitter + 5 * step).astype(np.float32)
    assert (q.astype(np.float64) == base + jitter + 5 * step).all()
    t = q.copy()
    t[k, axis] = q[k, axis] + sign * R  # exact in float32
    if beyond:
        t[k, axis] = np.nextafter(t[k, axis], sign * np.float32(np.inf))
    return q, t


def test_inclusive_radius_across_cell_borders(eng):
    R = np.float32(2.0 ** -3)
    q, t = border_pairs(False)
    # exact: the partners are representable, so d2 == R2
    d = np.abs(q.astype(np.float64) - t.astype(np.float64)).sum(axis=1)
    assert (d == float(R)).all()
    want, st = check(eng, q, t, R, 4)
    assert (want["index"] == np.arange(4096)).all() and (want["dist"] == R).all()
    # the cells are the smallest the grid makes: 40 to an axis
    assert want["hist"].tolist() == [0, 0, 0, 4096] and 39 ** 3 <= st["grid_cells"] <= 40 ** 3
    # one float32 step further apart: nobody matches
    q, t = border_pairs(True)
    d = np.abs(q.astype(np.float64) - t.astype(np.float64)).sum(axis=1)
    assert (d > float(R)).all() and (d < float(R) * (1 + 2.0 ** -16)).all()
    want, _ = check(eng, q, t, R, 4)
    assert (want["index"] == -1).all() and want["stats"]["unmatched"] == 4096


# ---- 4. outside the box ------------------------------------------------------------

def test_queries_outside_the_box(eng):
    R = 0.25
    rng = np.random.default_rng(3)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    t = np.concatenate([corners, rng.random((600, 3), dtype=np.float32),
                        np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]])])
    out = np.where(corners > 0, 1.0, -1.0)
    q = []
    for reach in (0.1, 0.2, 0.3, 0.6):
        # beyond the corners along one, two and three axes: faces, edges, corners
        for mask in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]):
            q.append(corners + out * np.float32(mask) * reach)
    far = []
    for axis in range(3):
        for v in (1e30, -1e30, np.inf, -np.inf, np.nan, F32_MAX, -F32_MAX):
            p = [0.5, 0.5, 0.5]
            p[axis] = v
            far.append(p)
    q = np.concatenate(q + [np.float32(far), np.float32([[1e30, -1e30, 1e30], [F32_MAX] * 3])]).astype(np.float32)
    want, _ = check(eng, q, t, R, 16)
    n = len(corners)
    assert (want["index"][:7 * n] >= 0).all()  # reach 0.1: within max_dist of a corner target
    assert (want["index"][7 * n:14 * n].reshape(7, n)[:3] >= 0).all()  # reach 0.2 along one axis
    assert (want["index"][21 * n:28 * n] == -1).all()  # reach 0.6: beyond
    assert (want["index"][28 * n:] == -1).all()
    assert want["stats"]["skipped_queries"] == 9 and want["stats"]["skipped_targets"] == 3


# ---- 5. degenerate extents ---------------------------------------------------------

@pytest.mark.parametrize("shape", ["one", "identical", "coplanar", "collinear", "non_finite"])
def test_degenerate_extents(eng, shape):
    rng = np.random.default_rng(5)
    q = (rng.random((700, 3), dtype=np.float32) - np.float32(0.25)) * np.float32(2)
    t = rng.random((900, 3), dtype=np.float32)
    q[:50] = t[0] + (rng.random((50, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.2)  # within 0.18 of t[0]
    if shape == "one":
        t = t[:1]
    elif shape == "identical":
        t[:] = t[0]
    elif shape == "coplanar":
        t[:, 2] = np.float32(0.5)
    elif shape == "collinear":
        t[:, 1:] = np.float32([0.25, 0.75])
    else:
        t[:, 0] = np.float32([np.nan, np.inf, -np.inf])[np.arange(900) % 3]
    want, st = check(eng, q, t, 0.2, 8)
    if shape == "non_finite":
        assert want["stats"]["targets"] == 0 and want["stats"]["unmatched"] == 700 and st["max_cell_targets"] == 0
    else:
        assert 0 < want["stats"]["matched"] < 700
    if shape in ("one", "identical"):
        assert st["grid_cells"] == 1 and set(want["index"].tolist()) == {-1, 0}


def test_empty_sets(eng):
    rng = np.random.default_rng(6)
    pts = rng.random((300, 3), dtype=np.float32)
    want, st = check(eng, pts, np.zeros((0, 3), np.float32), 0.5, 4)
    assert want["stats"]["unmatched"] == 300 and want["hist"].tolist() == [0] * 4 and st["max_cell_targets"] == 0
    want, _ = check(eng, np.zeros((0, 3), np.float32), pts, 0.5, 4)
    assert want["stats"]["targets"] == 300 and len(want["index"]) == 0
    check(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.5)


# ---- 6. an extent much larger than the radius ---------------------------------------

def test_two_clusters_a_million_apart(eng):
    rng = np.random.default_rng(8)
    R = 1e-3
    a = (rng.random((500, 3)) * 0.01).astype(np.float32)
    b = (rng.random((500, 3)) * 0.01 + [1e6, 0, 0]).astype(np.float32)
    t = np.concatenate([a, b])[rng.permutation(1000)]
    between = np.stack([np.linspace(0.02, 1e6 - 1, 200), np.full(200, 0.005), np.full(200, 0.005)], axis=1)
    q = np.concatenate([(rng.random((400, 3)) * 0.012).astype(np.float32),
                        (rng.random((400, 3)) * 0.012 + [1e6, 0, 0]).astype(np.float32),
                        between.astype(np.float32)])
    want, st = check(eng, q, t, R, 16)
    assert (want["index"][:400] >= 0).sum() > 100 and (want["index"][400:800] >= 0).sum() > 50
    assert (want["index"][800:] == -1).all()
    # the table stays bounded: extent / max_dist is 1e9 on x alone
    assert st["grid_cells"] <= CELL_CAP
    # and far wider still
    t2 = np.concatenate([a, a + np.float32([0, 3e38, 0]), a - np.float32([0, 0, 3e38])])
    q2 = np.concatenate([q[:400], q[:400] + np.float32([0, 3e38, 0])])
    _, st = check(eng, q2, t2, 1e-30)
    assert st["grid_cells"] <= CELL_CAP


# ---- 7. a dense cell -----------------------------------------------------------------

def ball(rng, n, radius):
    v = rng.standard_normal((n, 3))
    v *= (rng.random((n, 1)) ** (1 / 3) * radius) / np.linalg.norm(v, axis=1, keepdims=True)
    return v


def test_dense_cell(eng):
    rng = np.random.default_rng(9)
    R = 0.05
    t = np.concatenate([ball(rng, 5000, R / 4) + 0.5, rng.random((200, 3))]).astype(np.float32)
    q = np.concatenate([ball(rng, 500, R / 4) + 0.5, rng.random((500, 3))]).astype(np.float32)
    order = rng.permutation(len(q))
    want, st = check(eng, q[order], t[rng.permutation(len(t))], R, 64)
    assert st["max_cell_targets"] >= 5000 // 8 and (want["index"][np.argsort(order)][:500] >= 0).all()


# ---- 8. strides ----------------------------------------------------------------------

def test_strides(eng, unit_cube):
    q, t = unit_cube
    rng = np.random.default_rng(10)
    want = CR.nearest(q, t, 0.1, 32)

    def noisy(dtype, pos):
        a = np.frombuffer(rng.integers(0, 256, len(pos) * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()
        a["pos"] = pos
        return a

    qv = noisy(dp.MESH_VERTEX_DTYPE, q)
    for tdtype in (dp.PATCH_DTYPE, dp.FUSED_DTYPE):
        tr = noisy(tdtype, t)
        assert tr.dtype.itemsize in (80, 40) and qv.dtype.itemsize == 16
        for form in FORMS:
            assert_equal(search(eng, form, qv, tr, 0.1, 32), want)
    # a caller's own record: pos behind 8 bytes of something else, stride 20
    own = noisy(np.dtype([("id", "<u8"), ("pos", "<f4", 3)]), t)
    assert own.dtype.itemsize == 20
    for form in FORMS:
        assert_equal(search(eng, form, q, own, 0.1, 32), want)
    for stride in (10, 8):
        with pytest.raises(ValueError):
            eng.cloud_nearest_device(64, 3, stride, 128, 3, 12, 0.1, 256, 512)
        assert call(eng, qs=stride) == N.DP_E_ARG and call(eng, ts=stride, device=True) == N.DP_E_ARG


# ---- 9. errors -------------------------------------------------------------------------

PTS = np.zeros((4, 3), np.float32)


def call(eng, q=PTS.ctypes.data, nq=4, qs=12, t=PTS.ctypes.data, nt=4, ts=12, max_dist=0.5, bins=0, flags=0,
         opts=True, index=True, dist=True, hist=None, device=False):
    """the raw library call; the device form is refused before any address is used"""
    cno = N.DpCloudNearestOptions(max_dist, bins, flags)
    pi, pd = ctypes.c_void_p(), ctypes.c_void_p()
    args = [eng._ctx, q, nq, qs, t, nt, ts, ctypes.byref(cno) if opts else None]
    if device:
        return N.lib.dp_cloud_nearest_device(*args, ctypes.c_void_p(4096) if index is True else index,
                                             ctypes.c_void_p(8192) if dist is True else dist, hist, None, None)
    return N.lib.dp_cloud_nearest(*args, ctypes.byref(pi) if index else None, ctypes.byref(pd) if dist else None,
                                  hist, None)


@pytest.mark.parametrize("device", [False, True], ids=FORMS)
def test_refusals_name_the_argument(eng, device):
    cases = [
        (dict(nq=-1), "n_queries"), (dict(nq=2**31), "n_queries"), (dict(nt=-1), "n_targets"),
        (dict(nt=2**31), "n_targets"), (dict(q=None), "queries"), (dict(t=None), "targets"),
        (dict(qs=8), "query_stride"), (dict(qs=10), "query_stride"), (dict(qs=0), "query_stride"),
        (dict(ts=8), "target_stride"), (dict(ts=10), "target_stride"), (dict(ts=14), "target_stride"),
        (dict(opts=False), "opts"), (dict(max_dist=0.0), "max_dist"), (dict(max_dist=-1.0), "max_dist"),
        (dict(max_dist=float("inf")), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
        (dict(bins=-1), "hist_bins"), (dict(bins=65537), "hist_bins"), (dict(flags=1), "flags"),
        (dict(flags=-2**31), "flags"), (dict(index=None), "index"), (dict(dist=None), "dist"),
    ]
    for kw, name in cases:
        assert call(eng, device=device, **kw) == N.DP_E_ARG, kw
        msg = N.lib.dp_last_error(eng._ctx).decode()
        assert msg.startswith("dp_cloud_nearest_device:" if device else "dp_cloud_nearest:") and name in msg, (kw, msg)
    # an output that equals an input
    same = ctypes.c_void_p(PTS.ctypes.data)
    if device:
        assert call(eng, device=True, index=same) == N.DP_E_ARG
        assert call(eng, device=True, dist=same) == N.DP_E_ARG
    assert call(eng, device=device, hist=same, bins=4) == N.DP_E_ARG
    assert "output" in N.lib.dp_last_error(eng._ctx).decode()
    # zero counts with NULL arrays are legal
    assert call(eng, device=device, q=None, nq=0, t=None, nt=0, index=None if device else True,
                dist=None if device else True) == N.DP_OK


def test_python_layer_refuses_before_the_library(eng):
    for kw in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(hist_bins=-1), dict(hist_bins=65537)):
        with pytest.raises(ValueError):
            eng.cloud_nearest(PTS, PTS, **dict(dict(max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.cloud_nearest(np.zeros((4, 2), np.float32), PTS, 0.5)
    with pytest.raises(ValueError):
        eng.cloud_nearest_device(64, 3, 12, 128, 3, 12, 0.5, 64, 512)  # an output equals an input
    with pytest.raises(ValueError):
        eng.cloud_nearest_device(64, 3, 12, 128, 3, 12, 0.5, 0, 512)  # no d_index


# ---- 10. no views ------------------------------------------------------------------------

def test_no_views_and_an_optional_histogram(unit_cube):
    q, t = unit_cube
    want = CR.nearest(q[:300], t[:300], 0.2, 8)
    with dp.Engine(device=0) as bare:
        assert bare.num_views() == 0
        assert_equal(bare.cloud_nearest(q[:300], t[:300], 0.2, 8), want)
        # hist_bins > 0 without a histogram buffer: nothing is written for it
        got = search(bare, "device", q[:300], t[:300], 0.2, 8, want_hist=False)
        assert got["hist"] is None and CR.same_bits(got["index"], want["index"])
        cno = N.DpCloudNearestOptions(0.2, 8, 0)
        pi, pd = ctypes.c_void_p(), ctypes.c_void_p()
        pts = np.ascontiguousarray(q[:300])
        assert N.lib.dp_cloud_nearest(bare._ctx, pts.ctypes.data, 300, 12, pts.ctypes.data, 300, 12, ctypes.byref(cno),
                                      ctypes.byref(pi), ctypes.byref(pd), None, None) == N.DP_OK
        assert (np.ctypeslib.as_array(ctypes.cast(pi.value, ctypes.POINTER(ctypes.c_int32)), (300,))
                == np.arange(300)).all()


def test_cloud_compare_and_pmvs_evaluate(eng, unit_cube):
    q, t = unit_cube
    got = dp.cloud_compare(eng, q, t, 0.03)
    CR.assert_compare(got, CR.compare(q, t, 0.03))
    assert 0 < got["accuracy"]["within_tau"] < got["accuracy"]["matched"] <= 3000 and 0 < got["fscore"] < 1
    pm = dp.PMVS()
    v = np.zeros(len(q), dp.MESH_VERTEX_DTYPE)
    v["pos"] = q
    CR.assert_compare(pm.evaluate(t, 0.03, cloud=v), got)
    with pytest.raises(ValueError):
        pm.evaluate(t, 0.03)  # the patches of a run that never happened
    with pytest.raises(ValueError):
        pm.evaluate(t, 0.03, cloud="mesh")
