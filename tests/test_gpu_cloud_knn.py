"""dp_cloud_knn on the GPU against the brute-force CPU reference
(tests/cloudknn_ref.py, restated from the header's spec): index, dist, count and
every integer statistic bit for bit, in the host and the device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudknn_ref as KR
import cloudnearest_ref as CR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
CELL_CAP = 1 << 24
F32_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


def search(eng, form, queries, targets, k, max_dist, exclude_self=False):
    """cloud_knn in either form as the dict Engine.cloud_knn returns; the device
    form writes into sentinel-filled buffers with slack behind them and checks
    that nothing beyond the results and no input was written"""
    if form == "host":
        return eng.cloud_knn(queries, targets, k, max_dist, exclude_self)
    import torch

    qa, qp, nq, qs = pmvs._cloud_points("test", queries)
    ta, tp, nt, ts = pmvs._cloud_points("test", targets)
    dq = to_device(qa.reshape(-1)) if nq else None
    dt = to_device(ta.reshape(-1)) if nt else None
    width = {"index": 4 * nq * k, "dist": 4 * nq * k, "count": 4 * nq}
    bufs = {name: torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for name, n in width.items()}
    torch.cuda.synchronize()
    st = eng.cloud_knn_device(dq.data_ptr() + (qp - qa.ctypes.data) if nq else None, nq, qs,
                              dt.data_ptr() + (tp - ta.ctypes.data) if nt else None, nt, ts, k, max_dist,
                              bufs["index"].data_ptr(), bufs["dist"].data_ptr(), bufs["count"].data_ptr(),
                              exclude_self=exclude_self)
    torch.cuda.synchronize()
    out = {"stats": st}
    for name, dtype, shape in (("index", np.int32, (nq, k)), ("dist", np.float32, (nq, k)), ("count", np.int32, (nq,))):
        raw = bufs[name].cpu().numpy()
        assert (raw[width[name]:] == SENTINEL).all(), name
        out[name] = raw[:width[name]].view(dtype).reshape(shape).copy()
    if nq:
        assert dq.cpu().numpy().tobytes() == qa.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == ta.tobytes()
    return out


def assert_equal(got, want):
    for name in ("index", "dist", "count"):
        assert CR.same_bits(got[name], want[name]), name
    st = got["stats"]
    assert {c: st[c] for c in KR.KNN_COUNTS} == want["stats"]
    assert st["full"] + st["partial"] + st["empty"] == st["queries"]
    assert 1 <= st["grid_cells"] <= CELL_CAP and 0 <= st["max_cell_targets"] <= want["stats"]["targets"]
    assert st["build_ms"] >= 0 and st["query_ms"] >= 0


def check(eng, queries, targets, k, max_dist, exclude_self=False):
    """both forms against the reference (computed once); returns it and the last statistics"""
    want = KR.knn(queries, targets, k, max_dist, exclude_self)
    for form in FORMS:
        got = search(eng, form, queries, targets, k, max_dist, exclude_self)
        assert_equal(got, want)
    return want, got["stats"]


# ---- 1. random, on both sides of every list size ---------------------------------------

@pytest.fixture(scope="module")
def unit_cube():
    rng = np.random.default_rng(20261021)
    return rng.random((3000, 3), dtype=np.float32), rng.random((2500, 3), dtype=np.float32)


@pytest.mark.parametrize("k", [1, 5, 8, 9, 16, 17, 32])
def test_random_unit_cube(eng, unit_cube, k):
    q, t = unit_cube
    want, st = check(eng, q, t, k, 0.1)
    # about ten candidates per query: full, partial and empty rows at the larger k
    assert want["stats"]["neighbours"] > 2900 * min(k, 4) and 27 < st["grid_cells"] <= 11 ** 3
    if k >= 5:
        assert want["stats"]["partial"] > 100 and (want["stats"]["full"] > 50 or k == 32)
    if k == 1:
        near = eng.cloud_nearest(q, t, 0.1)
        for form in FORMS:
            got = search(eng, form, q, t, 1, 0.1)
            assert CR.same_bits(got["index"][:, 0], near["index"]) and CR.same_bits(got["dist"][:, 0], near["dist"])
            assert got["stats"]["full"] == near["stats"]["matched"]
            assert got["stats"]["empty"] == near["stats"]["unmatched"]


def test_the_order_of_the_queries_does_not_matter(eng, unit_cube):
    q, t = unit_cube
    perm = np.random.default_rng(11).permutation(len(q))
    a = search(eng, "host", q, t, 8, 0.1)
    for form in FORMS:
        b = search(eng, form, q[perm], t, 8, 0.1)
        for name in ("index", "dist", "count"):
            assert CR.same_bits(a[name][perm], b[name]), name


# ---- 2. ties across the k-th place -------------------------------------------------------

def lattice(n, step, origin=0.0):
    g = np.arange(n, dtype=np.float64) * step + origin
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("k", [3, 8, 13, 32])
def test_ties_straddle_the_kth_place(eng, k):
    rng = np.random.default_rng(7)
    base = lattice(8, 2.0 ** -4)  # 512 targets, every one twice, in shuffled order
    t = np.concatenate([base, base])[rng.permutation(1024)]
    # from a lattice point: 2 at d2 = 0, 12 at 1 step, 24 at sqrt 2, 16 at sqrt 3 (fewer at the faces);
    # from the midpoint of an x-edge: 4 at half a step, 16 at sqrt(1.25) steps
    q = np.concatenate([base, base[base[:, 0] < 7 * 2.0 ** -4] + np.float32([2.0 ** -5, 0, 0])])
    want, _ = check(eng, q, t, k, 2.0 ** -4 * 1.8)
    inner = 4 * 64 + 4 * 8 + 4  # lattice point (4, 4, 4)
    d = want["dist"][inner].astype(np.float64) * 16
    counts = [2, 12, 24, 16]
    expect = np.repeat(np.sqrt([0.0, 1.0, 2.0, 3.0]), counts)[:k].astype(np.float32)
    assert np.allclose(d, expect) and want["count"][inner] == k
    # within a tie the indices ascend, and the tie is cut at the lowest ones
    d2row = want["dist"][inner]
    for v in np.unique(d2row):
        tied = want["index"][inner][d2row == v]
        assert (np.diff(tied) > 0).all()
        everyone = np.flatnonzero(np.isclose(np.linalg.norm(t.astype(np.float64) - q[inner], axis=1), float(v)))
        assert tied.tolist() == everyone[:len(tied)].tolist()


# ---- 3. fewer than k candidates, and none --------------------------------------------------

def test_fewer_than_k_and_none(eng):
    rng = np.random.default_rng(12)
    t = rng.random((400, 3), dtype=np.float32)
    q = np.concatenate([rng.random((300, 3), dtype=np.float32), rng.random((50, 3), dtype=np.float32) + np.float32(3)])
    want, _ = check(eng, q, t, 16, 0.15)
    s = want["stats"]
    assert s["partial"] > 200 and s["empty"] >= 50 and s["full"] < 50
    assert (want["count"][300:] == 0).all() and (want["index"][300:] == -1).all() and np.isinf(want["dist"][300:]).all()
    want, _ = check(eng, q, t, 32, 0.01)
    assert want["stats"]["full"] == 0


# ---- 4. the inclusive radius across cell borders, outside the box ---------------------------

def test_queries_on_cell_borders(eng):
    # targets on a lattice of step R from an origin that is a lattice point: every
    # query on a lattice point sits on the border of its cell on all three axes and
    # has its six axis neighbours at exactly R
    R = np.float32(2.0 ** -3)
    t = lattice(9, float(R), origin=-0.5)
    q = t[::3]
    want, st = check(eng, q, t, 8, R)
    inner = np.all((q > -0.5) & (q < 0.5), axis=1)
    assert (want["count"][inner] == 7).all() and (want["dist"][inner][:, 1:7] == R).all()
    assert (want["dist"][:, 0] == 0).all() and st["grid_cells"] >= 8 ** 3
    # one float32 step inside the radius loses the six
    below = np.nextafter(R, np.float32(0))
    want, _ = check(eng, q, t, 8, below)
    assert (want["count"] == 1).all()


def test_queries_outside_the_box(eng):
    R = 0.25
    rng = np.random.default_rng(3)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    t = np.concatenate([corners, rng.random((600, 3), dtype=np.float32),
                        np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]])])
    out = np.where(corners > 0, 1.0, -1.0)
    q = []
    for reach in (0.1, 0.2, 0.3, 0.6):  # less than a cell beyond the box, and more
        for mask in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]):
            q.append(corners + out * np.float32(mask) * reach)
    far = []
    for axis in range(3):
        for v in (1e30, -1e30, np.inf, -np.inf, np.nan, F32_MAX, -F32_MAX):
            p = [0.5, 0.5, 0.5]
            p[axis] = v
            far.append(p)
    q = np.concatenate(q + [np.float32(far), np.float32([[1e30, -1e30, 1e30], [F32_MAX] * 3])]).astype(np.float32)
    want, _ = check(eng, q, t, 4, R)
    n = len(corners)
    assert (want["count"][:7 * n] >= 1).all() and (want["count"][21 * n:] == 0).all()
    assert want["stats"]["skipped_queries"] == 9 and want["stats"]["skipped_targets"] == 3


# ---- 5. the grid's other shapes ---------------------------------------------------------------

def test_an_extent_that_forces_cell_doubling(eng):
    rng = np.random.default_rng(8)
    R = 1e-3
    a = (rng.random((500, 3)) * 0.01).astype(np.float32)
    b = (rng.random((500, 3)) * 0.01 + [1e6, 0, 0]).astype(np.float32)
    t = np.concatenate([a, b])[rng.permutation(1000)]
    q = np.concatenate([(rng.random((400, 3)) * 0.012).astype(np.float32),
                        (rng.random((400, 3)) * 0.012 + [1e6, 0, 0]).astype(np.float32),
                        np.float32([[5e5, 0.005, 0.005]])])
    want, st = check(eng, q, t, 9, R)
    assert want["stats"]["neighbours"] > 400 and want["count"][800] == 0 and st["grid_cells"] <= CELL_CAP


def test_all_targets_in_one_cell(eng, unit_cube):
    q, t = unit_cube
    want, st = check(eng, q[:500], t, 17, 2.0)
    assert st["grid_cells"] == 1 and st["max_cell_targets"] == 2500 and want["stats"]["full"] == 500


# ---- 6. EXCLUDE_SELF ----------------------------------------------------------------------------

def test_exclude_self_with_exact_duplicates(eng):
    rng = np.random.default_rng(13)
    p = rng.random((600, 3), dtype=np.float32)
    p[300:400] = p[100:200]  # a duplicate under another index stays a neighbour at distance 0
    p[17] = np.float32([np.nan, 0, 0])
    want, _ = check(eng, p, p, 4, 0.2, exclude_self=True)
    assert (want["index"] != np.arange(600)[:, None]).all()
    assert (want["index"][100:200, 0] == np.arange(300, 400)).all() and (want["dist"][100:200, 0] == 0).all()
    assert (want["index"][300:400, 0] == np.arange(100, 200)).all()
    with_self, _ = check(eng, p, p, 4, 0.2)
    assert (with_self["index"][:17, 0] == np.arange(17)).all() and with_self["count"][17] == 0
    assert (with_self["index"][100:200, :2] == np.stack([np.arange(100, 200), np.arange(300, 400)], axis=1)).all()
    # the rule is on the index: another array of the same length, nothing in common
    other = rng.random((600, 3), dtype=np.float32)
    check(eng, other, p, 4, 0.2, exclude_self=True)


# ---- 7. points that are not finite, strides, sizes ------------------------------------------------

def test_nan_and_inf_in_queries_and_targets(eng):
    rng = np.random.default_rng(14)
    q, t = rng.random((500, 3), dtype=np.float32), rng.random((700, 3), dtype=np.float32)
    bad = np.float32([np.nan, np.inf, -np.inf])
    q[np.arange(0, 500, 7), np.arange(0, 500, 7) % 3] = bad[np.arange(0, 500, 7) % 3]
    t[np.arange(0, 700, 5), np.arange(0, 700, 5) % 3] = bad[np.arange(0, 700, 5) % 3]
    want, _ = check(eng, q, t, 8, 0.2)
    assert want["stats"]["skipped_queries"] == 72 and want["stats"]["skipped_targets"] == 140
    assert (want["count"][::7] == 0).all() and not np.isin(want["index"], np.arange(0, 700, 5)).any()
    t[:] = bad[0]
    want, st = check(eng, q, t, 8, 0.2)
    assert want["stats"]["targets"] == 0 and want["stats"]["empty"] == want["stats"]["queries"]


@pytest.mark.parametrize("stride", [12, 16, 40, 64])
def test_strides(eng, unit_cube, stride):
    q, t = unit_cube[0][:700], unit_cube[1][:900]
    rng = np.random.default_rng(stride)
    dtype = np.dtype([("pos", "<f4", 3), ("rest", "u1", stride - 12)]) if stride > 12 else None

    def records(pos):
        if dtype is None:
            return pos
        a = np.frombuffer(rng.integers(0, 256, len(pos) * stride, dtype=np.uint8).tobytes(), dtype).copy()
        a["pos"] = pos
        return a

    qr, tr = records(q), records(t)
    assert pmvs._cloud_points("t", tr)[3] == stride
    want = KR.knn(q, t, 9, 0.15)
    for form in FORMS:
        assert_equal(search(eng, form, qr, tr, 9, 0.15), want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(eng, n):
    rng = np.random.default_rng(100 + n)
    p = rng.random((n, 3), dtype=np.float32)
    other = rng.random((130, 3), dtype=np.float32)
    check(eng, p, p, 5, 0.4, exclude_self=True)
    check(eng, p, other, 16, 0.4)
    check(eng, other, p, 32, 0.4)


# ---- 8. errors ----------------------------------------------------------------------------------------

PTS = np.zeros((4, 3), np.float32)


def call(eng, q=PTS.ctypes.data, nq=4, qs=12, t=PTS.ctypes.data, nt=4, ts=12, max_dist=0.5, k=4, flags=0, opts=True,
         index=True, dist=True, count=True, device=False, outs=None):
    """the raw library call; the device form is refused before any address is used"""
    cko = N.DpCloudKnnOptions(max_dist, k, flags)
    args = [eng._ctx, q, nq, qs, t, nt, ts, ctypes.byref(cko) if opts else None]
    if device:
        return N.lib.dp_cloud_knn_device(*args, ctypes.c_void_p(4096) if index is True else index,
                                         ctypes.c_void_p(8192) if dist is True else dist,
                                         ctypes.c_void_p(12288) if count is True else count, None, None)
    pi, pd, pc = outs if outs else (ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p())
    return N.lib.dp_cloud_knn(*args, ctypes.byref(pi) if index else None, ctypes.byref(pd) if dist else None,
                              ctypes.byref(pc) if count else None, None)


@pytest.mark.parametrize("device", [False, True], ids=FORMS)
def test_refusals_name_the_argument_and_write_nothing(eng, device):
    cases = [
        (dict(nq=-1), "n_queries"), (dict(nq=2**31), "n_queries"), (dict(nt=-1), "n_targets"),
        (dict(nt=2**31), "n_targets"), (dict(q=None), "queries"), (dict(t=None), "targets"),
        (dict(qs=8), "query_stride"), (dict(qs=10), "query_stride"), (dict(ts=8), "target_stride"),
        (dict(ts=14), "target_stride"), (dict(opts=False), "opts"), (dict(max_dist=0.0), "max_dist"),
        (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"),
        (dict(max_dist=float("nan")), "max_dist"), (dict(k=0), "k must"), (dict(k=33), "k must"), (dict(k=-1), "k must"),
        (dict(flags=2), "flags"), (dict(flags=3), "flags"), (dict(flags=-2**31), "flags"),
        (dict(flags=1, nt=3), "EXCLUDE_SELF"), (dict(flags=1, nq=0, q=None), "EXCLUDE_SELF"),
        (dict(index=None), "index"), (dict(dist=None), "dist"), (dict(count=None), "count"),
    ]
    outs = (ctypes.c_void_p(1), ctypes.c_void_p(2), ctypes.c_void_p(3))
    for kw, name in cases:
        assert call(eng, device=device, outs=outs, **kw) == N.DP_E_ARG, kw
        msg = N.lib.dp_last_error(eng._ctx).decode()
        assert msg.startswith("dp_cloud_knn_device:" if device else "dp_cloud_knn:") and name in msg, (kw, msg)
        assert [o.value for o in outs] == [1, 2, 3]  # the host form's results are left alone
    if device:
        import torch

        # a refused call writes nothing: real buffers, a bad option, the sentinel everywhere
        buf = torch.full((3, 256), SENTINEL, dtype=torch.uint8, device="cuda")
        pts = to_device(PTS.reshape(-1))
        for kw in (dict(k=33), dict(max_dist=0.0), dict(flags=2), dict(flags=1, nt=3)):
            assert call(eng, device=True, q=pts.data_ptr(), t=pts.data_ptr(), index=ctypes.c_void_p(buf[0].data_ptr()),
                        dist=ctypes.c_void_p(buf[1].data_ptr()), count=ctypes.c_void_p(buf[2].data_ptr()),
                        **kw) == N.DP_E_ARG
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        same = ctypes.c_void_p(PTS.ctypes.data)
        for kw in (dict(index=same), dict(dist=same), dict(count=same)):
            assert call(eng, device=True, **kw) == N.DP_E_ARG
            assert "output" in N.lib.dp_last_error(eng._ctx).decode()
    # zero counts with NULL arrays are legal, with the flag too
    for flags in (0, 1):
        assert call(eng, device=device, q=None, nq=0, t=None, nt=0, flags=flags, index=None if device else True,
                    dist=None if device else True, count=None if device else True) == N.DP_OK


def test_python_layer_refuses_before_the_library(eng):
    for kw in (dict(max_dist=0.0), dict(k=0), dict(k=33), dict(exclude_self=1)):
        with pytest.raises(ValueError):
            eng.cloud_knn(PTS, PTS, **dict(dict(k=4, max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.cloud_knn(PTS, PTS[:3], 4, 0.5, exclude_self=True)
    with pytest.raises(ValueError):
        eng.cloud_knn_device(64, 3, 12, 128, 3, 12, 4, 0.5, 64, 512, 1024)  # an output equals an input
    with pytest.raises(ValueError):
        eng.cloud_knn_device(64, 3, 12, 128, 3, 12, 4, 0.5, 256, 512, 0)  # no d_count
