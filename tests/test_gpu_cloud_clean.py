"""dp_cloud_clean on the GPU against the brute-force CPU reference
(tests/cloudknn_ref.py, restated from the header's spec): keep, mean_dist, map,
the packed records, the kept count, every integer statistic and the bits of mu,
sigma and the threshold, in the host and the device form."""
import ctypes
import struct

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


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


def clean(eng, form, points, k, max_dist, **kw):
    """cloud_clean in either form as the dict Engine.cloud_clean returns, plus
    "n_out"; the device form writes into sentinel-filled buffers with slack
    behind them and checks that nothing beyond the results -- for the records:
    beyond the kept ones -- and no input was written"""
    if form == "host":
        out = eng.cloud_clean(points, k, max_dist, **kw)
        out["n_out"] = len(out["points"])
        return out
    import torch

    pa, pp, n, stride = pmvs._cloud_points("test", points)
    assert pp == pa.ctypes.data
    dpts = to_device(pa.reshape(-1)) if n else None
    width = {"keep": n, "mean_dist": 4 * n, "map": 4 * n, "out": n * stride, "n_out": 8}
    bufs = {name: torch.full((w + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for name, w in width.items()}
    torch.cuda.synchronize()
    st = eng.cloud_clean_device(dpts.data_ptr() if n else None, n, stride, k, max_dist, bufs["keep"].data_ptr(),
                                bufs["mean_dist"].data_ptr(), bufs["map"].data_ptr(), bufs["out"].data_ptr(),
                                bufs["n_out"].data_ptr(), **kw)
    torch.cuda.synchronize()
    raw = {name: b.cpu().numpy() for name, b in bufs.items()}
    n_out = int(raw["n_out"][:8].view(np.int64)[0])
    assert 0 <= n_out <= n
    width["out"] = n_out * stride
    for name, w in width.items():
        assert (raw[name][w:] == SENTINEL).all(), name
    if n:
        assert dpts.cpu().numpy().tobytes() == pa.tobytes()
    kept = raw["out"][:n_out * stride].copy().view(pa.dtype).reshape((n_out,) + pa.shape[1:])
    return {"keep": raw["keep"][:n].copy(), "mean_dist": raw["mean_dist"][:4 * n].view(np.float32).copy(),
            "map": raw["map"][:4 * n].view(np.int32).copy(), "points": kept, "n_out": n_out, "stats": st}


def bits(x):
    return struct.pack("<d", float(x))


def assert_equal(got, want):
    for name in ("keep", "mean_dist", "map"):
        assert CR.same_bits(got[name], want[name]), name
    assert got["n_out"] == len(want["points"]) == want["stats"]["kept"]
    assert got["points"].dtype == want["points"].dtype and got["points"].tobytes() == want["points"].tobytes()
    st = got["stats"]
    assert {c: st[c] for c in KR.CLEAN_COUNTS} == want["stats"]
    assert st["kept"] + st["removed_sparse"] + st["removed_far"] == st["points"]
    for name in ("mu", "sigma", "threshold"):
        assert bits(st[name]) == bits(want[name]), (name, st[name], want[name])
    assert st["knn_ms"] >= 0 and st["clean_ms"] >= 0 and st["grid_cells"] >= 1


def check(eng, points, k, max_dist, **kw):
    """both forms against the reference (computed once), which is returned"""
    want = KR.clean(points, k, max_dist, **kw)
    for form in FORMS:
        assert_equal(clean(eng, form, points, k, max_dist, **kw), want)
    return want


# ---- 1. a planted surface, isolated points and a far pair -----------------------------------

def planted():
    """a 40 x 40 lattice in the plane z = 0 with step 0.025 (indices 0..1599), five
    points with nothing within 0.1 (1600..1604), and two points 0.09 apart with
    nothing else within 0.1 of either (1605, 1606)"""
    g = np.arange(40, dtype=np.float64) * 0.025
    surface = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    alone = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, -0.4], [2.0, 0.0, 0.0], [-0.3, -0.3, 0.0], [0.5, 1.3, 0.0]])
    pair = np.array([[0.5, 0.5, 1.5], [0.5, 0.59, 1.5]])
    return np.concatenate([surface, alone, pair]).astype(np.float32)


def test_planted_outliers_under_each_mode(eng):
    p = planted()
    # the radius rule: the isolated points go, the pair have each other
    want = check(eng, p, 8, 0.1, radius_only=True)
    assert np.flatnonzero(want["keep"] == 0).tolist() == [1600, 1601, 1602, 1603, 1604]
    assert want["stats"] == dict(points=1607, skipped=0, eligible=1602, kept=1602, removed_sparse=5, removed_far=0)
    assert (want["mu"], want["sigma"], want["threshold"]) == (0.0, 0.0, 0.0)
    # the statistical rule: the pair's mean distance, 3.6 steps, is far above the
    # surface's (1.2 steps inside, 1.5 on an edge, 1.8 in a corner)
    want = check(eng, p, 8, 0.1, std_mul=10.0)
    assert np.flatnonzero(want["keep"] == 0).tolist() == [1600, 1601, 1602, 1603, 1604, 1605, 1606]
    assert want["stats"] == dict(points=1607, skipped=0, eligible=1602, kept=1600, removed_sparse=5, removed_far=2)
    assert 0.025 * 1.2 < want["mu"] < 0.025 * 1.3 and want["mean_dist"][1605] == np.float32(0.59) - np.float32(0.5)
    assert want["map"][1599] == 1599 and (want["map"][1600:] == -1).all()
    # a tighter threshold takes the lattice's corners and edges too, the reference says which
    want = check(eng, p, 8, 0.1, std_mul=2.0)
    assert want["stats"]["removed_far"] > 2 + 4 and want["keep"][20 * 40 + 20] == 1 and want["keep"][0] == 0


# ---- 2. sizes around the reduction's levels, distances over several binades --------------------

def binades(n, seed):
    """clusters of four points whose sizes run over ten binades, so the mean
    distances do: a sum in another order rounds differently"""
    rng = np.random.default_rng(seed)
    c = np.arange(n) // 4
    centre = np.stack([c % 32, (c // 32) % 32, c // 1024], axis=1).astype(np.float64)
    size = 2.0 ** -(2 + c % 10)
    return (centre + rng.random((n, 3)) * size[:, None]).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4097])
def test_sizes_around_the_reduction_levels(eng, n):
    p = binades(n, n)
    want = check(eng, p, 3, 0.45, std_mul=1.0)
    if n >= 255:
        assert want["stats"]["eligible"] >= n - 3 and 0 < want["stats"]["removed_far"] < n // 2
        m = np.where(want["keep"] | (want["mean_dist"] < np.inf), want["mean_dist"].astype(np.float64), 0.0)
        assert m.max() > 64 * m[m > 0].min()
    if n == 4097:
        # the order matters at this size: the sequential sum of the same terms has other bits
        _, d2, count, _, _ = KR.knn_d2(p, p, 3, 0.45, exclude_self=True)
        x = np.array([np.sqrt(d2[i, :c]).sum() / c if c else 0.0 for i, c in enumerate(count)])
        seq = 0.0
        for v in x:
            seq = seq + float(v)
        assert KR.pairwise_sum(x) != seq
    if n == 1:
        assert want["stats"]["removed_sparse"] == 1 and want["keep"].tolist() == [0]


# ---- 3. the options' ends ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(21)
    p = rng.random((1500, 3), dtype=np.float32)
    p[::97, 1] = np.float32(np.nan)
    p[5::211] = np.float32([np.inf, 0, 0])
    return p


def test_std_mul_zero(eng, cloud):
    want = check(eng, cloud, 8, 0.12, std_mul=0.0)
    s = want["stats"]
    assert bits(want["threshold"]) == bits(want["mu"]) and want["sigma"] > 0
    assert 0.25 * s["eligible"] < s["removed_far"] < 0.75 * s["eligible"] and s["skipped"] == 16 + 8


def test_min_neighbours_is_k(eng, cloud):
    want = check(eng, cloud, 8, 0.12, std_mul=2.0, min_neighbours=8)
    assert 100 < want["stats"]["removed_sparse"] < 1400 and want["stats"]["kept"] > 0
    want = check(eng, cloud, 8, 0.12, min_neighbours=8, radius_only=True)
    assert want["stats"]["removed_far"] == 0 and want["stats"]["kept"] == want["stats"]["eligible"]
    check(eng, cloud, 32, 0.12, std_mul=1.5, min_neighbours=4)
    check(eng, cloud, 16, 0.2, std_mul=1.5, min_neighbours=16)


def test_no_eligible_point_and_one(eng, cloud):
    want = check(eng, cloud, 4, 1e-4)  # nobody has a neighbour: N = 0
    assert want["stats"]["eligible"] == 0 and want["stats"]["kept"] == 0 and want["stats"]["removed_sparse"] == 1476
    assert (want["mu"], want["sigma"], want["threshold"]) == (0.0, 0.0, 0.0) and np.isinf(want["mean_dist"]).all()
    check(eng, cloud[:0], 4, 0.5)  # n = 0
    check(eng, np.full((5, 3), np.nan, np.float32), 4, 0.5)  # nobody takes part
    # three points on a line, only the middle one has two neighbours within 1: N = 1, var = 0, T = mu = 1
    line = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    want = check(eng, line, 2, 1.0, std_mul=3.0, min_neighbours=2)
    assert want["keep"].tolist() == [0, 1, 0] and (want["mu"], want["sigma"], want["threshold"]) == (1.0, 0.0, 1.0)
    assert want["stats"] == dict(points=3, skipped=0, eligible=1, kept=1, removed_sparse=2, removed_far=0)


def test_a_mean_equal_to_the_threshold_is_kept(eng):
    # the corners of a cube of side 0.3: every point has three neighbours at the
    # same distance, so every mean is the same double, sigma = 0 and T = mu = m_i
    side = np.float32(0.3)
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32) * side
    for std_mul in (0.0, 2.0):
        want = check(eng, p, 3, 0.31, std_mul=std_mul)
        assert want["keep"].tolist() == [1] * 8 and want["sigma"] == 0.0
        assert bits(want["threshold"]) == bits(want["mu"]) and (want["mean_dist"] == np.float32(want["mu"])).all()
    # one float32 step less for one corner's x: its mean is smaller, the others' larger than mu, and they go
    q = p.copy()
    q[7, 0] = np.nextafter(side, np.float32(0))
    want = check(eng, q, 3, 0.31, std_mul=0.0)
    assert 0 < want["stats"]["removed_far"] < 8 and want["sigma"] > 0


# ---- 4. whole records move --------------------------------------------------------------------------

def test_stride_40_records_move_whole(eng, cloud):
    rng = np.random.default_rng(22)
    rec = np.frombuffer(rng.integers(0, 256, len(cloud) * 40, dtype=np.uint8).tobytes(), dp.FUSED_DTYPE).copy()
    rec["pos"] = cloud
    assert rec.dtype.itemsize == 40 and len(set(rec["x"].tolist())) > 1400  # distinct payloads
    want = check(eng, rec, 8, 0.12, std_mul=1.0)
    plain = KR.clean(cloud, 8, 0.12, std_mul=1.0)
    assert CR.same_bits(want["keep"], plain["keep"]) and 0 < want["stats"]["kept"] < 1476
    assert want["points"].tobytes() == rec[want["keep"] == 1].tobytes()
    # the optional outputs left out: keep alone
    import torch

    d = to_device(rec)
    keep = torch.full((len(rec) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = eng.cloud_clean_device(d.data_ptr(), len(rec), 40, 8, 0.12, keep.data_ptr(), std_mul=1.0)
    torch.cuda.synchronize()
    raw = keep.cpu().numpy()
    assert CR.same_bits(raw[:len(rec)], want["keep"]) and (raw[len(rec):] == SENTINEL).all()
    assert st["kept"] == want["stats"]["kept"]
    assert eng.cloud_clean_device(d.data_ptr(), len(rec), 40, 8, 0.12, keep.data_ptr(), std_mul=1.0, stats=False) is None
    torch.cuda.synchronize()
    assert CR.same_bits(keep.cpu().numpy()[:len(rec)], want["keep"])


# ---- 5. errors --------------------------------------------------------------------------------------------

PTS = np.zeros((4, 3), np.float32)


def call(eng, p=PTS.ctypes.data, n=4, stride=12, max_dist=0.5, k=2, min_nb=1, std_mul=2.0, flags=0, opts=True,
         keep=True, mean=None, where=None, out=None, n_out=None, device=False):
    """the raw library call; the device form is refused before any address is used"""
    co = N.DpCloudCleanOptions(max_dist, k, min_nb, std_mul, flags)
    args = [eng._ctx, p, n, stride, ctypes.byref(co) if opts else None]
    if device:
        return N.lib.dp_cloud_clean_device(*args, ctypes.c_void_p(4096) if keep is True else keep, mean, where, out,
                                           n_out, None, None)
    pk = ctypes.c_void_p(1)
    rc = N.lib.dp_cloud_clean(*args, ctypes.byref(pk) if keep else None, mean, where, out, n_out, None)
    assert rc == N.DP_OK or pk.value == 1  # a refused call leaves the result alone
    return rc


@pytest.mark.parametrize("device", [False, True], ids=FORMS)
def test_refusals_name_the_argument_and_write_nothing(eng, device):
    cases = [
        (dict(n=-1), "n must"), (dict(n=2**31), "n must"), (dict(p=None), "points"), (dict(stride=8), "stride"),
        (dict(stride=14), "stride"), (dict(stride=0), "stride"), (dict(opts=False), "opts"),
        (dict(max_dist=0.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
        (dict(max_dist=float("inf")), "max_dist"), (dict(k=0), "k must"), (dict(k=33), "k must"),
        (dict(min_nb=0), "min_neighbours"), (dict(min_nb=3), "min_neighbours"), (dict(min_nb=-1), "min_neighbours"),
        (dict(std_mul=-0.5), "std_mul"), (dict(std_mul=float("nan")), "std_mul"), (dict(std_mul=float("inf")), "std_mul"),
        (dict(flags=2), "flags"), (dict(flags=3), "flags"), (dict(flags=-2**31), "flags"), (dict(keep=None), "keep"),
    ]
    for kw, name in cases:
        assert call(eng, device=device, **kw) == N.DP_E_ARG, kw
        msg = N.lib.dp_last_error(eng._ctx).decode()
        assert msg.startswith("dp_cloud_clean_device:" if device else "dp_cloud_clean:") and name in msg, (kw, msg)
    if device:
        import torch

        same = ctypes.c_void_p(PTS.ctypes.data)
        for kw in (dict(keep=same), dict(mean=same), dict(where=same), dict(out=same), dict(n_out=same),
                   dict(mean=ctypes.c_void_p(4096)), dict(out=ctypes.c_void_p(8192), where=ctypes.c_void_p(8192))):
            assert call(eng, device=True, **kw) == N.DP_E_ARG, kw
            assert "output" in N.lib.dp_last_error(eng._ctx).decode()
        # a refused call writes nothing: real buffers, a bad option, the sentinel everywhere
        buf = torch.full((5, 256), SENTINEL, dtype=torch.uint8, device="cuda")
        pts = to_device(PTS.reshape(-1))
        ptr = [ctypes.c_void_p(buf[i].data_ptr()) for i in range(5)]
        for kw in (dict(k=33), dict(min_nb=3), dict(std_mul=-1.0), dict(flags=2), dict(max_dist=0.0)):
            assert call(eng, device=True, p=pts.data_ptr(), keep=ptr[0], mean=ptr[1], where=ptr[2], out=ptr[3],
                        n_out=ptr[4], **kw) == N.DP_E_ARG
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
    # n = 0 with NULL arrays is legal
    assert call(eng, device=device, p=None, n=0, keep=None if device else True) == N.DP_OK


def test_python_layer_refuses_before_the_library(eng):
    for kw in (dict(max_dist=0.0), dict(k=0), dict(k=33), dict(min_neighbours=0), dict(min_neighbours=5),
               dict(std_mul=-1.0), dict(radius_only=1)):
        with pytest.raises(ValueError):
            eng.cloud_clean(PTS, **dict(dict(k=4, max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.cloud_clean(np.zeros(3, [("id", "<u8"), ("pos", "<f4", 3)]), 4, 0.5)  # pos is not the record's first field
    with pytest.raises(ValueError):
        eng.cloud_clean_device(64, 3, 12, 4, 0.5, 64)  # an output equals the input
    with pytest.raises(ValueError):
        eng.cloud_clean_device(64, 3, 12, 4, 0.5, 0)  # no d_keep


# ---- 6. PMVS.fused_cloud(clean=...) ---------------------------------------------------------------------------

def test_pmvs_fused_cloud_clean():
    from densepoints_amd import synth

    cfg = synth.config(4, 160, 120, 1)
    P, imgs, seeds = synth.scene_host(cfg)
    pm = dp.PMVS()
    for v in range(cfg.n_views):
        pm.add_camera(dp.View(P[v], imgs[v]))
    assert pm.run(seeds)
    cloud = pm.fused_cloud()
    assert 500 < len(cloud) < 20000 and "cloud_clean" not in pm.stats
    pos = cloud["pos"].astype(np.float64)
    ext = pos[:, :2].max(axis=0) - pos[:, :2].min(axis=0)
    R = float(np.float32(4 * np.sqrt(ext[0] * ext[1] / len(cloud))))
    want = KR.clean(cloud, 8, R, std_mul=1.0)
    assert 0 < want["stats"]["kept"] < len(cloud)
    cleaned = pm.fused_cloud(clean=dict(max_dist=R, std_mul=1.0))  # k defaults to 8
    assert cleaned.dtype == cloud.dtype and cleaned.tobytes() == want["points"].tobytes()
    st = pm.stats["cloud_clean"]
    assert {c: st[c] for c in KR.CLEAN_COUNTS} == want["stats"] and bits(st["mu"]) == bits(want["mu"])
    assert pm.stats["fused"]["emitted"] == len(cloud)
    only = pm.fused_cloud(clean=dict(k=4, max_dist=R, min_neighbours=4, radius_only=True))
    assert only.tobytes() == KR.clean(cloud, 4, R, min_neighbours=4, radius_only=True)["points"].tobytes()
