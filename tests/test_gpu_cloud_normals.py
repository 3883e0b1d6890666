"""dp_cloud_normals on the GPU against the CPU reference (tests/cloudnormals_ref.py,
restated from the header's spec): normal, variation, count and every integer
statistic bit for bit, in the host and the device form."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudknn_ref as KR
import cloudnearest_ref as CR
import cloudnormals_ref as NR
from cloudnormalscases import (LINE_DIR, SPHERE_CENTRE, TILT_A, TILT_B, duplicated, far, holed, lattice, line, sphere,
                               surface, tilted)
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
OWN = "own"  # directions = the records' own normal field, read in place


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


def normals(eng, form, points, k, max_dist, min_neighbours=3, viewpoint=None, directions=None):
    """cloud_normals in either form as the dict Engine.cloud_normals returns; the
    device form writes into sentinel-filled buffers with slack behind them and
    checks that nothing beyond the results and no input was written"""
    if form == "host":
        return eng.cloud_normals(points, k, max_dist=max_dist, min_neighbours=min_neighbours, viewpoint=viewpoint,
                                 directions=True if isinstance(directions, str) else directions)
    import torch

    pa, pp, n, stride = pmvs._cloud_points("test", points)
    assert pp == pa.ctypes.data
    dpts = to_device(pa.reshape(-1)) if n else None
    orient, d_toward, ts, dtw, tw = None, None, 0, None, None
    if viewpoint is not None or directions is not None:
        orient = "viewpoint" if viewpoint is not None else "direction"
        if isinstance(directions, str):
            d_toward, ts = dpts.data_ptr() + pa.dtype.fields["normal"][1], stride
        else:
            tw = np.ascontiguousarray(viewpoint if viewpoint is not None else directions, np.float32)
            dtw = to_device(tw.reshape(-1))
            d_toward, ts = dtw.data_ptr(), 0 if tw.shape == (3,) else 12
    width = {"normal": 12 * n, "variation": 4 * n, "count": 4 * n}
    bufs = {name: torch.full((w + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for name, w in width.items()}
    torch.cuda.synchronize()
    st = eng.cloud_normals_device(dpts.data_ptr() if n else None, n, stride, k, max_dist, bufs["normal"].data_ptr(),
                                  bufs["variation"].data_ptr(), bufs["count"].data_ptr(),
                                  min_neighbours=min_neighbours, orient=orient, d_toward=d_toward, toward_stride=ts)
    torch.cuda.synchronize()
    raw = {name: b.cpu().numpy() for name, b in bufs.items()}
    for name, w in width.items():
        assert (raw[name][w:] == SENTINEL).all(), name
    if n:
        assert dpts.cpu().numpy().tobytes() == pa.tobytes()
    if dtw is not None:
        assert dtw.cpu().numpy().tobytes() == tw.tobytes()
    return {"normal": raw["normal"][:12 * n].view(np.float32).reshape(n, 3).copy(),
            "variation": raw["variation"][:4 * n].view(np.float32).copy(),
            "count": raw["count"][:4 * n].view(np.int32).copy(), "stats": st}


def assert_equal(got, want):
    for name in ("count", "variation", "normal"):
        assert CR.same_bits(got[name], want[name]), name
    st = got["stats"]
    assert {c: st[c] for c in NR.COUNTS} == want["stats"]
    assert st["estimated"] + st["sparse"] + st["degenerate"] == st["points"]
    assert st["knn_ms"] >= 0 and st["normals_ms"] >= 0 and st["grid_cells"] >= 1


def reference(points, k, max_dist, min_neighbours=3, viewpoint=None, directions=None):
    if viewpoint is not None:
        return NR.normals(points, k, max_dist, min_neighbours, NR.ORIENT_VIEWPOINT, viewpoint)
    if directions is not None:
        w = np.asarray(points)["normal"] if isinstance(directions, str) else directions
        return NR.normals(points, k, max_dist, min_neighbours, NR.ORIENT_DIRECTION, w)
    return NR.normals(points, k, max_dist, min_neighbours)


def check(eng, points, k, max_dist, want=None, **kw):
    """both forms against the reference (computed once unless given), which is returned"""
    if want is None:
        want = reference(points, k, max_dist, **kw)
    for form in FORMS:
        assert_equal(normals(eng, form, points, k, max_dist, **kw), want)
    return want


# ---- 1. counts, every list width and both ends of min_neighbours -------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_tiny_clouds(eng, n):
    p = surface(4, 5)[:n]
    want = check(eng, p, 3, 2.0)
    assert want["stats"]["estimated"] == (n if n >= 3 else 0) and want["stats"]["sparse"] == (n if n < 3 else 0)
    if n == 4:
        check(eng, p, 4, 2.0, min_neighbours=4)


@pytest.mark.parametrize("k", [3, 8, 9, 16, 17, 32])
def test_every_list_width_with_ragged_waves(eng, k):
    p = surface(301, 40 + k)
    # about 10 points within the radius: rows are full for k <= 9 and short above
    want = check(eng, p, k, 0.1)
    full = int((want["count"] == k).sum())
    assert (full > 200) if k <= 8 else (full < 100) if k >= 16 else True
    assert want["stats"]["estimated"] > 290
    want = check(eng, p, k, 0.1, min_neighbours=k)
    assert want["stats"]["sparse"] == 301 - full and want["stats"]["estimated"] == full


def test_two_thousand_points_sparse_ones_and_non_finite_ones(eng):
    p = holed(2003, 7)
    want = check(eng, p, 16, 0.03)  # about 6 points within the radius
    s = want["stats"]
    assert s["skipped"] == 21 + 10 and 50 < s["sparse"] < 1500 and s["estimated"] > 400
    assert (want["count"] < 16).sum() > 1900
    bad = ~np.isfinite(p).all(axis=1)
    assert (want["count"][bad] == 0).all() and (want["normal"][bad] == 0).all() and np.isinf(want["variation"][bad]).all()
    est = np.isfinite(want["variation"])
    assert (want["variation"][est] >= 0).all() and (want["variation"][est] <= np.float32(1 / 3)).all()
    length = np.linalg.norm(want["normal"][est].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 1e-6
    # the surface is close to z = const, its noise a third of the radius: most
    # normals lean to +z (the canonical sign)
    assert np.median(want["normal"][est][:, 2]) > 0.5


# ---- 2. strides -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.dtype([("pos", "<f4", 3), ("w", "<f4")]), N.FUSED_DTYPE,
                                   np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("rest", "u1", 40)]), N.PATCH_DTYPE],
                         ids=["16", "40", "64", "80"])
def test_records_of_other_strides(eng, dtype):
    p = surface(300, 11)
    rng = np.random.default_rng(12)
    rec = np.frombuffer(rng.integers(0, 256, len(p) * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()
    rec["pos"] = p
    want = NR.normals(p, 8, 0.12)  # stride 12
    check(eng, p, 8, 0.12, want=want)
    check(eng, rec, 8, 0.12, want=want)


# ---- 3. degenerate shapes ---------------------------------------------------------------------

def test_coincident_points_are_degenerate(eng):
    p = np.tile(np.float32([[0.25, -1.5, 3.0]]), (70, 1))
    want = check(eng, p, 8, 0.5)
    assert want["stats"] == dict(points=70, skipped=0, estimated=0, sparse=0, degenerate=70, flipped=0, unoriented=0)
    assert (want["normal"] == 0).all() and np.isinf(want["variation"]).all() and (want["count"] == 8).all()


def test_duplicates_under_other_indices(eng):
    p = duplicated(150, 13)  # every third point three times
    want = check(eng, p, 8, 0.15)
    assert want["stats"]["estimated"] == len(p)
    assert CR.same_bits(want["normal"][150:200], want["normal"][200:250])


def test_collinear_points(eng):
    want = check(eng, line(40), 8, 0.2)
    # the direction of least spread is any normal of the line: the reference says which
    d = LINE_DIR / np.sqrt(6)
    assert want["stats"]["estimated"] == 40 and np.abs(want["normal"].astype(np.float64) @ d).max() < 1e-6
    assert want["variation"].max() < 1e-10


def test_coplanar_points_on_an_axis_plane_and_on_a_tilted_one(eng):
    want = check(eng, lattice(12), 9, 1.5)
    assert CR.same_bits(want["normal"], np.tile(np.float32([[0, 0, 1]]), (144, 1))) and (want["variation"] == 0).all()
    want = check(eng, tilted(200, 14), 16, 0.3)
    nrm = np.cross(TILT_A, TILT_B) / np.linalg.norm(np.cross(TILT_A, TILT_B))
    cos = np.abs(want["normal"][np.isfinite(want["variation"])].astype(np.float64) @ nrm)
    # a unit vector rounded to float32 is 2^-24 off in every component, and so in length
    assert cos.min() > 1 - 1e-6 and want["variation"][np.isfinite(want["variation"])].max() < 1e-10


def test_a_cloud_far_from_the_origin(eng):
    want = check(eng, far(300, 15), 16, 1.0)  # a float32 step is 2^-10 there
    assert want["stats"]["estimated"] > 290
    # without the centring the sums would be 1e8 and their differences noise: the
    # normals still follow the surface
    est = np.isfinite(want["variation"])
    assert np.median(want["normal"][est][:, 2]) > 0.8 and want["variation"][est].max() <= np.float32(1 / 3)


# ---- 4. orientation ---------------------------------------------------------------------------

def test_one_viewpoint_and_one_per_point(eng):
    c = SPHERE_CENTRE
    p = sphere(400, 16, c)
    want = check(eng, p, 12, 0.5, viewpoint=c)
    s = want["stats"]
    assert s["estimated"] == 400 and 100 < s["flipped"] < 300 and s["unoriented"] == 0
    inward = ((p.astype(np.float64) - c) * want["normal"]).sum(axis=1)
    assert (inward < 0).all()
    # per point: twice the position is outside the sphere for a point of the far half, every entry its own
    per = (c + 2 * (p - c)).astype(np.float32)
    want2 = check(eng, p, 12, 0.5, viewpoint=per)
    assert CR.same_bits(want2["normal"], -want["normal"]) and want2["stats"]["flipped"] == 400 - s["flipped"]


def test_directions_in_place_planted_zero_and_non_finite(eng):
    p = surface(300, 17)
    rec = np.zeros(300, N.FUSED_DTYPE)
    rec["pos"] = p
    rng = np.random.default_rng(18)
    rec["normal"] = rng.standard_normal((300, 3)).astype(np.float32)
    rec["normal"][7] = np.float32([np.nan, 0, 1])
    rec["normal"][9] = np.float32([0, np.inf, 0])
    rec["normal"][11] = 0  # s == 0
    want = check(eng, rec, 10, 0.15, directions=OWN)
    s = want["stats"]
    assert s["unoriented"] == 3 and 100 < s["flipped"] < 200
    plain = NR.normals(p, 10, 0.15)
    for i in (7, 9, 11):
        assert CR.same_bits(want["normal"][i], plain["normal"][i])
    # the same entries from an array of their own
    check(eng, rec, 10, 0.15, want=want, directions=rec["normal"].copy())
    # a lattice in z = 0 has exactly (0, 0, 1): a direction in the plane, or a viewpoint at the same height, is s == 0
    flat = lattice(6, 2.0)
    w = np.tile(np.float32([[1, -3, 0]]), (36, 1))
    w[::2] = np.float32([0, 0, -1])
    want = check(eng, flat, 9, 1.5, directions=w)
    assert want["stats"]["unoriented"] == 18 and want["stats"]["flipped"] == 18
    assert CR.same_bits(want["normal"][0], np.float32([-0.0, -0.0, -1])) and CR.same_bits(want["normal"][1], np.float32([0, 0, 1]))
    want = check(eng, flat, 9, 1.5, viewpoint=np.float32([40, 50, 2]))
    assert want["stats"]["unoriented"] == 36 and want["stats"]["flipped"] == 0


# ---- 5. errors --------------------------------------------------------------------------------

PTS = np.zeros((4, 3), np.float32)
TOW = np.zeros((4, 3), np.float32)


def call(eng, p=PTS.ctypes.data, n=4, stride=12, max_dist=0.5, k=3, min_nb=3, flags=0, opts=True, toward=None,
         ts=0, normal=True, var=None, count=None, device=False):
    """the raw library call; the device form is refused before any address is used"""
    co = N.DpCloudNormalsOptions(max_dist, k, min_nb, flags)
    args = [eng._ctx, p, n, stride, ctypes.byref(co) if opts else None, toward, ts]
    if device:
        return N.lib.dp_cloud_normals_device(*args, ctypes.c_void_p(4096) if normal is True else normal, var, count,
                                             None, None)
    pn = ctypes.c_void_p(1)
    rc = N.lib.dp_cloud_normals(*args, ctypes.byref(pn) if normal else None, var, count, None)
    assert rc == N.DP_OK or pn.value == 1  # a refused call leaves the result alone
    return rc


@pytest.mark.parametrize("device", [False, True], ids=FORMS)
def test_refusals_name_the_argument(eng, device):
    tw = ctypes.c_void_p(TOW.ctypes.data)
    cases = [
        (dict(n=-1), "n must"), (dict(n=2**31), "n must"), (dict(p=None), "points"), (dict(stride=8), "stride"),
        (dict(stride=14), "stride"), (dict(opts=False), "opts"), (dict(max_dist=0.0), "max_dist"),
        (dict(max_dist=float("nan")), "max_dist"), (dict(max_dist=float("inf")), "max_dist"), (dict(k=2), "k must"),
        (dict(k=33), "k must"), (dict(min_nb=2), "min_neighbours"), (dict(min_nb=4), "min_neighbours"),
        (dict(flags=3, toward=tw), "flags"), (dict(flags=4), "flags"), (dict(flags=-2**31), "flags"),
        (dict(flags=1), "toward"), (dict(flags=2), "toward"), (dict(toward=tw), "toward"), (dict(ts=12), "toward"),
        (dict(flags=1, toward=tw, ts=8), "toward_stride"), (dict(flags=2, toward=tw, ts=14), "toward_stride"),
        (dict(flags=1, toward=tw, ts=-12), "toward_stride"), (dict(normal=None), "normal"),
    ]
    for kw, name in cases:
        assert call(eng, device=device, **kw) == N.DP_E_ARG, kw
        msg = N.lib.dp_last_error(eng._ctx).decode()
        assert msg.startswith("dp_cloud_normals_device:" if device else "dp_cloud_normals:") and name in msg, (kw, msg)
    if device:
        same = ctypes.c_void_p(PTS.ctypes.data)
        for kw in (dict(normal=same), dict(var=same), dict(count=same), dict(var=ctypes.c_void_p(4096)),
                   dict(var=ctypes.c_void_p(8192), count=ctypes.c_void_p(8192)),
                   dict(flags=2, toward=tw, ts=12, count=tw)):
            assert call(eng, device=True, **kw) == N.DP_E_ARG, kw
            assert "output" in N.lib.dp_last_error(eng._ctx).decode()
    # n = 0 with NULL arrays is legal
    assert call(eng, device=device, p=None, n=0, normal=None if device else True) == N.DP_OK


def test_python_layer_refuses_before_the_library(eng):
    for kw in (dict(max_dist=0.0), dict(k=2), dict(k=33), dict(min_neighbours=2), dict(min_neighbours=5),
               dict(viewpoint=[0, 0, 0], directions=TOW), dict(viewpoint=[0, 0]), dict(directions=TOW[:3]),
               dict(directions=True), dict(directions=False)):
        with pytest.raises(ValueError):
            eng.cloud_normals(PTS, **dict(dict(k=4, max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.cloud_normals_device(64, 3, 12, 4, 0.5, 64)  # an output equals the input
    with pytest.raises(ValueError):
        eng.cloud_normals_device(64, 3, 12, 4, 0.5, 0)  # no d_normal
    with pytest.raises(ValueError):
        eng.cloud_normals_device(64, 3, 12, 4, 0.5, 128, orient="viewpoint")  # no d_toward
    with pytest.raises(ValueError):
        eng.cloud_normals_device(64, 3, 12, 4, 0.5, 128, d_toward=256)  # no orient mode


# ---- 6. the shared scratch is still the other calls' ------------------------------------------

def test_knn_and_clean_after_normals_on_the_same_context(eng):
    p = holed(500, 19)
    want = check(eng, p, 16, 0.1)
    got = eng.cloud_knn(p, p[:200], 5, 0.08)
    ref = KR.knn(p, p[:200], 5, 0.08)
    for name in ("index", "dist", "count"):
        assert CR.same_bits(got[name], ref[name]), name
    assert {c: got["stats"][c] for c in KR.KNN_COUNTS} == ref["stats"]
    got = eng.cloud_clean(p, 8, 0.1, std_mul=1.0)
    ref = KR.clean(p, 8, 0.1, std_mul=1.0)
    for name in ("keep", "mean_dist", "map"):
        assert CR.same_bits(got[name], ref[name]), name
    assert {c: got["stats"][c] for c in KR.CLEAN_COUNTS} == ref["stats"] and got["stats"]["mu"] == ref["mu"]
    assert got["points"].tobytes() == ref["points"].tobytes()
    # and the other way round
    assert_equal(eng.cloud_normals(p, 16, max_dist=0.1), want)
