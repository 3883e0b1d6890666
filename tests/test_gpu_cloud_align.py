"""dp_cloud_align and dp_cloud_transform on the GPU against the brute-force CPU
reference (tests/cloudalign_ref.py, restated from the header's spec): the matrix,
the scale, every trace record, the last pass's index and dist and every integer
statistic bit for bit, in the host and the device form; the evaluation helpers
and the densify CLI on top of them."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudalign_ref as AR
import cloudknn_ref as KR
import cloudnearest_ref as CR
from test_cloud_align_cpu import rotation
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]
F = np.float64
MOVE = np.hstack([rotation([1, 2, 3], 0.02), [[0.004], [-0.003], [0.005]]])


@pytest.fixture(scope="module")
def eng():
    # no views are ever set on this engine
    with dp.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def cube():
    return np.random.default_rng(20261021).random((700, 3), dtype=np.float32)


def run_align(eng, form, source, target, max_dist, **kw):
    """cloud_align in either form as the dict Engine.cloud_align returns with
    correspondences; the device form writes index and dist into sentinel-filled
    buffers with slack behind them and checks that no input was written"""
    if form == "host":
        return eng.cloud_align(source, target, max_dist, correspondences=True, **kw)
    import torch

    sa, sp, n, ss = pmvs._cloud_points("test", source)
    ta, tp, nt, ts = pmvs._cloud_points("test", target)
    ds = to_device(sa.reshape(-1)) if n else None
    dt = to_device(ta.reshape(-1)) if nt else None
    bufs = {name: torch.full((4 * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for name in ("index", "dist")}
    torch.cuda.synchronize()
    out = eng.cloud_align_device(ds.data_ptr() + (sp - sa.ctypes.data) if n else None, n, ss,
                                 dt.data_ptr() + (tp - ta.ctypes.data) if nt else None, nt, ts, max_dist,
                                 d_index=bufs["index"].data_ptr(), d_dist=bufs["dist"].data_ptr(), **kw)
    torch.cuda.synchronize()
    for name, dtype in (("index", np.int32), ("dist", np.float32)):
        raw = bufs[name].cpu().numpy()
        assert (raw[4 * n:] == SENTINEL).all(), name
        out[name] = raw[:4 * n].view(dtype).copy()
    if n:
        assert ds.cpu().numpy().tobytes() == sa.tobytes()
    if nt:
        assert dt.cpu().numpy().tobytes() == ta.tobytes()
    return out


def assert_equal(got, want):
    assert CR.same_bits(got["matrix"], want["matrix"]), (got["matrix"], want["matrix"])
    assert np.float64(got["scale"]).tobytes() == np.float64(want["scale"]).tobytes()
    assert got["trace"].dtype == AR.STEP_DTYPE and got["trace"].tobytes() == want["trace"].tobytes(), \
        (got["trace"], want["trace"])
    for name in ("index", "dist"):
        assert CR.same_bits(got[name], want[name]), name
    st = got["stats"]
    assert {c: st[c] for c in AR.COUNTS} == want["stats"]
    assert st["matched"] + st["unmatched"] == st["queries"] and st["grid_cells"] >= 1
    assert st["grid_ms"] >= 0 and st["iterate_ms"] >= 0


def check(eng, source, target, max_dist, **kw):
    """both forms against the reference (computed once); returns the reference's result"""
    want = AR.align(source, target, max_dist, correspondences=True, **kw)
    for form in FORMS:
        assert_equal(run_align(eng, form, source, target, max_dist, **kw), want)
    return want


# ---- 1. sizes: every level of the sum tree ----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 65537])
def test_source_sizes(eng, n):
    rng = np.random.default_rng(n)
    if n > 1000:  # the third level of the tree against a small target: most sources match one of 100
        t = rng.random((100, 3), dtype=np.float32)
        x = AR.transform_positions(t[rng.integers(0, 100, n)] + (rng.random((n, 3), dtype=np.float32) - 0.5) * 0.02,
                                   np.linalg.inv(np.vstack([MOVE, [0, 0, 0, 1]]))[:3])
        want = check(eng, x, t, 0.05, iterations=2)
        assert want["stats"]["iterations_run"] == 2 and want["trace"]["matched"][0] > 60000
        return
    t = rng.random((max(n, 40), 3), dtype=np.float32)
    x = t[:n] + np.float32([0.003, -0.002, 0.001])
    want = check(eng, x, t, 0.1, iterations=3)
    assert want["stats"]["stop_reason"] == (AR.STOP_PAIRS if n < 3 else AR.STOP_ITERATIONS)
    assert want["trace"]["matched"][0] == n
    want = check(eng, x, t, 0.1, iterations=2, scale=True)
    if n == 3:
        assert want["stats"]["iterations_run"] == 2


@pytest.mark.parametrize("scale", [False, True], ids=["rigid", "scale"])
def test_a_planted_motion(eng, cube, scale):
    truth = MOVE.copy()
    if scale:
        truth[:, :3] *= 1.01
    q = AR.transform_positions(cube, truth)
    want = check(eng, cube, q[np.random.default_rng(5).permutation(700)], 0.15, iterations=6, scale=scale)
    assert np.abs(want["matrix"] - truth).max() < 1e-7 and want["trace"]["rms"][-1] < 1e-7
    assert want["trace"]["rms"][0] > 5e-3 and want["stats"]["iterations_run"] == 6


def test_a_cloud_to_itself_is_the_identity_bit_for_bit(eng, cube):
    want = check(eng, cube, cube, 0.05, iterations=3)
    assert want["matrix"].tobytes() == np.eye(3, 4).tobytes() and (want["trace"]["rms"] == 0).all()
    got = eng.cloud_align(cube, cube, 0.05, iterations=3)
    assert got["matrix"].tobytes() == np.eye(3, 4).tobytes() and got["index"] is None and got["dist"] is None


# ---- 2. strides, pos not first --------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["packed", "stride16", "patch", "pos_last"])
def test_strides(eng, cube, layout):
    x, q = cube[:300], AR.transform_positions(cube[:400], MOVE)
    rng = np.random.default_rng(len(layout))
    dtype = {"packed": None, "stride16": N.MESH_VERTEX_DTYPE, "patch": N.PATCH_DTYPE,
             "pos_last": np.dtype([("tag", "<i4"), ("w", "<f4", 2), ("pos", "<f4", 3)])}[layout]

    def records(pos):
        if dtype is None:
            return pos
        a = np.frombuffer(rng.integers(0, 256, len(pos) * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()
        a["pos"] = pos
        return a

    xr, qr = records(x), records(q)
    if dtype is not None:
        assert pmvs._cloud_points("t", xr)[3] == dtype.itemsize
    if layout == "pos_last":
        assert pmvs._cloud_points("t", xr)[1] != xr.ctypes.data
    want = AR.align(x, q, 0.15, iterations=3, correspondences=True)
    for form in FORMS:
        assert_equal(run_align(eng, form, xr, qr, 0.15, iterations=3), want)


# ---- 3. ties, points that are not finite, nothing matched, too few ---------------------------------

def test_duplicated_targets_tie_to_the_lowest_index(eng, cube):
    q = AR.transform_positions(cube[:200], MOVE)
    t = np.concatenate([q, q, q[:50]])[np.random.default_rng(3).permutation(450)]
    want = check(eng, cube[:200], t, 0.15, iterations=4)
    final = AR.transform_positions(cube[:200], want["matrix"])
    d = np.linalg.norm(t.astype(F)[None] - final.astype(F)[:, None], axis=2)
    assert (want["index"] == d.argmin(axis=1)).all()  # argmin takes the first of equal minima


def test_nan_and_inf_on_both_sides(eng, cube):
    x, q = cube[:500].copy(), AR.transform_positions(cube[:500], MOVE)
    bad = np.float32([np.nan, np.inf, -np.inf])
    x[np.arange(0, 500, 7), np.arange(0, 500, 7) % 3] = bad[np.arange(0, 500, 7) % 3]
    q[np.arange(0, 500, 5), np.arange(0, 500, 5) % 3] = bad[np.arange(0, 500, 5) % 3]
    want = check(eng, x, q, 0.15, iterations=3, scale=True)
    assert want["stats"]["skipped_queries"] == 72 and want["stats"]["skipped_targets"] == 100
    assert (want["index"][::7] == -1).all() and np.isfinite(want["matrix"]).all()
    q[:] = bad[0]
    want = check(eng, x, q, 0.15, iterations=3)
    assert want["stats"]["targets"] == 0 and want["stats"]["stop_reason"] == AR.STOP_PAIRS


def test_nothing_matched_too_few_and_empty(eng, cube):
    want = check(eng, cube[:300], cube[:300] + np.float32(10), 0.1, iterations=4)
    assert want["stats"]["stop_reason"] == AR.STOP_PAIRS and want["stats"]["unmatched"] == 300
    assert want["trace"].tolist() == [(0, 0.0)] * 5
    # ten points matched, min_pairs = 11
    t = np.concatenate([cube[:10] + np.float32(0.001), cube[300:400] + np.float32(5)])
    want = check(eng, cube[:300], t, 0.01, iterations=4, min_pairs=11)
    assert want["stats"]["stop_reason"] == AR.STOP_PAIRS and want["trace"]["matched"].tolist() == [10, 0, 0, 0, 0]
    want = check(eng, cube[:300], t, 0.01, iterations=2, min_pairs=10)
    assert want["stats"]["iterations_run"] == 2
    init = np.hstack([rotation([0, 0, 1], 0.1), [[1.0], [2.0], [3.0]]])
    for a, b in ((cube[:0], cube), (cube[:5], cube[:0]), (cube[:0], cube[:0])):
        want = check(eng, a, b, 0.1, iterations=3, init=init)
        assert want["stats"]["stop_reason"] == AR.STOP_EMPTY and np.array_equal(want["matrix"], init)


# ---- 4. degenerate shapes, the mirror ---------------------------------------------------------------

def test_collinear_coplanar_coincident_and_mirrored_sources(eng, cube):
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = np.linspace(0, 1, 200)
    line[:, 1] = line[:, 0] * np.float32(0.3)
    plane = cube[:400].copy()
    plane[:, 2] = np.float32(0.5)
    for src in (line, plane):
        for scale in (False, True):
            want = check(eng, src, AR.transform_positions(src, MOVE), 0.1, iterations=3, scale=scale)
            assert want["stats"]["iterations_run"] == 3 and abs(AR.det3(want["matrix"] / want["scale"]) - 1) < 1e-9
    same = np.repeat(cube[:1], 300, axis=0)
    want = check(eng, same, cube, 2.0, iterations=3)
    assert want["stats"]["stop_reason"] == AR.STOP_DEGENERATE and want["trace"]["matched"].tolist() == [300, 0, 0, 0]
    mirrored = cube.copy()
    mirrored[:, 0] = np.float32(1) - mirrored[:, 0]
    for scale in (False, True):
        want = check(eng, cube, mirrored, 0.3, iterations=3, scale=scale)
        assert want["stats"]["iterations_run"] == 3 and abs(AR.det3(want["matrix"][:, :3] / want["scale"]) - 1) < 1e-9


# ---- 5. init, the early stop, one iteration --------------------------------------------------------------

def test_init_rms_tol_and_one_iteration(eng, cube):
    big = np.hstack([rotation([0, 1, 0], 0.7), [[0.5], [-0.25], [1.0]]])
    q = AR.transform_positions(cube, big)
    assert check(eng, cube, q, 0.05, iterations=3)["trace"]["matched"][0] < 100  # hopeless from the identity
    near = np.hstack([rotation([0, 1, 0], 0.69), [[0.5], [-0.25], [1.0]]])
    want = check(eng, cube, q, 0.05, iterations=8, init=near)
    assert np.abs(want["matrix"] - big).max() < 1e-6 and want["trace"]["matched"][-1] == 700
    want = check(eng, cube, q, 0.05, iterations=12, init=near, rms_tol=1e-7)
    k = want["stats"]["iterations_run"]
    assert want["stats"]["stop_reason"] == AR.STOP_RMS and 2 <= k < 12
    assert (want["trace"]["matched"][:k + 1] > 0).all() and want["trace"][k + 1:].tolist() == [(0, 0.0)] * (12 - k)
    want = check(eng, cube, AR.transform_positions(cube, MOVE), 0.15, iterations=1, scale=True)
    assert want["stats"]["iterations_run"] == 1 and len(want["trace"]) == 2
    assert want["trace"]["rms"][1] < 0.1 * want["trace"]["rms"][0]


# ---- 6. dp_cloud_transform ----------------------------------------------------------------------------------

def run_transform(eng, form, points, matrix, normals=False):
    if form == "host":
        return eng.cloud_transform(points, matrix, normals)
    import torch

    pa, _, n, stride = pmvs._cloud_points("test", points)
    off = pmvs._cloud_normal_offset("test", pa, normals)
    d_in = to_device(pa.reshape(-1))
    nbytes = n * stride
    if form == "in_place":
        eng.cloud_transform_device(d_in.data_ptr(), n, stride, matrix, d_in.data_ptr(), off)
        torch.cuda.synchronize()
        return d_in.cpu().numpy().view(pa.dtype).reshape(pa.shape).copy()
    d_out = torch.full((nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.cloud_transform_device(d_in.data_ptr(), n, stride, matrix, d_out.data_ptr(), off)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[nbytes:] == SENTINEL).all() and d_in.cpu().numpy().tobytes() == pa.tobytes()
    return raw[:nbytes].view(pa.dtype).reshape(pa.shape).copy()


@pytest.mark.parametrize("form", ["host", "device", "in_place"])
def test_transform_with_and_without_normals(eng, cube, form):
    M = np.hstack([1.7 * rotation([2, -1, 1], 1.1), [[3.0], [-2.0], [0.5]]])
    M[0, 1] += 0.2  # not a similarity: the normals must be renormalised
    rng = np.random.default_rng(9)
    for dtype in (N.FUSED_DTYPE, N.PATCH_DTYPE):
        rec = np.frombuffer(rng.integers(0, 256, 600 * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()
        rec["pos"] = cube[:600]
        nrm = rng.standard_normal((600, 3)).astype(np.float32)
        rec["normal"] = nrm
        rec["pos"][5] = [np.nan, 0, 0]
        rec["pos"][6] = [0, np.inf, 0]
        rec["normal"][7] = 0  # a zero normal stays
        rec["normal"][8] = [np.nan, 1, 0]
        rec["normal"][5] = [0, 0, 2]  # the normal of a point that is not finite is still treated
        for normals in (False, True):
            got = run_transform(eng, form, rec, M, normals)
            want = AR.transform(rec, M, normals)
            assert got.dtype == rec.dtype and got.tobytes() == want.tobytes(), (dtype.itemsize, normals)
        assert want["pos"][5].tobytes() == rec["pos"][5].tobytes() and want["normal"][7].tolist() == [0, 0, 0]
        assert abs(np.linalg.norm(want["normal"][5].astype(F)) - 1) < 1e-6
    got = run_transform(eng, form, cube, M)
    assert CR.same_bits(got, AR.transform(cube, M))
    if form == "host":
        assert len(eng.cloud_transform(cube[:0], M)) == 0
        with pytest.raises(ValueError):
            eng.cloud_transform(cube, M, normals=True)
        with pytest.raises(ValueError):
            eng.cloud_transform(cube, np.eye(3))


# ---- 7. the searches after a registration: the scratch is shared -------------------------------------------

def test_nearest_and_knn_after_an_align_call(eng, cube):
    q, t = cube[:500], cube[200:] + np.float32(0.01)
    eng.cloud_align(cube, AR.transform_positions(cube[:300], MOVE), 0.1, iterations=3)
    near, want = eng.cloud_nearest(q, t, 0.08, hist_bins=16), CR.nearest(q, t, 0.08, hist_bins=16)
    assert CR.same_bits(near["index"], want["index"]) and CR.same_bits(near["dist"], want["dist"])
    assert (near["hist"] == want["hist"]).all() and {c: near["stats"][c] for c in CR.COUNTS} == want["stats"]
    eng.cloud_align(q, t, 0.05, iterations=2, scale=True)
    knn, want = eng.cloud_knn(q, t, 5, 0.08), KR.knn(q, t, 5, 0.08)
    for name in ("index", "dist", "count"):
        assert CR.same_bits(knn[name], want[name]), name
    assert {c: knn["stats"][c] for c in KR.KNN_COUNTS} == want["stats"]


# ---- 8. refusals ---------------------------------------------------------------------------------------------

def test_refusals(eng, cube):
    import ctypes

    ao = N.DpCloudAlignOptions(0.5, 2, 3, 0, 0.0)
    M, s, trace = (ctypes.c_double * 12)(), ctypes.c_double(7.0), (N.DpCloudAlignStep * 3)()
    pts = np.zeros((4, 3), np.float32)
    nan_init = (ctypes.c_double * 12)(*([float("nan")] + [0.0] * 11))

    def call(device, opts=ao, src=pts.ctypes.data, n=4, ss=12, nt=4, ts=12, init=None, matrix=M, index=None, dist=None):
        args = [eng._ctx, src, n, ss, pts.ctypes.data, nt, ts, ctypes.byref(opts) if opts else None, init, matrix,
                ctypes.byref(s), trace]
        if device:
            return N.lib.dp_cloud_align_device(*args, index, dist, None, None)
        return N.lib.dp_cloud_align(*args, index, dist, None)

    def opts(**kw):
        base = dict(max_dist=0.5, iterations=2, min_pairs=3, flags=0, rms_tol=0.0)
        base.update(kw)
        return N.DpCloudAlignOptions(*[base[k] for k in ("max_dist", "iterations", "min_pairs", "flags", "rms_tol")])

    for device in (False, True):
        who = "dp_cloud_align_device:" if device else "dp_cloud_align:"
        cases = [(dict(n=-1), "n_"), (dict(nt=2**31), "n_"), (dict(src=None), "must be given"), (dict(ss=8), "stride"),
                 (dict(ts=14), "target_stride"), (dict(opts=None), "opts"), (dict(opts=opts(max_dist=0.0)), "max_dist"),
                 (dict(opts=opts(max_dist=float("nan"))), "max_dist"), (dict(opts=opts(iterations=0)), "iterations"),
                 (dict(opts=opts(iterations=1001)), "iterations"), (dict(opts=opts(min_pairs=2)), "min_pairs"),
                 (dict(opts=opts(rms_tol=-1.0)), "rms_tol"), (dict(opts=opts(rms_tol=float("inf"))), "rms_tol"),
                 (dict(opts=opts(flags=2)), "flags"), (dict(opts=opts(flags=-1)), "flags"),
                 (dict(init=nan_init), "init"), (dict(matrix=None), "matrix"),
                 (dict(index=ctypes.c_void_p(4096)), "together")]
        for kw, word in cases:
            assert call(device, **kw) == N.DP_E_ARG, kw
            msg = N.lib.dp_last_error(eng._ctx).decode()
            assert msg.startswith(who) and word in msg, (kw, msg)
        assert s.value == 7.0
    out = ctypes.c_void_p(1)
    for kw, word in ((dict(n=-1), "n must"), (dict(stride=10), "stride"), (dict(matrix=None), "matrix"),
                     (dict(matrix=nan_init), "finite"), (dict(off=8), "normal_offset"), (dict(off=4), "normal_offset"),
                     (dict(stride=16, off=12), "normal_offset")):
        a = dict(dict(n=4, stride=12, matrix=M, off=-1), **kw)
        assert N.lib.dp_cloud_transform(eng._ctx, pts.ctypes.data, a["n"], a["stride"], a["matrix"], a["off"],
                                        ctypes.byref(out)) == N.DP_E_ARG
        assert word in N.lib.dp_last_error(eng._ctx).decode() and out.value == 1
        assert N.lib.dp_cloud_transform_device(eng._ctx, pts.ctypes.data, a["n"], a["stride"], a["matrix"], a["off"],
                                               ctypes.c_void_p(4096), None) == N.DP_E_ARG
    for kw in (dict(max_dist=0.0), dict(iterations=0), dict(min_pairs=2), dict(scale=1), dict(init=np.eye(3))):
        with pytest.raises(ValueError):
            eng.cloud_align(cube, cube, **dict(dict(max_dist=0.5), **kw))
    with pytest.raises(ValueError):
        eng.cloud_align_device(64, 3, 12, 128, 3, 12, 0.5, d_index=64, d_dist=512)  # an output equals an input
    with pytest.raises(ValueError):
        eng.cloud_align_device(64, 3, 12, 128, 3, 12, 0.5, d_index=256)  # one without the other


# ---- 9. the evaluation helpers ------------------------------------------------------------------------------

def test_cloud_compare_with_align_undoes_a_planted_offset(eng):
    rng = np.random.default_rng(21)
    xy = rng.random((3000, 2))
    truth = np.column_stack([xy, 0.1 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])]).astype(np.float32)
    recon = truth + (rng.standard_normal((3000, 3)) * 0.0005).astype(np.float32)
    tau = 0.004
    off = np.hstack([rotation([1, 1, 0], 0.01), [[0.012], [-0.008], [0.02]]])
    moved = AR.transform_positions(recon, off)
    unmoved = dp.cloud_compare(eng, recon, truth, tau)
    before = dp.cloud_compare(eng, moved, truth, tau)
    kw = dict(iterations=10, max_dist=0.08)
    after = dp.cloud_compare(eng, moved, truth, tau, align=kw)
    assert before["fscore"] < 0.1 < 0.9 < unmoved["fscore"]
    assert abs(after["fscore"] - unmoved["fscore"]) < 0.01
    assert set(before) == set(unmoved) == {"accuracy", "completeness", "fscore"} and set(after) == set(before) | {"align"}
    assert set(after["align"]) == {"matrix", "scale", "trace", "stats"}
    # the same pipeline on the reference, bit for bit
    want = AR.align(moved, truth, 0.08, iterations=10)
    assert CR.same_bits(after["align"]["matrix"], want["matrix"])
    assert after["align"]["trace"].tobytes() == want["trace"].tobytes() and after["align"]["scale"] == want["scale"]
    assert {c: after["align"]["stats"][c] for c in AR.COUNTS} == want["stats"]
    ref = CR.compare(AR.transform_positions(moved, want["matrix"]), truth, tau)
    CR.assert_compare({k: after[k] for k in before}, ref)
    assert after["accuracy"]["within_tau"] == ref["accuracy"]["within_tau"]
    assert dp.cloud_compare(eng, moved, truth, tau, align=None) == before  # key for key
    # a mesh over the same vertices: they ride along with the same motion
    tris = np.arange(3000, dtype=np.int32).reshape(-1, 3)
    m0 = dp.mesh_compare(eng, moved, tris, truth, tau)
    m1 = dp.mesh_compare(eng, moved, tris, truth, tau, align=kw)
    assert set(m1) == set(m0) | {"align"} and CR.same_bits(m1["align"]["matrix"], want["matrix"])
    assert m1["accuracy"] == after["accuracy"] and m1["fscore"] > m0["fscore"]
    p = dp.PMVS()
    assert p.evaluate(truth, tau, cloud=moved, align=kw)["accuracy"] == after["accuracy"]
    assert p.evaluate(truth, tau, cloud=moved) == before


# ---- 10. densify --evaluate truth.xyz --eval-align --------------------------------------------------------

def test_cli_registers_before_it_measures(tmp_path):
    from test_cli import run
    from test_gpu_cloud_nearest_cli import read_ply_positions
    from densepoints_amd import synth

    d = str(tmp_path)
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    cfg = synth.config(4, 160, 120, 1)
    seeds = synth.seeds(cfg, synth.cameras(cfg))
    lo, hi = seeds[:, :2].min(axis=0), seeds[:, :2].max(axis=0)
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 96), np.linspace(lo[1], hi[1], 72), indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
    z, _ = synth.surface(cfg, xy)
    truth = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    pitch = max((hi[0] - lo[0]) / 95, (hi[1] - lo[1]) / 71)
    tau = float(np.float32(2 * pitch))
    # the truth in another frame: a small planted motion, well within the search radius
    ext = float(np.linalg.norm(hi - lo))
    planted = np.hstack([rotation([0.2, -0.3, 1], 0.01), np.array([[1.0], [-0.7], [0.8]]) * 1.5 * pitch])
    moved = AR.transform_positions(truth, planted)
    path = os.path.join(d, "truth_moved.xyz")
    with open(path, "w") as f:
        for p in moved:
            f.write("%.9g %.9g %.9g\n" % tuple(float(c) for c in p))
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"))
    pts, fused, mesh = (str(tmp_path / n) for n in ("points.ply", "fused.ply", "mesh.ply"))
    common = (*base, "-o", pts, "--fuse", fused, "--mesh", mesh, "--mesh-dim", "40", "--evaluate", path, "--eval-tau",
              "%.17g" % tau)
    plain = json.loads(run(*common).stdout)
    before = {n: open(p, "rb").read() for n, p in (("pts", pts), ("fused", fused), ("mesh", mesh))}
    report = json.loads(run(*common, "--eval-align", "--eval-align-iterations", "20").stdout)
    assert "align" not in plain and sorted(report["align"]) == ["iterations", "matched", "matrix", "rms", "rms_before",
                                                                 "scale"]
    al = report["align"]
    assert len(al["matrix"]) == 12 and al["scale"] == 1.0 and 1 <= al["iterations"] <= 20 and al["matched"] > 0
    assert al["rms"] < al["rms_before"] and ext > 0
    # the files are what they were: the transform went to copies
    assert before == {n: open(p, "rb").read() for n, p in (("pts", pts), ("fused", fused), ("mesh", mesh))}
    # the estimate is cloud_align's on the written patches, and every entry is cloud_compare's on the moved cloud
    with dp.Engine(device=0) as eng:
        want = eng.cloud_align(read_ply_positions(pts), moved, 10 * tau, iterations=20)
        assert np.array_equal(np.array(al["matrix"]).reshape(3, 4), want["matrix"])
        assert al["matched"] == want["trace"]["matched"][want["stats"]["iterations_run"]]
        assert al["rms_before"] == want["trace"]["rms"][0] and al["iterations"] == want["stats"]["iterations_run"]
        for name, p in (("patches", pts), ("fused", fused), ("mesh_vertices", mesh)):
            cloud = eng.cloud_transform(read_ply_positions(p), want["matrix"])
            ref = dp.cloud_compare(eng, cloud, moved, tau)
            got = report["evaluate"][name]
            got = {k: ({f: float("nan") if x is None else x for f, x in v.items()} if isinstance(v, dict) else v)
                   for k, v in got.items()}
            CR.assert_compare(got, ref)
    # without --eval-align nothing of the report changes
    again = json.loads(run(*common).stdout)

    def strip(r):  # the times, at every depth
        return {k: strip(v) if isinstance(v, dict) else v for k, v in r.items() if k != "ms" and not k.endswith("_ms")}

    assert strip(again) == strip(plain)
