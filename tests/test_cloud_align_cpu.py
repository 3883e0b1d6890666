"""dp_cloud_align and dp_cloud_transform without a GPU: the reference
(tests/cloudalign_ref.py) on hand-worked cases and planted motions, the
multi-channel tree against pairwise_sum, the Python layer's argument checks
against the header's error lists, the ctypes mirrors against the header, and the
error returns that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudalign_ref as AR
import cloudknn_ref as KR
from test_cloud_knn_cpu import header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float64


def f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def rotation(axis, angle):
    a = np.asarray(axis, F) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@pytest.fixture(scope="module")
def cube():
    return np.random.default_rng(20261021).random((300, 3), dtype=np.float32)


# ---- hand-worked cases ---------------------------------------------------------------------

def test_three_points_and_their_translate():
    x = f32([[0, 0, 0], [3, 0, 0], [0, 6, 0]])  # the means (1, 2, 0) and every centred value are exact
    q = x + np.float32([0.25, -0.125, 0.5])
    r = AR.align(x, q, 1.0, iterations=1, correspondences=True)
    assert r["trace"]["matched"].tolist() == [3, 3]
    assert r["trace"]["rms"][0] == np.sqrt(F(0.25 ** 2 + 0.125 ** 2 + 0.5 ** 2)) and r["trace"]["rms"][1] == 0.0
    assert np.array_equal(r["matrix"], np.hstack([np.eye(3), [[0.25], [-0.125], [0.5]]]))
    assert r["scale"] == 1.0 and r["index"].tolist() == [0, 1, 2] and r["dist"].tolist() == [0.0, 0.0, 0.0]
    assert r["stats"] == dict(queries=3, targets=3, skipped_queries=0, skipped_targets=0, matched=3, unmatched=0,
                              iterations_run=1, stop_reason=AR.STOP_ITERATIONS)


def test_a_cloud_registered_to_itself_is_exactly_the_identity(cube):
    info = {}
    r = AR.align(cube, cube, 0.05, iterations=3, info=info)
    assert r["matrix"].tobytes() == np.eye(3, 4).tobytes()  # bit for bit: no -0.0 either
    assert r["scale"] == 1.0 and (r["trace"]["matched"] == 300).all() and (r["trace"]["rms"] == 0.0).all()
    # with x == q, S is symmetric bit for bit: the first row of N is zero off the diagonal before the
    # sweeps, so no rotation ever touches row 0 and column 0 of V stays e0
    _, m, mux, muq, S, Sx, _ = AR.one_pass(cube, cube, AR.IDENTITY, 0.05)
    N0 = AR.horn_matrix(S)
    assert [N0[0][k] for k in (1, 2, 3)] == [0.0, 0.0, 0.0] and mux == muq and m == 300
    Nd, V = AR.jacobi(N0)
    assert [V[k][0] for k in range(4)] == [1.0, 0.0, 0.0, 0.0] and Nd[0][0] == N0[0][0]
    assert all(Nd[0][0] > Nd[k][k] for k in (1, 2, 3))
    r = AR.align(cube, cube, 0.05, iterations=2, scale=True)
    assert r["scale"] == 1.0 and r["matrix"].tobytes() == np.eye(3, 4).tobytes()


def test_a_mirrored_cloud_gives_a_proper_rotation(cube):
    mirrored = cube.copy()
    mirrored[:, 0] = np.float32(1) - mirrored[:, 0]
    for scale in (False, True):
        r = AR.align(cube, mirrored, 0.3, iterations=4, scale=scale)
        A = r["matrix"][:, :3] / r["scale"]
        assert r["stats"]["iterations_run"] >= 1 and abs(np.linalg.det(A) - 1.0) < 1e-12
        assert np.abs(A @ A.T - np.eye(3)).max() < 1e-12


def test_stops_and_their_reasons(cube):
    far = cube + np.float32(10)
    r = AR.align(cube, far, 0.1, iterations=5, correspondences=True)
    assert r["stats"]["stop_reason"] == AR.STOP_PAIRS and r["stats"]["iterations_run"] == 0
    assert r["trace"].tolist() == [(0, 0.0)] * 6 and (r["index"] == -1).all() and np.isinf(r["dist"]).all()
    assert np.array_equal(r["matrix"], AR.IDENTITY) and r["stats"]["unmatched"] == 300
    # two matched pairs are below min_pairs = 3; four are below min_pairs = 5
    r = AR.align(cube[:2], cube[:2], 0.01, iterations=2)
    assert r["stats"]["stop_reason"] == AR.STOP_PAIRS and r["trace"]["matched"].tolist() == [2, 0, 0]
    r = AR.align(cube[:4], cube[:4], 0.01, iterations=2, min_pairs=5)
    assert r["stats"]["stop_reason"] == AR.STOP_PAIRS and r["stats"]["iterations_run"] == 0
    # empty clouds: init comes back, with the reason EMPTY
    init = np.hstack([rotation([0, 0, 1], 0.1), [[1.0], [2.0], [3.0]]])
    for a, b in ((cube[:0], cube), (cube, cube[:0]), (cube[:0], cube[:0])):
        r = AR.align(a, b, 0.1, iterations=3, init=init, correspondences=True)
        assert r["stats"]["stop_reason"] == AR.STOP_EMPTY and r["stats"]["iterations_run"] == 0
        assert np.array_equal(r["matrix"], init) and r["scale"] == 1.0 and r["trace"].tolist() == [(0, 0.0)] * 4
        assert len(r["index"]) == len(a) and (r["index"] == -1).all()
    # every matched source point the same: the centred source vanishes
    same = np.repeat(cube[:1], 5, axis=0)
    r = AR.align(same, cube[:50], 2.0, iterations=3)
    assert r["stats"]["stop_reason"] == AR.STOP_DEGENERATE and r["trace"]["matched"].tolist() == [5, 0, 0, 0]


def test_points_that_are_not_finite_take_no_part(cube):
    x, q = cube[:50].copy(), cube[:50].copy() + np.float32([0.01, 0, 0])
    x[3, 0], x[7, 2], q[11, 1], q[13, 0] = np.nan, np.inf, -np.inf, np.nan
    r = AR.align(x, q, 0.05, iterations=2, correspondences=True)
    s = r["stats"]
    assert (s["queries"], s["skipped_queries"], s["targets"], s["skipped_targets"]) == (48, 2, 48, 2)
    assert r["index"][3] == -1 and r["index"][7] == -1 and not np.isin([11, 13], r["index"]).any()
    assert np.isfinite(r["matrix"]).all() and abs(r["matrix"][0, 3] - 0.01) < 1e-6
    clean = np.delete(np.arange(50), [3, 7, 11, 13])
    # the bad points enter no sum: the same transform as without them, up to the tree's shape
    r2 = AR.align(x[clean], q[clean], 0.05, iterations=2)
    assert np.abs(r["matrix"] - r2["matrix"]).max() < 1e-12


def test_rms_tol_stops_early_and_zero_fills_the_trace(cube):
    R, t = rotation([1, 2, 3], 0.02), np.array([0.004, -0.003, 0.005])
    q = (cube.astype(F) @ R.T + t).astype(np.float32)
    full = AR.align(cube, q, 0.2, iterations=6)
    r = AR.align(cube, q, 0.2, iterations=6, rms_tol=1e-6)
    # the first step whose rms is within the tolerance of the step before makes no update
    rms = full["trace"]["rms"]
    k = next(k for k in range(1, 7) if abs(rms[k] - rms[k - 1]) <= 1e-6)
    assert 2 <= k <= 4 and abs(rms[1] - rms[0]) > 1e-6
    assert r["stats"]["stop_reason"] == AR.STOP_RMS and r["stats"]["iterations_run"] == k
    assert r["trace"][:k + 1].tolist() == full["trace"][:k + 1].tolist()
    assert r["trace"][k + 1:].tolist() == [(0, 0.0)] * (6 - k)
    # never at step 0, whatever the tolerance; 0 means never
    assert AR.align(cube, q, 0.2, iterations=2, rms_tol=1e9)["stats"]["iterations_run"] == 1
    assert full["stats"]["stop_reason"] == AR.STOP_ITERATIONS and (full["trace"]["matched"] == 300).all()


# ---- planted motions ---------------------------------------------------------------------------

def test_a_planted_rigid_motion_and_a_planted_similarity_are_recovered(cube):
    R, t = rotation([1, 2, 3], 0.005), np.array([0.001, -0.00075, 0.00125])
    for s in (1.0, 1.003):
        truth = np.hstack([s * R, t[:, None]])
        q = AR.transform_positions(cube, truth)  # rounded to fp32: about 6e-8 per coordinate
        # the motion is small enough that the first matches are the true ones
        assert (AR.nearest(cube, q, 0.2)["index"] == np.arange(300)).all()
        r = AR.align(cube, q, 0.2, iterations=5, scale=s != 1.0)
        err = np.abs(r["matrix"] - truth).max()
        # measured here: 2.2e-9 (rigid), 2.7e-9 (similarity; its scale 7.3e-10): the fp32 rounding of
        # 300 targets averaged out; the bounds are ten times that
        assert err <= 2.7e-8, err
        assert abs(r["scale"] - s) <= 7.3e-9 and r["stats"]["iterations_run"] == 5
        assert r["trace"]["rms"][0] > 2e-3 and (r["trace"]["rms"][1:] < 6e-8).all()
    # a rigid fit of the similarity's targets leaves the scale's residual
    r = AR.align(cube, q, 0.2, iterations=5)
    assert r["scale"] == 1.0 and r["trace"]["rms"][-1] > 5e-4


def test_the_jacobi_solve_agrees_with_numpy(cube):
    R, t = rotation([3, -1, 2], 0.3), np.array([0.1, 0.2, -0.3])
    q = AR.transform_positions(cube, np.hstack([R, t[:, None]]))
    y = cube  # matched by index: build S directly
    mux, muq = cube.astype(F).mean(axis=0), q.astype(F).mean(axis=0)
    dx, dq = cube.astype(F) - mux, q.astype(F) - muq
    S = [[F((dx[:, a] * dq[:, b]).sum()) for b in range(3)] for a in range(3)]
    N0 = np.array(AR.horn_matrix(S), F)
    Nd, V = AR.jacobi(AR.horn_matrix(S))
    w = np.linalg.eigvalsh(N0)
    assert np.allclose(sorted(float(Nd[k][k]) for k in range(4)), w, rtol=0, atol=1e-13 * abs(w).max())
    assert all(Nd[p][q] == 0.0 for p, q in AR.PAIRS)
    M, s = AR.solve(S, F((dx * dx).sum()), list(mux), list(muq), False)
    assert np.abs(M[:, :3] - R).max() < 1e-7 and np.abs(M[:, 3] - t).max() < 1e-7 and s == 1.0 and y is cube


def test_transform_reference():
    M = np.hstack([2.0 * rotation([0, 0, 1], np.pi / 2), [[1.0], [2.0], [3.0]]])
    rec = np.zeros(4, [("pos", "<f4", 3), ("normal", "<f4", 3), ("tag", "<i4")])
    rec["pos"] = [[1, 0, 0], [np.nan, 0, 0], [0, 1, 0], [0, 0, np.inf]]
    rec["normal"] = [[1, 0, 0], [0, 2, 0], [0, 0, 0], [np.nan, 0, 0]]
    rec["tag"] = [7, 8, 9, 10]
    out = AR.transform(rec, M, normals=True)
    assert np.allclose(out["pos"][0], [1, 4, 3]) and np.allclose(out["pos"][2], [-1, 2, 3])
    assert out["pos"][1].tobytes() == rec["pos"][1].tobytes() and out["pos"][3].tobytes() == rec["pos"][3].tobytes()
    assert np.allclose(out["normal"][0], [0, 1, 0], atol=1e-7) and np.allclose(out["normal"][1], [-1, 0, 0], atol=1e-7)
    assert out["normal"][2].tolist() == [0, 0, 0] and out["normal"][3].tobytes() == rec["normal"][3].tobytes()
    assert out["tag"].tolist() == [7, 8, 9, 10]
    assert np.array_equal(AR.transform(rec, M)["normal"], rec["normal"], equal_nan=True)
    assert AR.same_bits(AR.transform(rec["pos"], M), out["pos"])


# ---- the multi-channel tree ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_the_levels_of_256_are_the_pairwise_sum(n):
    rng = np.random.default_rng(n)
    terms = (rng.random((n, 11)) - 0.5) * 2.0 ** rng.integers(-20, 4, (n, 11)) + 0.0
    terms[rng.random(n) < 0.2] = 0.0  # the unmatched
    got = AR.tree_levels(terms)
    assert got == [KR.pairwise_sum(terms[:, ch]) for ch in range(11)] == AR.channel_sums(terms)
    assert AR.tree_levels(terms[:, :6]) == got[:6]


def test_a_negative_zero_term_is_why_the_terms_add_zero():
    # -0.0 alone survives pairwise_sum but not a level padded to 256; with + 0.0 the two agree
    assert np.signbit(KR.pairwise_sum([-0.0])) and not np.signbit(AR.tree_levels(np.array([-0.0]))[0])
    x = np.array([-0.0]) + 0.0
    assert not np.signbit(KR.pairwise_sum(x)) and not np.signbit(AR.tree_levels(x)[0])


# ---- the Python layer's checks -------------------------------------------------------------------

def test_check_cloud_align_args_refuses_every_listed_error():
    ok, init = pmvs.check_cloud_align_args(3, 4, 0.5, 10, True, np.eye(3, 4), 1e-6, 5, 16, 64)
    assert (ok.max_dist, ok.iterations, ok.min_pairs, ok.flags, ok.rms_tol) == (0.5, 10, 5, N.CLOUD_ALIGN_SCALE, 1e-6)
    assert init.dtype == np.float64 and init.shape == (3, 4) and init.flags.c_contiguous
    ok, init = pmvs.check_cloud_align_args(0, 0, 0.5)
    assert (ok.iterations, ok.min_pairs, ok.flags, ok.rms_tol, init) == (30, 3, 0, 0.0, None)
    nan_init = np.eye(3, 4)
    nan_init[1, 2] = np.nan
    bad = [
        dict(n_source=-1), dict(n_source=2**31), dict(n_target=-1), dict(n_target=True), dict(n_source=1.5),
        dict(source_stride=8), dict(source_stride=14), dict(target_stride=0), dict(target_stride=12.0),
        dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
        dict(max_dist=1e39), dict(max_dist=1e-50), dict(max_dist=None), dict(max_dist=True),
        dict(iterations=0), dict(iterations=1001), dict(iterations=-1), dict(iterations=3.0), dict(iterations=True),
        dict(min_pairs=2), dict(min_pairs=0), dict(min_pairs=3.0), dict(min_pairs=True), dict(min_pairs=2**31),
        dict(rms_tol=-1e-9), dict(rms_tol=float("inf")), dict(rms_tol=float("nan")), dict(rms_tol=None),
        dict(rms_tol=True),
        dict(scale=1), dict(scale=2), dict(scale=None),
        dict(init=nan_init), dict(init=np.full((3, 4), np.inf)), dict(init=np.eye(3)), dict(init=np.eye(4)),
        dict(init="identity"), dict(init=[1.0] * 11),
        dict(inputs=(100, 200), outputs=(200,)), dict(inputs=(100, 200), outputs=(300, 100)),
    ]
    for kw in bad:
        args = dict(dict(n_source=3, n_target=3, max_dist=0.5), **kw)
        with pytest.raises(ValueError):
            pmvs.check_cloud_align_args(**args)
    pmvs.check_cloud_align_args(2**31 - 1, 0, 1e-45, 1, init=list(range(12)))
    pmvs.check_cloud_align_args(0, 0, 3e38, 1000, True, None, 0.0, 2**31 - 1, 40, 16, inputs=(100, 0, None),
                                outputs=(300, 0, None))
    assert dp.check_cloud_align_args is pmvs.check_cloud_align_args


def test_check_cloud_transform_args_refuses_every_listed_error():
    m = pmvs.check_cloud_transform_args(5, list(range(12)), 40, 12)
    assert m.shape == (3, 4) and m.dtype == np.float64 and m[2, 3] == 11.0
    nan = np.eye(3, 4)
    nan[0, 0] = np.nan
    bad = [
        dict(n=-1), dict(n=2**31), dict(n=True), dict(stride=8), dict(stride=14), dict(stride=12.0),
        dict(matrix=None), dict(matrix=nan), dict(matrix=np.full((3, 4), -np.inf)), dict(matrix=np.eye(4)),
        dict(matrix=np.eye(3)), dict(matrix="m"),
        dict(normal_offset=0), dict(normal_offset=8), dict(normal_offset=14), dict(normal_offset=32),
        dict(normal_offset=-2), dict(normal_offset=12.0), dict(normal_offset=True),
        dict(stride=12, normal_offset=12), dict(stride=20, normal_offset=12),
    ]
    for kw in bad:
        args = dict(dict(n=5, matrix=np.eye(3, 4), stride=40), **kw)
        with pytest.raises(ValueError):
            pmvs.check_cloud_transform_args(**args)
    pmvs.check_cloud_transform_args(0, np.eye(3, 4))
    pmvs.check_cloud_transform_args(2**31 - 1, np.eye(3, 4), 40, 28)
    pmvs.check_cloud_transform_args(1, np.eye(3, 4), 24, 12)
    assert dp.check_cloud_transform_args is pmvs.check_cloud_transform_args
    with pytest.raises(ValueError):
        pmvs._cloud_normal_offset("t", np.zeros((3, 3), np.float32), True)  # no normal field
    with pytest.raises(ValueError):
        pmvs._cloud_normal_offset("t", np.zeros(3, N.FUSED_DTYPE), 1)
    assert pmvs._cloud_normal_offset("t", np.zeros(3, N.FUSED_DTYPE), True) == 12
    assert pmvs._cloud_normal_offset("t", np.zeros(3, N.FUSED_DTYPE), False) == -1


def test_binding_matches_the_header():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = f.read()
    for name, mirror, size in (("dp_cloud_align_options", N.DpCloudAlignOptions, 24),
                               ("dp_cloud_align_step", N.DpCloudAlignStep, 16),
                               ("dp_cloud_align_stats", N.DpCloudAlignStats, 96)):
        fields = header_struct(text, name)
        assert fields == list(mirror._fields_), name
        assert ctypes.sizeof(mirror) == size == sum(ctypes.sizeof(t) for _, t in fields), name
    names = [n for n, _ in N.DpCloudAlignStats._fields_]
    assert names[:6] + names[8:10] == list(AR.COUNTS)
    assert N.CLOUD_ALIGN_STEP_DTYPE == AR.STEP_DTYPE and N.CLOUD_ALIGN_STEP_DTYPE.itemsize == 16
    assert re.search(r"#define DP_CLOUD_ALIGN_SCALE %d\b" % N.CLOUD_ALIGN_SCALE, text)
    for name, value in (("ITERATIONS", AR.STOP_ITERATIONS), ("RMS", AR.STOP_RMS), ("PAIRS", AR.STOP_PAIRS),
                        ("DEGENERATE", AR.STOP_DEGENERATE), ("EMPTY", AR.STOP_EMPTY)):
        assert re.search(r"#define DP_CLOUD_ALIGN_STOP_%s %d\b" % (name, value), text)
        assert getattr(N, "CLOUD_ALIGN_STOP_" + name) == value
    assert AR.SWEEPS >= 6 and ("DP_CLOUD_ALIGN_SWEEPS is %d." % AR.SWEEPS) in text  # stated with its reasoning
    assert re.search(r"#define DP_ABI_VERSION 2\b", text)  # additions only: the version stays
    sigs = dict((s[0], s) for s in N.SIGNATURES)
    for name in ("dp_cloud_transform", "dp_cloud_transform_device", "dp_cloud_align", "dp_cloud_align_device"):
        args = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")
        assert len(args) == len(sigs[name][2]), name
        for a, t in zip(args, sigs[name][2]):
            assert ("*" in a) == (t is ctypes.c_void_p) and ("int64_t" in a and "*" not in a) == (t is ctypes.c_int64)
        assert hasattr(N.lib, name)


def test_the_sweeps_leave_no_off_diagonal_mass(cube):
    # the count in the header: after six sweeps every N_pq of the reference is exactly zero on these
    # inputs (so the remaining sweeps skip every rotation), and after four it is below 2^-50 of the top
    R, t = rotation([1, 2, 3], 0.02), np.array([0.004, -0.003, 0.005])
    plane, line = cube.copy(), np.zeros((100, 3), np.float32)
    plane[:, 2] = 0.5
    line[:, 0] = np.linspace(0, 1, 100)
    line[:, 1] = line[:, 0] * np.float32(0.3)
    mirrored = cube.copy()
    mirrored[:, 0] = np.float32(1) - mirrored[:, 0]
    doubled = np.concatenate([cube[:100], cube[:100]])
    move = np.hstack([R, t[:, None]])
    for a, b in ((cube, AR.transform_positions(cube, move)), (plane, AR.transform_positions(plane, move)),
                 (line, AR.transform_positions(line, move)), (cube, mirrored), (cube, cube),
                 (doubled, AR.transform_positions(doubled, move))):
        _, _, _, _, S, _, _ = AR.one_pass(a, b, AR.IDENTITY, 0.3)
        for sweeps, bound in ((4, 2.0 ** -50), (6, 0.0)):
            Nd, _ = AR.jacobi(AR.horn_matrix(S), sweeps)
            off = np.sqrt(sum(float(Nd[p][q]) ** 2 for p, q in AR.PAIRS))
            assert off <= bound * max(abs(float(Nd[k][k])) for k in range(4)), (sweeps, off)


def test_a_null_context_is_an_argument_error():
    # the one error return that needs no device (a context cannot be made without one)
    ao = N.DpCloudAlignOptions(1.0, 1, 3, 0, 0.0)
    M, s, trace = (ctypes.c_double * 12)(), ctypes.c_double(), (N.DpCloudAlignStep * 2)()
    out = ctypes.c_void_p()
    assert N.lib.dp_cloud_align(None, None, 0, 12, None, 0, 12, ctypes.byref(ao), None, M, ctypes.byref(s), trace, None,
                                None, None) == N.DP_E_ARG
    assert N.lib.dp_cloud_align_device(None, None, 0, 12, None, 0, 12, ctypes.byref(ao), None, M, ctypes.byref(s), trace,
                                       None, None, None, None) == N.DP_E_ARG
    assert N.lib.dp_cloud_transform(None, None, 0, 12, M, -1, ctypes.byref(out)) == N.DP_E_ARG
    assert N.lib.dp_cloud_transform_device(None, None, 0, 12, M, -1, None, None) == N.DP_E_ARG


def test_compare_refuses_a_bad_align_dict_before_any_device_call():
    pts = np.zeros((4, 3), np.float32)
    bad = ("yes", 3, [], dict(radius=1.0), dict(iterations=0), dict(iterations=1001), dict(max_dist=0.0),
           dict(scale=1), dict(init=np.eye(3)), dict(rms_tol=-1.0), dict(min_pairs=2), dict(correspondences=True))
    for align in bad:
        with pytest.raises(ValueError):
            dp.cloud_compare(None, pts, pts, 0.1, align=align)  # no engine is ever touched
        with pytest.raises(ValueError):
            dp.mesh_compare(None, pts, np.zeros((0, 3), np.int32), pts, 0.1, align=align)
        with pytest.raises(ValueError):
            dp.PMVS().evaluate(pts, 0.1, cloud=pts, align=align)
    kw = pmvs.check_compare_align(dict(iterations=5), 0.25)
    assert kw == dict(iterations=5, max_dist=0.25) and pmvs.check_compare_align(None, 0.25) is None
    assert pmvs.check_compare_align(dict(max_dist=0.5, scale=True), 0.25) == dict(max_dist=0.5, scale=True)
