"""dp_cloud_knn and dp_cloud_clean without a GPU: the reference
(tests/cloudknn_ref.py) on hand-worked cases, the pairwise sum against an exact
sum and against a sequential one, the Python layer's argument checks against the
header's error lists, the ctypes mirrors against the header, and the error
returns that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudknn_ref as KR
import cloudnearest_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def test_three_points_on_a_line():
    p = f32([[0, 0, 0], [1, 0, 0], [3, 0, 0]])
    r = KR.knn(p, p, 2, 2.0)
    assert r["index"].tolist() == [[0, 1], [1, 0], [2, 1]]
    assert r["dist"].tolist() == [[0.0, 1.0], [0.0, 1.0], [0.0, 2.0]]  # 2 is on the radius: inclusive
    assert r["count"].tolist() == [2, 2, 2]
    assert r["stats"] == dict(queries=3, targets=3, skipped_queries=0, skipped_targets=0, full=3, partial=0, empty=0,
                              neighbours=6)
    r = KR.knn(p, p, 2, 2.0, exclude_self=True)
    assert r["index"].tolist() == [[1, -1], [0, 2], [1, -1]]
    assert r["dist"][0].tolist() == [1.0, np.inf] and r["dist"][1].tolist() == [1.0, 2.0]
    assert r["count"].tolist() == [1, 2, 1]
    assert (r["stats"]["full"], r["stats"]["partial"], r["stats"]["empty"], r["stats"]["neighbours"]) == (1, 2, 0, 4)
    r = KR.knn(p, p, 3, 0.5, exclude_self=True)
    assert (r["index"] == -1).all() and (r["dist"] == INF).all() and r["stats"]["empty"] == 3


def test_a_tie_across_the_kth_place_goes_to_the_lower_indices():
    # four targets at distance 1 and one at 0.5: k = 3 takes 0.5 and the two lowest indices of the tie
    t = f32([[0, 1, 0], [1, 0, 0], [0, 0, 0.5], [-1, 0, 0], [0, -1, 0]])
    r = KR.knn(f32([[0, 0, 0]]), t, 3, 4.0)
    assert r["index"].tolist() == [[2, 0, 1]] and r["dist"].tolist() == [[0.5, 1.0, 1.0]]
    r = KR.knn(f32([[0, 0, 0]]), t[::-1], 3, 4.0)
    assert r["index"].tolist() == [[2, 0, 1]]  # the reversed array: 0.5 is again 2, the tie 0 and 1
    # a duplicate of the query under another index stays a neighbour at distance 0
    p = f32([[1, 1, 1], [2, 2, 2], [1, 1, 1]])
    r = KR.knn(p, p, 1, 1.0, exclude_self=True)
    assert r["index"].tolist() == [[2], [-1], [0]] and r["dist"][:, 0].tolist() == [0.0, np.inf, 0.0]


def test_points_that_are_not_finite_take_no_part():
    q = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    t = f32([[np.nan, 0, 0], [0, 0, 1], [np.inf, 0, 0], [0, 0, 0.5]])
    r = KR.knn(q, t, 2, 2.0)
    assert r["index"].tolist() == [[3, 1], [-1, -1], [-1, -1]] and r["count"].tolist() == [2, 0, 0]
    assert r["stats"] == dict(queries=1, targets=2, skipped_queries=2, skipped_targets=2, full=1, partial=0, empty=0,
                              neighbours=2)
    r = KR.knn(f32([]), t, 2, 2.0)
    assert r["index"].shape == (0, 2) and r["stats"]["queries"] == 0 and r["stats"]["targets"] == 2
    r = KR.knn(q, f32([]), 2, 2.0)
    assert (r["index"] == -1).all() and r["stats"]["empty"] == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_k_one_is_cloud_nearest(seed):
    rng = np.random.default_rng(seed)
    q, t = rng.random((300, 3), np.float32), rng.random((200, 3), np.float32)
    t[50:60] = t[40:50]  # duplicates: ties
    q[7, 1] = np.nan
    t[3, 0] = np.inf
    a, b = KR.knn(q, t, 1, 0.1), CR.nearest(q, t, 0.1)
    assert CR.same_bits(a["index"][:, 0], b["index"]) and CR.same_bits(a["dist"][:, 0], b["dist"])
    assert a["stats"]["full"] == b["stats"]["matched"] and a["stats"]["empty"] == b["stats"]["unmatched"]
    assert a["stats"]["partial"] == 0 and a["stats"]["neighbours"] == b["stats"]["matched"]


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4097])
def test_pairwise_sum_is_close_to_the_exact_sum(n):
    rng = np.random.default_rng(n)
    x = rng.random(n) * 2.0 ** rng.integers(-20, 4, n)
    exact = math.fsum(x)
    # a balanced tree of depth ceil(log2 n) over non-negative terms: (1 + 2^-53)^depth - 1, and fsum's own rounding
    depth = max(1, math.ceil(math.log2(n))) if n > 1 else 0
    assert abs(KR.pairwise_sum(x) - exact) <= (depth + 1) * 2.0 ** -53 * exact * (1 + 2.0 ** -40)
    assert KR.pairwise_sum([]) == 0.0 and KR.pairwise_sum([3.5]) == 3.5


def test_pairwise_and_sequential_sums_differ_in_bits():
    # 1, then three times 2^-53: in sequence every add rounds back to 1; in pairs
    # (1 + 2^-53) + (2^-53 + 2^-53) = 1 + 2^-52
    x = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53])
    seq = 0.0
    for v in x:
        seq = seq + float(v)
    assert seq == 1.0 and KR.pairwise_sum(x) == 1.0 + 2.0 ** -52
    assert KR.pairwise_sum(x) != seq
    # and on distances spanning several binades, as the GPU tests use
    rng = np.random.default_rng(5)
    y = rng.random(4097) * 2.0 ** rng.integers(-12, 1, 4097)
    seq = 0.0
    for v in y:
        seq = seq + float(v)
    assert KR.pairwise_sum(y) != seq


def test_clean_reference_on_a_planted_line():
    # five points one apart, a far pair 0.9 apart, one isolated point
    p = f32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [10, 0, 0], [10, 0.9, 0], [20, 0, 0],
             [np.nan, 0, 0]])
    r = KR.clean(p, 2, 1.0, std_mul=0.0, radius_only=True)
    assert r["keep"].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0] and r["map"].tolist() == [0, 1, 2, 3, 4, 5, 6, -1, -1]
    assert r["stats"] == dict(points=8, skipped=1, eligible=7, kept=7, removed_sparse=1, removed_far=0)
    assert (r["mu"], r["sigma"], r["threshold"]) == (0.0, 0.0, 0.0)
    assert r["mean_dist"][:5].tolist() == [1.0] * 5 and r["mean_dist"][5] == np.float32(np.float64(np.float32(0.9)))
    assert r["mean_dist"][7] == INF and r["mean_dist"][8] == INF
    r = KR.clean(p, 2, 1.0, std_mul=2.0, min_neighbours=2)
    # only the three inner points have two neighbours; their means are all 1: sigma = 0, T = 1
    assert r["keep"].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert r["stats"] == dict(points=8, skipped=1, eligible=3, kept=3, removed_sparse=5, removed_far=0)
    assert (r["mu"], r["sigma"], r["threshold"]) == (1.0, 0.0, 1.0)
    assert len(r["points"]) == 3 and r["points"].tolist() == p[1:4].tolist()


def test_check_cloud_knn_args_refuses_every_listed_error():
    ok = pmvs.check_cloud_knn_args(3, 3, 8, 0.5, True, 16, 64)
    assert (ok.max_dist, ok.k, ok.flags) == (0.5, 8, N.CLOUD_KNN_EXCLUDE_SELF)
    assert pmvs.check_cloud_knn_args(3, 4, 32, 0.5).flags == 0
    bad = [
        dict(n_queries=-1), dict(n_queries=2**31), dict(n_targets=-1), dict(n_targets=True), dict(n_queries=1.5),
        dict(query_stride=8), dict(query_stride=14), dict(target_stride=0), dict(target_stride=12.0),
        dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
        dict(max_dist=1e39), dict(max_dist=1e-50), dict(max_dist=None), dict(max_dist=True),
        dict(k=0), dict(k=33), dict(k=-1), dict(k=8.0), dict(k=None), dict(k=True),
        dict(exclude_self=1), dict(exclude_self=True, n_targets=4),
        dict(inputs=(100, 200), outputs=(200,)), dict(inputs=(100, 200), outputs=(300, 400, 100)),
    ]
    for kw in bad:
        args = dict(dict(n_queries=3, n_targets=3, k=8, max_dist=0.5), **kw)
        with pytest.raises(ValueError):
            pmvs.check_cloud_knn_args(**args)
    pmvs.check_cloud_knn_args(2**31 - 1, 0, 1, 1e-45)
    pmvs.check_cloud_knn_args(0, 0, 32, 3e38, True, 40, 16, inputs=(100, 0, None), outputs=(300, 0, None))
    assert dp.check_cloud_knn_args is pmvs.check_cloud_knn_args


def test_check_cloud_clean_args_refuses_every_listed_error():
    ok = pmvs.check_cloud_clean_args(5, 8, 0.5, 1.5, 3, True, 40)
    assert (ok.max_dist, ok.k, ok.min_neighbours, ok.std_mul, ok.flags) == (0.5, 8, 3, 1.5, N.CLOUD_CLEAN_RADIUS_ONLY)
    ok = pmvs.check_cloud_clean_args(5, 8, 0.5)
    assert (ok.min_neighbours, ok.std_mul, ok.flags) == (1, 2.0, 0)
    bad = [
        dict(n=-1), dict(n=2**31), dict(n=True), dict(stride=8), dict(stride=14), dict(stride=12.0),
        dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=1e39), dict(max_dist=None),
        dict(k=0), dict(k=33), dict(k=8.0),
        dict(min_neighbours=0), dict(min_neighbours=9), dict(min_neighbours=1.0), dict(min_neighbours=True),
        dict(std_mul=-0.5), dict(std_mul=float("inf")), dict(std_mul=float("nan")), dict(std_mul=1e39),
        dict(std_mul=None), dict(std_mul=True),
        dict(radius_only=1),
        dict(inputs=(100,), outputs=(200, 100)), dict(inputs=(100,), outputs=(200, 300, 200)),
    ]
    for kw in bad:
        args = dict(dict(n=5, k=8, max_dist=0.5), **kw)
        with pytest.raises(ValueError):
            pmvs.check_cloud_clean_args(**args)
    pmvs.check_cloud_clean_args(0, 1, 1e-45, 0.0, 1)
    pmvs.check_cloud_clean_args(2**31 - 1, 32, 3e38, 3e38, 32, inputs=(100,), outputs=(200, None, 0, 300))
    assert dp.check_cloud_clean_args is pmvs.check_cloud_clean_args


def header_struct(text, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    fields = []
    for typ, names in re.findall(r"(float|int32_t|int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    return fields


def test_binding_matches_the_header():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = f.read()
    for name, mirror, size in (("dp_cloud_knn_options", N.DpCloudKnnOptions, 12),
                               ("dp_cloud_knn_stats", N.DpCloudKnnStats, 96),
                               ("dp_cloud_clean_options", N.DpCloudCleanOptions, 20),
                               ("dp_cloud_clean_stats", N.DpCloudCleanStats, 104)):
        fields = header_struct(text, name)
        assert fields == list(mirror._fields_), name
        assert ctypes.sizeof(mirror) == size == sum(ctypes.sizeof(t) for _, t in fields), name
    assert [n for n, _ in N.DpCloudKnnStats._fields_][:8] == list(KR.KNN_COUNTS)
    assert [n for n, _ in N.DpCloudCleanStats._fields_][:6] == list(KR.CLEAN_COUNTS)
    assert re.search(r"#define DP_CLOUD_KNN_EXCLUDE_SELF %d\b" % N.CLOUD_KNN_EXCLUDE_SELF, text)
    assert re.search(r"#define DP_CLOUD_CLEAN_RADIUS_ONLY %d\b" % N.CLOUD_CLEAN_RADIUS_ONLY, text)
    assert re.search(r"#define DP_ABI_VERSION 2\b", text)  # additions only: the version stays
    sigs = dict((s[0], s) for s in N.SIGNATURES)
    for name in ("dp_cloud_knn", "dp_cloud_knn_device", "dp_cloud_clean", "dp_cloud_clean_device"):
        args = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")
        assert len(args) == len(sigs[name][2]), name
        for a, t in zip(args, sigs[name][2]):
            assert ("*" in a) == (t is ctypes.c_void_p) and ("int64_t" in a and "*" not in a) == (t is ctypes.c_int64)
        assert hasattr(N.lib, name)


def test_a_null_context_is_an_argument_error():
    # the one error return that needs no device (a context cannot be made without one)
    ko, co = N.DpCloudKnnOptions(1.0, 1, 0), N.DpCloudCleanOptions(1.0, 1, 1, 2.0, 0)
    p = ctypes.c_void_p()
    assert N.lib.dp_cloud_knn(None, None, 0, 12, None, 0, 12, ctypes.byref(ko), ctypes.byref(p), ctypes.byref(p),
                              ctypes.byref(p), None) == N.DP_E_ARG
    assert N.lib.dp_cloud_knn_device(None, None, 0, 12, None, 0, 12, ctypes.byref(ko), None, None, None, None,
                                     None) == N.DP_E_ARG
    assert N.lib.dp_cloud_clean(None, None, 0, 12, ctypes.byref(co), ctypes.byref(p), None, None, None, None,
                                None) == N.DP_E_ARG
    assert N.lib.dp_cloud_clean_device(None, None, 0, 12, ctypes.byref(co), None, None, None, None, None, None,
                                       None) == N.DP_E_ARG


def test_fused_cloud_refuses_a_bad_clean_dict_before_any_device_call():
    p = dp.PMVS()
    with pytest.raises(ValueError):
        p.fused_cloud(clean=dict(max_dist=0.1))  # nothing has run
    p._ran = True
    for clean in (dict(k=8), dict(), "yes", 8, dict(max_dist=0.1, radius=2), dict(max_dist=0.0), dict(max_dist=0.1, k=33),
                  dict(max_dist=0.1, k=4, min_neighbours=5), dict(max_dist=0.1, std_mul=-1.0),
                  dict(max_dist=0.1, radius_only="no")):
        with pytest.raises(ValueError):
            p.fused_cloud(clean=clean)
