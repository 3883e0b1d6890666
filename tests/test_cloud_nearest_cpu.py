"""dp_cloud_nearest without a GPU: the reference (tests/cloudnearest_ref.py) on
hand-computed cases, the Python layer's argument checks against the header's
error list, the ctypes mirrors against the header, and cloud_compare's ratios
and F-score on a planted pair of clouds."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudnearest_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def test_three_four_five():
    r = CR.nearest(f32([[0, 0, 0]]), f32([[3, 4, 0], [0, 0, 6]]), 5.0)
    assert r["index"].tolist() == [0] and r["dist"].tolist() == [5.0]
    assert r["stats"] == dict(queries=1, targets=2, skipped_queries=0, skipped_targets=0, matched=1, unmatched=0)
    # the radius is inclusive: 5 matches at max_dist 5 and not one f32 below it
    below = np.nextafter(np.float32(5), np.float32(0))
    r = CR.nearest(f32([[0, 0, 0]]), f32([[3, 4, 0]]), below)
    assert r["index"].tolist() == [-1] and r["dist"][0] == INF and r["stats"]["unmatched"] == 1


def test_tie_at_a_midpoint_and_a_duplicate_go_to_the_lowest_index():
    t = f32([[2, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0]])
    r = CR.nearest(f32([[1, 0, 0], [0, 0, 0], [1.75, 0, 0]]), t, 4.0)
    assert r["index"].tolist() == [0, 1, 0] and r["dist"].tolist() == [1.0, 0.0, 0.25]
    # the same targets in another order: the lowest index again
    r = CR.nearest(f32([[1, 0, 0]]), t[::-1], 4.0)
    assert r["index"].tolist() == [0]


def test_points_that_are_not_finite_take_no_part():
    q = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0]])
    t = f32([[np.nan, 0, 0], [0, 0, 1], [np.inf, 0, 0], [0, 0, 0.5]])
    r = CR.nearest(q, t, 2.0, hist_bins=4)
    assert r["index"].tolist() == [3, -1, -1, -1, -1]
    assert r["dist"][0] == np.float32(0.5) and (r["dist"][1:] == INF).all()
    assert r["stats"] == dict(queries=2, targets=2, skipped_queries=3, skipped_targets=2, matched=1, unmatched=1)
    assert r["hist"].tolist() == [0, 1, 0, 0] and r["hist"].dtype == np.uint64


def test_empty_sets():
    r = CR.nearest(f32([]), f32([[0, 0, 0]]), 1.0, hist_bins=2)
    assert len(r["index"]) == 0 and len(r["dist"]) == 0 and r["hist"].tolist() == [0, 0]
    assert r["stats"] == dict(queries=0, targets=1, skipped_queries=0, skipped_targets=0, matched=0, unmatched=0)
    r = CR.nearest(f32([[0, 0, 0], [1, 1, 1]]), f32([]), 1.0)
    assert r["index"].tolist() == [-1, -1] and (r["dist"] == INF).all() and r["hist"] is None
    assert r["stats"] == dict(queries=2, targets=0, skipped_queries=0, skipped_targets=0, matched=0, unmatched=2)
    r = CR.nearest(f32([[0, 0, 0]]), f32([[np.nan, 0, 0]]), 1.0)
    assert r["index"].tolist() == [-1] and r["stats"]["targets"] == 0 and r["stats"]["skipped_targets"] == 1


def test_histogram_edge_bins():
    # distances 0, 0.25, 0.5 - ulp, 0.5, 0.999.., 1.0 at max_dist 1 with 4 bins
    d = [0.0, 0.25, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.5,
         float(np.nextafter(np.float32(1), np.float32(0))), 1.0, 1.5]
    q = f32([[x, 0, 0] for x in d])
    r = CR.nearest(q, f32([[0, 0, 0]]), 1.0, hist_bins=4)
    assert r["index"].tolist() == [0] * 6 + [-1]
    # dist == max_dist computes bin 4 and is clamped into the last one
    assert r["hist"].tolist() == [1, 2, 1, 2] and int(r["hist"].sum()) == r["stats"]["matched"] == 6
    assert CR.nearest(q, f32([[0, 0, 0]]), 1.0, hist_bins=1)["hist"].tolist() == [6]


def test_max_dist_is_the_float32_the_struct_holds():
    # 0.1 as f32 is a little above 0.1: a target at f32(0.1) is on the radius
    t = f32([[np.float32(0.1), 0, 0]])
    assert CR.nearest(f32([[0, 0, 0]]), t, 0.1)["index"].tolist() == [0]


def test_check_cloud_nearest_args_refuses_every_listed_error():
    ok = pmvs.check_cloud_nearest_args(3, 4, 0.5, 32, 16, 64)
    assert (ok.max_dist, ok.hist_bins, ok.flags) == (0.5, 32, 0)
    bad = [
        dict(n_queries=-1), dict(n_queries=2**31), dict(n_targets=-1), dict(n_targets=2**31), dict(n_queries=1.5),
        dict(n_targets=True),
        dict(query_stride=8), dict(query_stride=10), dict(query_stride=14), dict(target_stride=8),
        dict(target_stride=10), dict(target_stride=0), dict(target_stride=-12), dict(query_stride=12.0),
        dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
        dict(max_dist=1e39), dict(max_dist=1e-50), dict(max_dist=None), dict(max_dist="1"), dict(max_dist=True),
        dict(hist_bins=-1), dict(hist_bins=65537), dict(hist_bins=1.0), dict(hist_bins=None),
        dict(flags=1), dict(flags=-1),
        dict(inputs=(100, 200), outputs=(200,)), dict(inputs=(100, 200), outputs=(300, 400, 100)),
    ]
    for kw in bad:
        args = dict(dict(n_queries=3, n_targets=4, max_dist=0.5), **kw)
        with pytest.raises(ValueError):
            pmvs.check_cloud_nearest_args(**args)
    # legal neighbours of the refused values
    pmvs.check_cloud_nearest_args(2**31 - 1, 0, 1e-45, 65536, 12, 80)
    pmvs.check_cloud_nearest_args(0, 2**31 - 1, 3e38, 0, 40, 16, inputs=(100, 0, None), outputs=(300, 0, None))


def test_cloud_points_keep_a_structured_arrays_stride():
    for dtype, stride, off in ((N.MESH_VERTEX_DTYPE, 16, 0), (N.FUSED_DTYPE, 40, 0), (N.PATCH_DTYPE, 80, None)):
        a = np.zeros(5, dtype)
        arr, addr, n, s = pmvs._cloud_points("t", a)
        assert (n, s) == (5, stride) and addr == arr.ctypes.data + dtype.fields["pos"][1]
        assert off is None or dtype.fields["pos"][1] == off
    arr, addr, n, s = pmvs._cloud_points("t", np.zeros((7, 3), np.float64))
    assert (n, s) == (7, 12) and arr.dtype == np.float32 and addr == arr.ctypes.data
    for wrong in (np.zeros((4, 2), np.float32), np.zeros(6, np.float32), np.zeros(3, [("xyz", "<f4", 3)]),
                  np.zeros(3, [("pos", "<f8", 3)])):
        with pytest.raises(ValueError):
            pmvs._cloud_points("t", wrong)


def test_binding_matches_the_header():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = f.read()
    m = re.search(r"typedef struct dp_cloud_nearest_options \{(.*?)\} dp_cloud_nearest_options;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = re.findall(r"(float|int32_t)\s+(\w+);", body)
    assert [n for _, n in decl] == [n for n, _ in N.DpCloudNearestOptions._fields_]
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [ctype[t] for t, _ in decl] == [t for _, t in N.DpCloudNearestOptions._fields_]
    assert ctypes.sizeof(N.DpCloudNearestOptions) == 12
    assert [getattr(N.DpCloudNearestOptions, n).offset for n, _ in N.DpCloudNearestOptions._fields_] == [0, 4, 8]
    m = re.search(r"typedef struct dp_cloud_nearest_stats \{(.*?)\} dp_cloud_nearest_stats;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_int64 if typ == "int64_t" else ctypes.c_double) for n in names.split(",")]
    assert fields == list(N.DpCloudNearestStats._fields_)
    assert [n for n, _ in fields] == list(CR.COUNTS) + ["grid_cells", "max_cell_targets", "build_ms", "query_ms"]
    assert ctypes.sizeof(N.DpCloudNearestStats) == 8 * len(fields) == 80
    assert [getattr(N.DpCloudNearestStats, n).offset for n, _ in fields] == [8 * k for k in range(len(fields))]
    sigs = dict((s[0], s) for s in N.SIGNATURES)
    for name in ("dp_cloud_nearest", "dp_cloud_nearest_device"):
        args = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")
        assert len(args) == len(sigs[name][2])
        for a, t in zip(args, sigs[name][2]):
            assert ("*" in a) == (t is ctypes.c_void_p) and ("int64_t" in a and "*" not in a) == (t is ctypes.c_int64)
    assert hasattr(N.lib, "dp_cloud_nearest") and hasattr(N.lib, "dp_cloud_nearest_device")


class RefEngine:
    """cloud_compare's engine, with the reference as its cloud_nearest"""
    def cloud_nearest(self, queries, targets, max_dist, hist_bins=0):
        return CR.nearest(queries, targets, max_dist, hist_bins)


def test_cloud_compare_on_planted_clouds():
    # truth: 10 points on the x axis, one apart.  recon: 4 points exactly on the
    # truth, 2 at 0.25 from it, 1 at 0.75, 1 at 3 (beyond max_dist 2), 1 NaN.
    truth = f32([[x, 0, 0] for x in range(10)])
    recon = f32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0.25, 0], [5, 0, 0.25], [6, 0.75, 0], [7, 3, 0],
                 [np.nan, 0, 0]])
    got = pmvs.cloud_compare(RefEngine(), recon, truth, 0.5, max_dist=2.0)
    acc, com = got["accuracy"], got["completeness"]
    assert (acc["n"], acc["matched"], acc["within_tau"]) == (8, 7, 6) and acc["ratio"] == 6 / 8
    assert acc["mean"] == pytest.approx((0.25 + 0.25 + 0.75) / 7) and acc["median"] == 0.0
    assert acc["p90"] == pytest.approx(0.25 + 0.5 * 0.4)  # pos 5.4 between 0.25 and 0.75
    # truth -> recon: 0..5 within tau, 6 at 0.75; 7 has (6, 0.75, 0) at sqrt(1.5625) = 1.25; 8 has it at
    # sqrt(4.5625) > 2 and (7, 3, 0) at sqrt(10): unmatched, as is 9
    assert (com["n"], com["matched"], com["within_tau"]) == (10, 8, 6) and com["ratio"] == 0.6
    assert com["median"] == pytest.approx(0.125) and com["mean"] == pytest.approx((0.5 + 0.75 + 1.25) / 8)
    p, r = 0.75, 0.6
    assert got["fscore"] == pytest.approx(2 * p * r / (p + r))
    CR.assert_compare(got, CR.compare(recon, truth, 0.5, 2.0))
    # the default radius is 10 tau: everything finite matches
    wide = pmvs.cloud_compare(RefEngine(), recon, truth, 0.5)
    assert wide["accuracy"]["matched"] == 8 and wide["completeness"]["matched"] == 10
    assert wide["accuracy"]["within_tau"] == 6
    # structured clouds are read through pos
    v = np.zeros(len(recon), N.MESH_VERTEX_DTYPE)
    v["pos"] = recon
    CR.assert_compare(pmvs.cloud_compare(RefEngine(), v, truth, 0.5, 2.0), got)


def test_cloud_compare_degenerate_sides():
    empty = f32([])
    got = pmvs.cloud_compare(RefEngine(), empty, f32([[0, 0, 0]]), 0.5)
    for s in (got["accuracy"], got["completeness"]):
        assert s["ratio"] == 0.0 and s["matched"] == 0 and all(math.isnan(s[k]) for k in ("mean", "median", "p90"))
    assert got["accuracy"]["n"] == 0 and got["completeness"]["n"] == 1 and got["fscore"] == 0.0
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=None),
               dict(tau=1.0, max_dist=0.5), dict(tau=1.0, max_dist=float("inf")), dict(tau=1.0, max_dist="2")):
        with pytest.raises(ValueError):
            pmvs.cloud_compare(RefEngine(), empty, empty, **kw)
