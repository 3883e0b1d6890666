"""The densify CLI's report writer (programs/densify/report_json.h) and its
evaluation statistics (eval_stats.h/.cpp) without a GPU:
tests/cli_report_check.cpp, a stand-alone program over those files alone (no HIP
include path, no library: that it builds is the check that they are free of the
GPU), built with the host compiler under ASan + UBSan.  It answers the cases
written here, one JSON object each; the statistics are compared with
cloud_quantile, cloud_side and cloud_normal_error of densepoints_amd.pmvs on the
same arrays.

Tolerances: counts, ratio, median, p90 and max are exact (both sides do the same
IEEE operations on the same fp64 values); a mean is within 1e-14 relative (at
most 16 terms summed in another order: 16 x 2^-53); angles are within 1e-9
degrees (two acos implementations, the bound of
tests/test_gpu_cloud_normals_cli.py::close)."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from densepoints_amd import pmvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "programs", "densify")
NAN = float("nan")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("cli_report") / "cli_report_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CLI, os.path.join(ROOT, "tests", "cli_report_check.cpp"),
                    os.path.join(CLI, "eval_stats.cpp"), "-o", out], check=True)
    return out


def answers(exe, tmp_path, cases):
    """the program's answer to each case (a list of words), and the text of each"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(w) for w in case) + "\n" for case in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases), r.stdout
    return [json.loads(ln) for ln in lines], lines


def f32(x):
    return "%.9g" % np.float32(x)  # reads back to the same float


def f64(x):
    return "%.17g" % x


def search_words(index, dist):
    return [len(index)] + [w for i, d in zip(index, dist) for w in (int(i), f32(d))]


def same(got, want):
    """null for NaN, else the same double"""
    return got is None if math.isnan(want) else got == want


def mean_close(got, want):
    return got is None if math.isnan(want) else abs(got - want) <= 1e-14 * abs(want)


# ---- the distances of a search --------------------------------------------------------------------

TAU = 0.25
SEARCHES = {
    "none": ([], []),
    "none_matched": ([-1, -1, -1], [np.inf, np.inf, np.inf]),
    "one": ([4], [0.125]),
    "two": ([0, 7], [0.3, 0.1]),
    # ties, three without a match, three exactly at tau (0.25 is a float), one just above it
    "ten": ([3, -1, 0, 0, 9, -1, 2, 5, -1, 1],
            [0.25, np.inf, 0.1, 0.1, 0.25, np.inf, np.nextafter(np.float32(0.25), np.float32(1)), 0.7, np.inf, 0.25]),
}


def nearest(index, dist):
    index, dist = np.asarray(index, np.int32), np.asarray(dist, np.float32)
    return {"index": index, "dist": dist,
            "stats": {"queries": len(index), "matched": int(np.count_nonzero(index >= 0))}}


@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_side_entry_is_cloud_side(exe, tmp_path, name):
    near = nearest(*SEARCHES[name])
    n, matched = near["stats"]["queries"], near["stats"]["matched"]
    (got,), _ = answers(exe, tmp_path, [["side", f64(TAU), n, matched] + search_words(near["index"], near["dist"])])
    want = pmvs.cloud_side(near, TAU)
    e = got["entry"]
    assert list(e) == ["n", "matched", "within_tau", "ratio", "mean", "median", "p90"]
    assert (e["n"], e["matched"], e["within_tau"]) == (want["n"], want["matched"], want["within_tau"])
    assert e["ratio"] == want["ratio"] == got["ratio"]
    assert mean_close(e["mean"], want["mean"]) and same(e["median"], want["median"]) and same(e["p90"], want["p90"])
    if matched == 0:  # nothing to divide by, nothing to report
        assert e["ratio"] == 0 and e["mean"] is None and e["median"] is None and e["p90"] is None
    if name == "two":  # p90 lies between the only two ranks
        lo, hi = np.float64(np.float32(0.1)), np.float64(np.float32(0.3))
        assert e["p90"] == lo + (hi - lo) * 0.9 and e["median"] == lo + (hi - lo) * 0.5
    if name == "ten":  # <= tau: the three at tau count, the one above does not
        assert (e["matched"], e["within_tau"]) == (7, 5)


@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_deviation_entry(exe, tmp_path, name):
    near = nearest(*SEARCHES[name])
    n, matched = near["stats"]["queries"], near["stats"]["matched"]
    (got,), _ = answers(exe, tmp_path, [["deviation", n, matched] + search_words(near["index"], near["dist"])])
    want = pmvs.cloud_side(near, TAU)
    d = near["dist"][near["index"] >= 0].astype(np.float64)
    top = float(d.max()) if len(d) else NAN
    e = got["entry"]
    assert list(e) == ["n", "matched", "mean", "median", "p90", "max"]
    assert (e["n"], e["matched"]) == (n, matched)
    assert mean_close(e["mean"], want["mean"]) and same(e["median"], want["median"]) and same(e["p90"], want["p90"])
    assert same(e["max"], top) and same(got["top"], top)


def test_quantile_fscore_and_larger(exe, tmp_path):
    d = np.sort(np.float64([0.5, 0.1, 0.1, 2.0, 0.7]))
    cases, want = [], []
    for p in (0.0, 0.5, 0.9, 1.0):
        for vals in (d, d[:1], d[:0]):
            cases.append(["quantile", f64(p), len(vals)] + [f64(x) for x in vals])
            want.append(("quantile", pmvs.cloud_quantile(vals, p)))
    for p, r in ((0.0, 0.0), (0.5, 0.0), (0.25, 0.75), (1.0, 1.0), (1 / 3, 0.1)):
        cases.append(["fscore", f64(p), f64(r)])
        want.append(("fscore", 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0))
    for a, b, top in ((NAN, NAN, NAN), (NAN, 2.0, 2.0), (3.0, NAN, 3.0), (1.0, 4.0, 4.0), (5.0, 4.0, 5.0)):
        cases.append(["larger", "nan" if math.isnan(a) else f64(a), "nan" if math.isnan(b) else f64(b)])
        want.append(("larger", top))
    got, _ = answers(exe, tmp_path, cases)
    for g, (key, w), case in zip(got, want, cases):
        assert list(g) == [key] and same(g[key], w), (case, g, w)


# ---- the normals ----------------------------------------------------------------------------------

TRUTH = np.float32([[0, 0, -3], [0, 1, 0], [0, 0, 0], [2, 2, 2], [0.6, 0, 0.8]])
# (index, dist, the query's normal): what it exercises, the angle it must give (None: it does not count)
QUERIES = {
    "zero_normal": ((4, 0.1, (0, 0, 0)), None),
    "nan_component": ((4, 0.1, (0, NAN, 1)), None),
    "zero_truth_normal": ((2, 0.1, (0, 0, 1)), None),
    "beyond_tau": ((4, 0.26, (0, 0, 1)), None),
    "no_match": ((-1, np.inf, (0, 0, 1)), None),
    "antiparallel": ((0, 0.1, (0, 0, 2)), 0.0),
    "orthogonal": ((1, 0.25, (1, 0, 0)), 90.0),
    "ratio_above_one": ((3, 0.0, (1, 1, 1)), 0.0),
    "oblique": ((4, 0.2, (0, 0, 1)), math.degrees(math.acos(
        np.float64(np.float32(0.8)) / math.sqrt(np.float64(np.float32(0.6)) ** 2 + np.float64(np.float32(0.8)) ** 2)))),
}


def normals_words(queries, stride, offset):
    words = ["normals", f64(TAU), stride, offset, len(TRUTH)] + [f32(x) for x in TRUTH.reshape(-1)]
    words.append(len(queries))
    for index, dist, normal in queries:
        words += [index, f32(dist)] + [f32(x) for x in normal]
    return words


def normal_error(queries):
    return pmvs.cloud_normal_error(np.float32([q[2] for q in queries]).reshape(-1, 3), TRUTH,
                                   np.int32([q[0] for q in queries]), np.float32([q[1] for q in queries]), TAU)


def angles_close(got, want):
    assert list(got) == ["n", "mean_deg", "median_deg", "p90_deg"] and got["n"] == want["n"]
    for key in ("mean_deg", "median_deg", "p90_deg"):
        if want["n"] == 0:
            assert got[key] is None and math.isnan(want[key])
        else:
            assert abs(got[key] - want[key]) <= 1e-9, (key, got[key], want[key])


def test_the_ratio_above_one_case_is_one():
    a, b = np.float64([1, 1, 1]), np.float64([2, 2, 2])
    assert (a @ b) / (np.sqrt(a @ a) * np.sqrt(b @ b)) > 1.0


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_normals_entry_of_one_query(exe, tmp_path, name):
    query, angle = QUERIES[name]
    (got,), _ = answers(exe, tmp_path, [normals_words([query], 24, 12)])
    angles_close(got, normal_error([query]))
    if angle is None:
        assert got == {"n": 0, "mean_deg": None, "median_deg": None, "p90_deg": None}
    else:
        assert got["n"] == 1 and got["mean_deg"] == got["median_deg"] == got["p90_deg"]
        assert abs(got["mean_deg"] - angle) <= 1e-9
        if angle == 0.0:
            assert got["mean_deg"] == 0.0  # acos(1): not NaN, not a rounding's worth of angle


# the records as tight as they come, and with bytes between a normal and the next record
@pytest.mark.parametrize("stride,offset", [(24, 12), (48, 12), (40, 16)])
def test_normals_entry_of_all_queries(exe, tmp_path, stride, offset):
    queries = [QUERIES[k][0] for k in sorted(QUERIES)]
    none = [q for q, angle in QUERIES.values() if angle is None]
    got, _ = answers(exe, tmp_path, [normals_words(queries, stride, offset), normals_words(none, stride, offset),
                                     normals_words([], stride, offset)])
    angles_close(got[0], normal_error(queries))
    assert got[0]["n"] == 4
    for g in got[1:]:
        assert g == {"n": 0, "mean_deg": None, "median_deg": None, "p90_deg": None}


# ---- the writer -----------------------------------------------------------------------------------

def test_a_long_member_list_is_whole(exe, tmp_path):
    # 40 members of 19 digits: some 1100 bytes, more than twice the largest of the buffers there were
    values = [(-1) ** i * (10 ** 18 + i * 123456789012345678 % (8 * 10 ** 18)) for i in range(39)] + [2 ** 63 - 1]
    assert all(len(str(abs(v))) == 19 for v in values)
    (got,), (line,) = answers(exe, tmp_path, [["integers", len(values)] + values])
    assert len(line) > 1000
    assert list(got) == ["k%d" % i for i in range(len(values))] and list(got.values()) == values
    (empty,), (line,) = answers(exe, tmp_path, [["integers", 0]])
    assert empty == {} and line == "{}"


def test_numbers_round_trip_and_what_is_not_finite_is_null(exe, tmp_path):
    rng = np.random.default_rng(5)
    values = list(rng.standard_normal(6) * 10.0 ** rng.integers(-300, 300, 6))
    values += [0.1, 1 / 3, 5e-324, 1.7976931348623157e308, -2.5e-7, 123456789.0]
    assert len(values) == 12
    words = [f64(v) for v in values] + ["nan", "inf", "-inf"]
    (got,), _ = answers(exe, tmp_path, [["numbers", len(words)] + words])
    assert len(got["array"]) == 15 and got["array"][12:] == [None, None, None]
    for g, v in zip(got["array"], values):
        assert np.float64(g).tobytes() == np.float64(v).tobytes()
    assert list(got["each"].values()) == got["array"]


def test_every_other_format(exe, tmp_path):
    x = 1234.56789123456789
    (got,), (line,) = answers(exe, tmp_path, [["formats", f64(x)]])
    assert got == {"yes": True, "no": False, "empty": {}, "name": "a b/c.ply", "ms": float("%.3f" % x),
                   "g9": float("%.9g" % x), "g17": x, "size": 2 ** 64 - 1, "least": -2 ** 63, "short": -3,
                   "dim": [7, -8, 2147483647], "none": [], "raw": [{}, "s", x], "outer": {"inner": {"deep": 1}},
                   "deep": 1}
    assert '"ms": %.3f, "g9": %.9g, "g17": %.17g, ' % (x, x, x) in line
    assert line.startswith('{"yes": true, "no": false, "empty": {}, "name": "a b/c.ply", ')
    assert line.endswith('"dim": [7, -8, 2147483647], "none": [], "raw": [{}, "s", %.17g], '
                         '"outer": {"inner": {"deep": 1}}, "deep": 1}' % x)
