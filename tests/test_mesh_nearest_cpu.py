"""dp_mesh_nearest without a GPU: the reference (tests/meshnearest_ref.py)
against independent statements of the distance to a triangle, its behaviour on
degenerate input, the Python layer's argument checks, the ctypes mirrors against
the header, and the arithmetic of mesh_compare and mesh_deviation."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs

import cloudnearest_ref as CR
import meshnearest_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def min_angle(a, b, c):
    def ang(u, v):
        return np.arccos(np.clip((u * v).sum(-1) / (np.linalg.norm(u, axis=-1) * np.linalg.norm(v, axis=-1)), -1, 1))
    return np.minimum(np.minimum(ang(b - a, c - a), ang(a - b, c - b)), ang(a - c, b - c))


@pytest.fixture(scope="module")
def fat_pairs():
    """2,000 (query, triangle) pairs: triangles in the unit cube with every angle
    at least 10 degrees, queries in the cube grown by a half"""
    rng = np.random.default_rng(20261022)
    tri = rng.random((20000, 3, 3), dtype=np.float32).astype(np.float64)
    keep = min_angle(tri[:, 0], tri[:, 1], tri[:, 2]) >= np.deg2rad(10.0)
    tri = tri[keep][:2000]
    assert len(tri) == 2000
    q = (rng.random((2000, 3), dtype=np.float32) * np.float32(2) - np.float32(0.5)).astype(np.float64)
    return q, tri, MR.pair_distance(q, tri[:, 0], tri[:, 1], tri[:, 2])


def test_the_reference_is_below_every_sample_of_the_triangle(fat_pairs):
    q, tri, r = fat_pairs
    n = 12
    for i in range(n + 1):
        for j in range(n + 1 - i):
            u, v = i / n, j / n
            p = tri[:, 0] * (1 - u - v) + tri[:, 1] * u + tri[:, 2] * v
            s2 = ((q - p) ** 2).sum(axis=1)
            assert (r["d2"] <= s2 * (1 + 2.0 ** -40)).all(), (i, j)
    # and the point it names is that far away (the point is rounded to float32)
    back = ((q - r["point"].astype(np.float64)) ** 2).sum(axis=1)
    assert np.allclose(np.sqrt(back), np.sqrt(r["d2"]), rtol=0, atol=4e-7)


def ericson(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5: the closest point by the
    seven Voronoi regions, in the arithmetic of the arguments"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + (d1 / (d1 - d3)) * ab
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + (d2 / (d2 - d6)) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
    den = 1 / (va + vb + vc)
    return a + ab * (vb * den) + ac * (vc * den)


# the largest relative discrepancy of d2 between the reference and Ericson's
# closest point in np.longdouble on fat_pairs, measured where this test was
# written (x86-64, 80-bit long double): 6.21e-15; the assertion
# allows 16 times that for another libm or numpy
MEASURED_REL = 6.21e-15


def test_the_reference_against_ericsons_regions_in_long_double(fat_pairs):
    q, tri, r = fat_pairs
    L = np.longdouble
    worst = 0.0
    for i in range(len(q)):
        p = ericson(q[i].astype(L), tri[i, 0].astype(L), tri[i, 1].astype(L), tri[i, 2].astype(L))
        e2 = ((q[i].astype(L) - p) ** 2).sum()
        worst = max(worst, float(abs(L(r["d2"][i]) - e2) / e2))
    print("largest relative discrepancy of d2: %.3g" % worst)
    assert worst <= 16 * MEASURED_REL


def test_every_region_of_a_triangle_wins():
    q, v, t, R, want = MR.seven_region_case()
    r = MR.nearest(q, v, t, R, hist_bins=4)
    assert (r["index"] == 0).all() and r["stats"]["matched"] == len(q) == 28
    assert r["label"].tolist() == want.tolist() and set(want.tolist()) == set(range(7))
    # hand-computed: above the face, beside an edge, beyond a vertex
    assert r["dist"][0] == np.float32(0.5) and r["closest"][0].tolist() == [1, 1, 0]
    assert r["dist"][4] == np.float32(math.sqrt(1.25)) and r["closest"][4].tolist() == [2, 0, 0]
    assert r["dist"][16] == np.float32(math.sqrt(2)) and r["closest"][16].tolist() == [0, 0, 0]
    assert r["closest"][8].tolist() == [2, 2, 0] and r["closest"][24].tolist() == [0, 4, 0]


def test_three_four_five_and_the_inclusive_radius():
    v, t = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]])
    r = MR.nearest(f32([[-3, -4, 0]]), v, t, 5.0)
    assert r["index"].tolist() == [0] and r["dist"].tolist() == [5.0] and r["closest"].tolist() == [[0, 0, 0]]
    below = np.nextafter(np.float32(5), np.float32(0))
    r = MR.nearest(f32([[-3, -4, 0]]), v, t, below)
    assert r["index"].tolist() == [-1] and r["dist"][0] == INF and (r["closest"] == INF).all()
    assert r["stats"]["unmatched"] == 1


def test_ties_go_to_the_lowest_triangle():
    # two triangles sharing the edge (0,0,0)-(0,1,0); the query beside that edge's line
    v = f32([[0, 0, 0], [0, 1, 0], [1, 0, 1], [-1, 0, 1]])
    for tris in ([[0, 1, 2], [1, 0, 3]], [[1, 0, 3], [0, 1, 2]]):
        r = MR.nearest(f32([[0, 0.5, -1]]), v, np.int32(tris), 2.0)
        assert r["index"].tolist() == [0] and r["dist"].tolist() == [1.0]


def test_never_nan():
    v = f32([[0, 0, 0], [0, 0, 0], [0, 0, 0],          # 0..2 coincide
             [1, 1, 1], [2, 2, 2], [3, 3, 3],          # 3..5 collinear
             [0, 0, 5], [1, 0, 5], [1, 1e-7, 5],       # 6..8 a 1e-7 radian sliver
             [np.nan, 0, 0], [np.inf, 0, 0], [0, 0, 9]])
    t = np.int32([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 0, 1], [3, 5, 3], [-1, 0, 1], [0, 1, 12], [2**31 - 1, 0, 1],
                  [9, 0, 3], [10, 11, 3], [-2**31, 5, 6]])
    assert MR.classify(v, t).tolist() == [0, 0, 0, 2, 2, 1, 1, 1, 3, 3, 1]
    q = f32([[0.5, 0, 0], [2.5, 2.5, 2.5], [4, 4, 4], [0.5, 0.25, 5], [0.5, 0, 5.5], [np.nan, 0, 0], [0, np.inf, 0]])
    r = MR.nearest(q, v, t, 2.0, hist_bins=8)
    assert r["index"].tolist() == [0, 1, 1, 2, 2, -1, -1]
    assert np.isfinite(r["dist"][:5]).all() and np.isfinite(r["closest"][:5]).all()
    assert r["dist"][0] == np.float32(0.5) and r["closest"][2].tolist() == [3, 3, 3]
    assert r["dist"][4] == np.float32(0.5) and (r["dist"][5:] == INF).all() and (r["closest"][5:] == INF).all()
    assert r["stats"] == dict(queries=5, skipped_queries=2, matched=5, unmatched=0, triangles=3, invalid_triangles=4,
                              degenerate_triangles=2, nonfinite_triangles=2)
    # the sliver's plane is not used: its edges answer
    P = v[6:9].astype(np.float64)
    pd = MR.pair_distance(q[3:5].astype(np.float64), P[None, 0].repeat(2, 0), P[None, 1].repeat(2, 0),
                          P[None, 2].repeat(2, 0))
    assert not pd["conditioned"].any() and (pd["label"] > 0).all() and np.isfinite(pd["d2"]).all()
    # no triangle takes part, or none is given
    r = MR.nearest(q, v, t[3:], 2.0, hist_bins=2)
    assert (r["index"] == -1).all() and r["stats"]["unmatched"] == 5 and r["hist"].tolist() == [0, 0]
    r = MR.nearest(q, f32([]), np.zeros((0, 3), np.int32), 2.0)
    assert (r["index"] == -1).all() and r["stats"]["triangles"] == 0
    r = MR.nearest(f32([]), v, t, 2.0, hist_bins=2)
    assert len(r["index"]) == 0 and r["closest"].shape == (0, 3) and r["stats"]["triangles"] == 3


def test_the_box_test_is_part_of_the_answer():
    # a query max_dist * (1 + 2^-20) from the triangle's box passes the box test and fails the radius
    v, t = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]])
    R = np.float32(0.5)
    r = MR.nearest(f32([[0.25, 0.25, 0.5], [0.25, 0.25, np.nextafter(R, np.float32(1))]]), v, t, R)
    assert r["index"].tolist() == [0, -1] and r["dist"][0] == R


def test_check_mesh_nearest_args_refuses_every_listed_error():
    ok = pmvs.check_mesh_nearest_args(3, 5, 4, 0.5, 32, 16)
    assert isinstance(ok, N.DpMeshNearestOptions) and (ok.max_dist, ok.hist_bins, ok.flags) == (0.5, 32, 0)
    bad = [
        dict(n_queries=-1), dict(n_queries=2**31), dict(n_vertices=-1), dict(n_vertices=2**31), dict(n_triangles=-1),
        dict(n_triangles=2**31), dict(n_queries=1.5), dict(n_triangles=True), dict(n_vertices=None),
        dict(query_stride=8), dict(query_stride=10), dict(query_stride=14), dict(query_stride=12.0),
        dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
        dict(max_dist=1e39), dict(max_dist=1e-50), dict(max_dist=None), dict(max_dist="1"), dict(max_dist=True),
        dict(hist_bins=-1), dict(hist_bins=65537), dict(hist_bins=1.0), dict(flags=1), dict(flags=-1),
        dict(inputs=(100, 200, 300), outputs=(200,)), dict(inputs=(100, 200, 300), outputs=(400, 500, 300)),
    ]
    for kw in bad:
        args = dict(dict(n_queries=3, n_vertices=5, n_triangles=4, max_dist=0.5), **kw)
        with pytest.raises(ValueError) as e:
            pmvs.check_mesh_nearest_args(**args)
        assert "mesh_nearest" in str(e.value) and "cloud" not in str(e.value) and "target" not in str(e.value)
    pmvs.check_mesh_nearest_args(2**31 - 1, 0, 0, 1e-45, 65536, 80)
    pmvs.check_mesh_nearest_args(0, 2**31 - 1, 2**31 - 1, 3e38, 0, 40, inputs=(100, 0, None), outputs=(300, 0, None))


def test_mesh_vertices_are_taken_as_records_or_rows():
    rec = np.zeros(3, N.MESH_VERTEX_DTYPE)
    rec["pos"] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert pmvs._mesh_vertices("t", rec).tobytes() == rec.tobytes()
    assert pmvs._mesh_vertices("t", rec["pos"].astype(np.float64)).tobytes() == rec.tobytes()
    assert len(pmvs._mesh_vertices("t", [])) == 0
    with pytest.raises(ValueError):
        pmvs._mesh_vertices("t", np.zeros((3, 2)))


def test_binding_matches_the_header():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = f.read()
    assert re.search(r"#define DP_ABI_VERSION\s+2\b", text)
    m = re.search(r"typedef struct dp_mesh_nearest_options \{(.*?)\} dp_mesh_nearest_options;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decl = re.findall(r"(float|int32_t)\s+(\w+);", body)
    assert [n for _, n in decl] == [n for n, _ in N.DpMeshNearestOptions._fields_] == ["max_dist", "hist_bins", "flags"]
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [ctype[t] for t, _ in decl] == [t for _, t in N.DpMeshNearestOptions._fields_]
    assert ctypes.sizeof(N.DpMeshNearestOptions) == 12
    assert [getattr(N.DpMeshNearestOptions, n).offset for n, _ in N.DpMeshNearestOptions._fields_] == [0, 4, 8]
    m = re.search(r"typedef struct dp_mesh_nearest_stats \{(.*?)\} dp_mesh_nearest_stats;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_int64 if typ == "int64_t" else ctypes.c_double) for n in names.split(",")]
    assert fields == list(N.DpMeshNearestStats._fields_)
    assert [n for n, _ in fields] == list(MR.COUNTS) + ["grid_cells", "grid_entries", "max_cell_entries", "build_ms",
                                                        "query_ms"]
    assert ctypes.sizeof(N.DpMeshNearestStats) == 8 * len(fields) == 104
    assert [getattr(N.DpMeshNearestStats, n).offset for n, _ in fields] == [8 * k for k in range(len(fields))]
    sigs = dict((s[0], s) for s in N.SIGNATURES)
    for name, count in (("dp_mesh_nearest", 14), ("dp_mesh_nearest_device", 15)):
        args = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")
        assert len(args) == len(sigs[name][2]) == count
        for a, t in zip(args, sigs[name][2]):
            assert ("*" in a) == (t is ctypes.c_void_p) and ("int64_t" in a and "*" not in a) == (t is ctypes.c_int64)
    assert hasattr(N.lib, "dp_mesh_nearest") and hasattr(N.lib, "dp_mesh_nearest_device")


class RefEngine:
    """the comparisons' engine, with the references as its searches"""
    def cloud_nearest(self, queries, targets, max_dist, hist_bins=0):
        return CR.nearest(queries, targets, max_dist, hist_bins)

    def mesh_nearest(self, queries, vertices, triangles, max_dist, hist_bins=0, closest=False):
        return MR.nearest(queries, vertices, triangles, max_dist, hist_bins)


def test_mesh_compare_on_a_planted_square():
    # the mesh: the square [0, 4]^2 at z = 0 as two triangles, its four corners the only vertices
    v = f32([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]])
    t = np.int32([[0, 1, 2], [0, 2, 3]])
    # the truth: points 0.25 above the square's inside (far from every vertex), one corner, one far away
    truth = f32([[2, 2, 0.25], [1, 3, 0.25], [3, 1, -0.25], [2, 1, 0.75], [0, 0, 0], [2, 2, 9]])
    got = pmvs.mesh_compare(RefEngine(), v, t, truth, 0.5, max_dist=1.0)
    acc, com = got["accuracy"], got["completeness"]
    # vertices -> truth: only the corner (0, 0, 0) has a truth point within 1
    assert (acc["n"], acc["matched"], acc["within_tau"]) == (4, 1, 1) and acc["ratio"] == 0.25 and acc["mean"] == 0.0
    # truth -> surface: 0.25, 0.25, 0.25, 0.75, 0, unmatched
    assert (com["n"], com["matched"], com["within_tau"]) == (6, 5, 4) and com["ratio"] == 4 / 6
    assert com["mean"] == pytest.approx(1.5 / 5) and com["median"] == 0.25 and com["p90"] == pytest.approx(0.25 + 0.5 * 0.6)
    p, r = 0.25, 4 / 6
    assert got["fscore"] == pytest.approx(2 * p * r / (p + r))
    # against the vertices alone the completeness is what cloud_compare says: one point within tau
    cloud = pmvs.cloud_compare(RefEngine(), v, truth, 0.5, max_dist=1.0)
    assert cloud["completeness"]["within_tau"] == 1 and cloud["accuracy"] == acc
    # records and rows are the same mesh
    rec = np.zeros(4, N.MESH_VERTEX_DTYPE)
    rec["pos"] = v
    CR.assert_compare(pmvs.mesh_compare(RefEngine(), rec, t, truth, 0.5, 1.0), got)
    for kw in (dict(tau=0.0), dict(tau=1.0, max_dist=0.5)):
        with pytest.raises(ValueError):
            pmvs.mesh_compare(RefEngine(), v, t, truth, **kw)


def test_mesh_deviation_on_two_planted_squares():
    a = (f32([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]]), np.int32([[0, 1, 2], [0, 2, 3]]))
    # b: the same square lifted by 0.5, with a fifth vertex in the middle lifted by 1.5, and one at z = 50
    b = (f32([[0, 0, 0.5], [4, 0, 0.5], [4, 4, 0.5], [0, 4, 0.5], [2, 2, 1.5], [2, 2, 50]]),
         np.int32([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]]))
    got = pmvs.mesh_deviation(RefEngine(), a, b, 2.0)
    ab, ba = got["a_to_b"], got["b_to_a"]
    assert (ab["n"], ab["matched"]) == (4, 4) and ab["mean"] == ab["median"] == ab["p90"] == ab["max"] == 0.5
    # b's corners are 0.5 above a, its apex 1.5, the stray vertex beyond the radius
    assert (ba["n"], ba["matched"]) == (6, 5) and ba["max"] == 1.5 and ba["median"] == 0.5
    assert ba["mean"] == pytest.approx(3.5 / 5) and ba["p90"] == pytest.approx(0.5 + 1.0 * 0.6)
    assert got["max"] == 1.5 and set(got) == {"a_to_b", "b_to_a", "max"}
    assert set(ab) == {"n", "matched", "mean", "median", "p90", "max"}
    none = pmvs.mesh_deviation(RefEngine(), a, (f32([]), np.zeros((0, 3), np.int32)), 2.0)
    assert none["a_to_b"]["matched"] == 0 and math.isnan(none["max"]) and none["b_to_a"]["n"] == 0
