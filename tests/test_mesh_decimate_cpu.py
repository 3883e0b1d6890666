"""dp_mesh_decimate without a GPU: the properties of the CPU reference
(tests/meshdecimate_ref.py, restated from the spec in include/densepoints.h) on
the meshes the GPU test compares the kernels on, the counts of its three
placement branches, the argument check of the Python layer and the header /
ctypes agreement."""
import ctypes
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs

import meshdecimate_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPHERE = dict(cell=0.5, origin=(0.0, 0.0, 0.0))
CUBE = dict(cell=0.25, origin=(-0.0625, -0.0625, -0.0625))


@pytest.fixture(scope="module")
def sphere():
    return DR.uv_sphere(24, 48)


@pytest.fixture(scope="module")
def cube():
    return DR.cube(8)


@pytest.fixture(scope="module")
def results(sphere, cube):
    """the reference's results the tests below share, computed once"""
    planted = DR.planted_mesh()
    out = {}
    for quadric in (False, True):
        out["sphere", quadric] = DR.decimate(*sphere, quadric=quadric, **SPHERE)
        out["cube", quadric] = DR.decimate(*cube, quadric=quadric, **CUBE)
        out["planted", quadric] = DR.decimate(*planted, quadric=quadric, **DR.PLANTED)
    return out


def directed_edges(tris):
    t = np.asarray(tris).reshape(-1, 3)
    return [(int(a), int(b)) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))]


def assert_closed(tris):
    """every edge once per direction"""
    edges = directed_edges(tris)
    assert len(set(edges)) == len(edges)
    assert set(edges) == {(b, a) for a, b in edges}


def assert_consistent(verts, tris, r):
    """what holds for every result: indices in range, no unused output vertex, no
    collapsed or duplicate output triangle, maps that agree with the outputs, the
    placement counts"""
    st, vo, to = r["stats"], r["vertices"], r["triangles"]
    assert st["vertices_out"] == len(vo) and st["triangles_out"] == len(to)
    assert st["quadric_vertices"] + st["mean_vertices"] == st["vertices_out"]
    assert st["clusters"] - st["orphan_clusters"] == st["vertices_out"]
    if len(to):
        assert to.min() >= 0 and to.max() < len(vo)
    assert np.array_equal(np.unique(to), np.arange(len(vo)))
    assert not ((to[:, 0] == to[:, 1]) | (to[:, 1] == to[:, 2]) | (to[:, 0] == to[:, 2])).any()
    canon = [min((a, b, c), (b, c, a), (c, a, b)) for a, b, c in to.tolist()]
    assert len(set(canon)) == len(canon)
    vm, tm = r["vertex_map"], r["triangle_map"]
    assert len(vm) == len(verts) and len(tm) == len(tris)
    kept = np.flatnonzero(tm >= 0)
    assert np.array_equal(tm[kept], np.arange(len(to)))  # input order
    assert np.array_equal(vm[tris[kept]], to)            # positions kept, indices through the vertex map
    assert set(vm[vm >= 0].tolist()) == set(range(len(vo)))
    assert (vo["pad"] == 0).all()


def test_sphere_counts_and_branches(sphere, results):
    """24 x 48 UV sphere at cell 0.5: quadric placements and one candidate outside its cell"""
    verts, tris = sphere
    assert (len(verts), len(tris)) == (1200, 2304)
    r = results["sphere", True]
    st = r["stats"]
    assert (st["clusters"], st["triangles_out"], st["max_cluster"]) == (59, 112, 66)
    assert (st["quadric_vertices"], st["mean_vertices"]) == (58, 1)
    assert r["placement"].count("quadric") == 58 and r["placement"].count("outside") == 1
    assert st["orphan_clusters"] == 0 and st["duplicate_triangles"] == 0
    m = results["sphere", False]
    assert m["stats"]["mean_vertices"] == 59 and m["stats"]["quadric_vertices"] == 0
    assert np.array_equal(m["triangles"], r["triangles"]) and np.array_equal(m["vertex_map"], r["vertex_map"])
    # (a pole row is 48 vertices at one point that no triangle joins: the sphere is
    # closed as a surface, not as an index mesh, so closedness is the cube's test)
    for q in (False, True):
        assert_consistent(verts, tris, results["sphere", q])


def test_cube_counts_and_branches(cube, results):
    """the 8 x 8 cube at cell 0.25: the corners are solvable, faces and edges take the mean"""
    verts, tris = cube
    assert (len(verts), len(tris)) == (386, 768)
    assert_closed(tris)
    r = results["cube", True]
    st = r["stats"]
    assert (st["clusters"], st["triangles_out"]) == (98, 192)
    assert (st["quadric_vertices"], st["mean_vertices"]) == (8, 90)
    assert r["placement"].count("unsolvable") == 90
    # the quadric puts the corner clusters on the cube's corners: three exact planes
    # and a well-conditioned 3 x 3 solve in fp64, so within a few fp64 roundings
    corners = r["vertices"]["pos"][[i for i, p in enumerate(r["placement"]) if p == "quadric"]]
    want = np.repeat([[0.0], [1.0]], 4, axis=0) * np.ones(3)
    assert np.allclose(np.sort(corners.astype(np.float64), axis=0), want, rtol=0, atol=1e-12)
    for q in (False, True):
        assert_consistent(verts, tris, results["cube", q])
        assert st["duplicate_triangles"] == 0
        assert_closed(results["cube", q]["triangles"])


def test_planted_cases(results):
    verts, tris = DR.planted_mesh()
    for q in (False, True):
        r = results["planted", q]
        st = r["stats"]
        assert_consistent(verts, tris, r)
        assert (st["invalid_triangles"], st["degenerate_triangles"], st["unused_vertices"]) == (2, 1, 1)
        assert (st["clamped_vertices"], st["collapsed_triangles"], st["duplicate_triangles"]) == (1, 1, 1)
        assert (st["clusters"], st["orphan_clusters"], st["max_cluster"]) == (6, 1, 3)
        tm, vm = r["triangle_map"], r["vertex_map"]
        # the first of the two equal triples stays, the oppositely wound one too; its indices keep their places
        assert tm.tolist() == [0, -1, 1, -1, -1, -1, -1, 2]
        assert r["triangles"][0].tolist() == vm[[0, 1, 2]].tolist() and r["triangles"][1].tolist() == vm[[6, 8, 7]].tolist()
        assert vm[0] == vm[3] == vm[6] and vm[1] == vm[4] == vm[7] and vm[2] == vm[5] == vm[8]
        assert (vm[9:13] == -1).all()
        # cell order (k_z, k_y, k_x): the negative x cell before cell 0 (floor), the clamped one after cell 1
        assert vm[14] == 0 and vm[0] == 1 and vm[1] == 2 and vm[13] == 3 and vm[2] == 4
        assert DR.cell_of(verts["pos"][14], [0.0] * 3, 1.0) == ((0, 0, -1), False)
        assert DR.cell_of(verts["pos"][13], [0.0] * 3, 1.0) == ((0, 0, 2**20 - 1), True)
    assert DR.cell_of([np.nan, -4.0e6, 0.0], [0.0] * 3, 1.0) == ((0, -2**20, -2**20), True)


def test_tiny_cell_keeps_the_proper_mesh(cube):
    """a cell far below the smallest edge, MEAN: the proper triangles' mesh, its
    vertices in cell order and their records bit for bit"""
    verts, tris = cube
    verts = verts.copy()
    tris = np.concatenate([tris, [(0, 0, 1), (-1, 2, 3)]]).astype(np.int32)
    r = DR.decimate(verts, tris, 1.0 / 1024, (-0.5 / 1024,) * 3, False)
    st = r["stats"]
    assert st["clusters"] == len(verts) == st["vertices_out"] and st["triangles_out"] == 768 and st["max_cluster"] == 1
    assert (st["collapsed_triangles"], st["duplicate_triangles"], st["invalid_triangles"], st["degenerate_triangles"]) == \
        (0, 0, 1, 1)
    order = np.lexsort((verts["pos"][:, 0], verts["pos"][:, 1], verts["pos"][:, 2]))
    assert r["vertices"].tobytes() == verts[order].tobytes()
    assert np.array_equal(r["vertex_map"][order], np.arange(len(verts)))
    assert np.array_equal(r["triangles"], r["vertex_map"][tris[:768]])


def test_one_huge_cell_leaves_nothing(sphere):
    verts, tris = sphere
    for q in (False, True):
        r = DR.decimate(verts, tris, 64.0, (-32.0, -32.0, -32.0), q)
        st = r["stats"]
        assert (st["clusters"], st["orphan_clusters"], st["max_cluster"]) == (1, 1, 1200)
        assert st["collapsed_triangles"] == 2304 and st["vertices_out"] == 0 and st["triangles_out"] == 0
        assert len(r["vertices"]) == 0 and r["triangles"].shape == (0, 3)
        assert (r["vertex_map"] == -1).all() and (r["triangle_map"] == -1).all()


def test_empty_inputs():
    for nv, tris in ((0, []), (5, []), (0, [(0, 1, 2)])):
        r = DR.decimate(DR.random_vertices(nv, 1), tris, 1.0)
        assert r["stats"]["vertices_out"] == 0 and r["stats"]["clusters"] == 0 and r["stats"]["unused_vertices"] == nv


def test_check_mesh_decimate_args_accepts_and_fills_the_struct():
    o = pmvs.check_mesh_decimate_args(0.5)
    assert (list(o.origin), o.cell, o.mode, o.flags, o.reserved) == ([0.0, 0.0, 0.0], 0.5, N.DP_DECIMATE_MEAN, 0, 0)
    o = pmvs.check_mesh_decimate_args(np.float32(2), (1, -2.5, np.float64(3)), True)
    assert (list(o.origin), o.cell, o.mode) == ([1.0, -2.5, 3.0], 2.0, N.DP_DECIMATE_QUADRIC)
    pmvs.check_mesh_decimate_args(cell=1e-30, origin=np.array([0.0, 1e30, -1e30]), quadric=np.bool_(False))


@pytest.mark.parametrize("bad", [dict(cell=0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")),
                                 dict(cell=1e-60), dict(cell=1e39), dict(cell="1"), dict(cell=True), dict(cell=None),
                                 dict(cell=1.0, origin=(0, 0)), dict(cell=1.0, origin=(0, 0, float("nan"))),
                                 dict(cell=1.0, origin=(0, float("inf"), 0)), dict(cell=1.0, origin=(0, 0, 1e39)),
                                 dict(cell=1.0, origin=5), dict(cell=1.0, origin=(0, 0, "x")),
                                 dict(cell=1.0, quadric=1), dict(cell=1.0, quadric=2), dict(cell=1.0, quadric=None)],
                         ids=repr)
def test_check_mesh_decimate_args_rejects(bad):
    with pytest.raises(ValueError):
        pmvs.check_mesh_decimate_args(**bad)


def test_decimate_cell_of_pmvs_mesh():
    assert pmvs.decimate_cell(dict(cell=0.25), 0.1) == dict(cell=0.25)
    d = pmvs.decimate_cell(dict(factor=2, quadric=True), 0.1)
    assert d == dict(cell=float(np.float32(2.0 * float(np.float32(0.1)))), quadric=True)
    for bad in (dict(), dict(quadric=True), dict(cell=1.0, factor=2), dict(factor=0), dict(factor=float("nan")),
                dict(factor="2"), dict(cell=1.0, mode=1)):
        with pytest.raises(ValueError):
            pmvs.decimate_cell(bad, 0.1)


def test_header_declares_and_ctypes_binds():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym, n_args in (("dp_default_mesh_decimate_options", 1), ("dp_mesh_decimate", 13), ("dp_mesh_decimate_device", 16)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, text)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args == len(bound[sym]), sym
        assert hasattr(N.lib, sym)
    assert "#define DP_DECIMATE_DET_EPS 1e-6" in text and float(DR.DET_EPS) == 1e-6
    assert (N.DP_DECIMATE_MEAN, N.DP_DECIMATE_QUADRIC) == (0, 1)
    assert ctypes.sizeof(N.DpMeshDecimateOptions) == 28 and ctypes.sizeof(N.DpMeshDecimateStats) == 128
    assert [n for n, _ in N.DpMeshDecimateStats._fields_] == list(DR.COUNTS) + ["decimate_ms"]
    o = N.DpMeshDecimateOptions()
    o.cell, o.mode, o.flags = 3.0, 1, 7
    N.lib.dp_default_mesh_decimate_options(ctypes.byref(o))
    assert (list(o.origin), o.cell, o.mode, o.flags, o.reserved) == ([0.0] * 3, 0.0, 0, 0, 0)
