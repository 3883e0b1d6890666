"""dp_mesh_adjacency / dp_mesh_smooth / dp_mesh_normals without a GPU: the CPU
reference (tests/meshsmooth_ref.py, restated from the spec in
include/densepoints.h) against answers written out by hand and against
orderings on a noisy sphere, and the host-side pieces: bindings, struct
layouts, argument validation, the PLY writer."""
import ctypes
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs
from densepoints_amd._native import MESH_VERTEX_DTYPE

import meshsmooth_ref as SR
import tsdf_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_default_mesh_smooth_options", "dp_mesh_adjacency", "dp_mesh_adjacency_device", "dp_mesh_smooth",
       "dp_mesh_smooth_device", "dp_mesh_normals", "dp_mesh_normals_device")


def rows(adj):
    off = adj["offsets"]
    return [adj["neighbours"][off[v]:off[v + 1]].tolist() for v in range(len(off) - 1)]


def counts(adj):
    off = adj["offsets"]
    return [adj["edge_triangles"][off[v]:off[v + 1]].tolist() for v in range(len(off) - 1)]


def test_one_triangle():
    adj = SR.adjacency([(0, 1, 2)], 3)
    assert adj["offsets"].tolist() == [0, 2, 4, 6]
    assert rows(adj) == [[1, 2], [0, 2], [0, 1]] and counts(adj) == [[1, 1]] * 3
    assert adj["vertex_flags"].tolist() == [1, 1, 1]
    assert adj["stats"] == dict(vertices_in=3, triangles_in=1, invalid_triangles=0, degenerate_triangles=0,
                                isolated_vertices=0, edges=3, boundary_edges=3, nonmanifold_edges=0,
                                boundary_vertices=3, max_valence=2)


def test_two_triangles_on_a_shared_edge():
    adj = SR.adjacency([(0, 1, 2), (2, 1, 3)], 4)
    assert rows(adj) == [[1, 2], [0, 2, 3], [0, 1, 3], [1, 2]]
    assert counts(adj) == [[1, 1], [1, 2, 1], [1, 2, 1], [1, 1]]
    assert adj["vertex_flags"].tolist() == [1, 1, 1, 1]
    assert adj["stats"]["edges"] == 5 and adj["stats"]["boundary_edges"] == 4 and adj["stats"]["max_valence"] == 3


TETRA = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]


def test_tetrahedron_is_closed():
    adj = SR.adjacency(TETRA, 4)
    assert rows(adj) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]] and counts(adj) == [[2, 2, 2]] * 4
    assert adj["vertex_flags"].tolist() == [0, 0, 0, 0]
    st = adj["stats"]
    assert (st["edges"], st["boundary_edges"], st["nonmanifold_edges"], st["boundary_vertices"], st["max_valence"]) == \
        (6, 0, 0, 0, 3)


def test_tetrahedron_centroid_step_by_hand():
    """lambda = 0.5, one plain step: every vertex moves half way to the mean of the other three"""
    v = np.zeros(4, MESH_VERTEX_DTYPE)
    v["pos"] = [(0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 16)]
    v["rgb"], v["pad"] = [(1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)], [9, 8, 7, 6]
    out = SR.smooth(v, TETRA, iterations=1, lam=0.5, mu=0.0)
    # means of the others: (4/3, 8/3, 16/3), (0, 8/3, 16/3), (4/3, 0, 16/3), (4/3, 8/3, 0)
    want = np.array([(2 / 3, 4 / 3, 8 / 3), (2, 4 / 3, 8 / 3), (2 / 3, 4, 8 / 3), (2 / 3, 4 / 3, 8)])
    assert np.array_equal(out["vertices"]["pos"], want.astype(np.float32))
    assert out["vertices"]["rgb"].tolist() == v["rgb"].tolist() and out["vertices"]["pad"].tolist() == [9, 8, 7, 6]
    assert out["stats"]["steps"] == 1 and out["stats"]["movable_vertices"] == 4 and out["stats"]["pinned_vertices"] == 0
    # with mu: two steps per iteration
    assert SR.smooth(v, TETRA, iterations=3)["stats"]["steps"] == 6


def test_bow_tie_and_nonmanifold_edge():
    bow = SR.adjacency([(0, 1, 2), (2, 3, 4)], 5)
    assert rows(bow)[2] == [0, 1, 3, 4] and bow["vertex_flags"].tolist() == [1] * 5
    assert bow["stats"]["nonmanifold_edges"] == 0 and bow["stats"]["edges"] == 6
    three = SR.adjacency([(0, 1, 2), (0, 1, 3), (1, 0, 4)], 5)
    assert counts(three)[0] == [3, 1, 1, 1] and rows(three)[0] == [1, 2, 3, 4]
    assert three["vertex_flags"].tolist() == [3, 3, 1, 1, 1]
    assert three["stats"]["nonmanifold_edges"] == 1 and three["stats"]["boundary_edges"] == 6


def test_degenerate_invalid_duplicate_and_empty():
    tris = [(0, 1, 1), (2, 2, 2), (-1, 0, 1), (0, 1, 6), (3, 4, 5), (3, 4, 5), (5, 3, 4)]
    adj = SR.adjacency(tris, 6)
    st = adj["stats"]
    assert st["invalid_triangles"] == 2 and st["degenerate_triangles"] == 2 and st["isolated_vertices"] == 3
    assert rows(adj) == [[], [], [], [4, 5], [3, 5], [3, 4]] and counts(adj)[3] == [3, 3]
    assert adj["vertex_flags"].tolist() == [0, 0, 0, 2, 2, 2] and st["nonmanifold_edges"] == 3 and st["edges"] == 3
    for nv, t in ((0, []), (4, []), (0, [(0, 0, 0)])):
        e = SR.adjacency(t, nv)
        assert e["offsets"].tolist() == [0] * (nv + 1) and len(e["neighbours"]) == 0
        assert e["stats"]["isolated_vertices"] == nv and e["stats"]["max_valence"] == 0
        assert e["stats"]["invalid_triangles"] == len(t)
        assert SR.normals(SR.random_vertices(nv, 1), t)["stats"]["zero_normals"] == nv
        assert len(SR.smooth(SR.random_vertices(nv, 1), t)["vertices"]) == nv
    # isolated vertices and the vertices of degenerate triangles do not move
    v = SR.random_vertices(6, 2)
    out = SR.smooth(v, tris, iterations=2)["vertices"]
    assert out[:3].tobytes() == v[:3].tobytes() and not np.array_equal(out["pos"][3:], v["pos"][3:])


@pytest.fixture(scope="module")
def sphere():
    """the closed sphere mesh of test_tsdf_cpu.py's case (tsdf_ref's integration
    and mesh of 12 views), clean and with Gaussian vertex noise of a fifth of a voxel"""
    from test_tsdf_cpu import SphereCase

    case = SphereCase()
    verts = case.mesh["vertices"].astype(MESH_VERTEX_DTYPE)
    return case, verts, SR.noisy(verts, 0.2 * case.VOXEL, 7), case.mesh["triangles"]


def test_sphere_smoothing_orderings(sphere):
    """orderings only: Taubin lowers the roughness, and keeps the volume better than plain Laplacian"""
    case, clean, noisy, tris = sphere
    adj = SR.adjacency(tris, len(noisy))
    assert adj["stats"]["boundary_edges"] == 0 and adj["stats"]["nonmanifold_edges"] == 0  # closed
    assert adj["stats"]["isolated_vertices"] == 0 and (adj["vertex_flags"] == 0).all()
    taubin = SR.smooth(noisy, tris, iterations=10)
    laplace = SR.smooth(noisy, tris, iterations=10, mu=0.0)
    assert SR.roughness(taubin["vertices"]["pos"], adj) < SR.roughness(noisy["pos"], adj)
    v0 = SR.volume(noisy["pos"], tris)
    assert v0 > 0
    assert abs(SR.volume(taubin["vertices"]["pos"], tris) - v0) < abs(SR.volume(laplace["vertices"]["pos"], tris) - v0)
    assert taubin["vertices"]["rgb"].tobytes() == noisy["rgb"].tobytes()
    assert taubin["stats"]["steps"] == 20 and laplace["stats"]["steps"] == 10
    assert taubin["stats"]["movable_vertices"] == len(noisy)
    # iterations = 0 is the identity
    assert SR.smooth(noisy, tris, iterations=0)["vertices"].tobytes() == noisy.tobytes()


def test_sphere_normals_point_outwards(sphere):
    """the winding rule of dp_tsdf_mesh: every non-zero normal of the noise-free
    sphere has a positive dot product with (v - centre)"""
    case, clean, _, tris = sphere
    nrm = SR.normals(clean, tris)
    n = nrm["normals"].astype(np.float64)
    nonzero = (n != 0).any(axis=1)
    assert nrm["stats"]["zero_normals"] == int((~nonzero).sum()) == 0
    assert np.allclose(np.linalg.norm(n[nonzero], axis=1), 1.0, atol=1e-6)
    out = (n * (clean["pos"].astype(np.float64) - case.CENTRE)).sum(axis=1)
    assert (out[nonzero] > 0).all(), int((out[nonzero] <= 0).sum())


def test_open_sheet_pins_its_boundary():
    tris, nv = SR.grid_sheet(7)
    v = SR.grid_vertices(7, 5)
    adj = SR.adjacency(tris, nv)
    border = adj["vertex_flags"] & 1 != 0
    idx = np.arange(49).reshape(7, 7)
    want = np.zeros(49, bool)
    want[np.concatenate([idx[0], idx[-1], idx[:, 0], idx[:, -1]])] = True
    assert np.array_equal(border, want) and adj["stats"]["boundary_vertices"] == 24
    pinned = SR.smooth(v, tris, iterations=3)
    assert pinned["vertices"][border].tobytes() == v[border].tobytes()
    assert (pinned["vertices"]["pos"][~border] != v["pos"][~border]).any(axis=1).all()
    assert pinned["stats"]["pinned_vertices"] == 24 and pinned["stats"]["movable_vertices"] == 25
    free = SR.smooth(v, tris, iterations=3, free_boundary=True)
    assert (free["vertices"]["pos"][border] != v["pos"][border]).any(axis=1).all()
    assert free["stats"]["pinned_vertices"] == 0 and free["stats"]["movable_vertices"] == 49


def test_normals_by_hand():
    v = np.zeros(5, MESH_VERTEX_DTYPE)
    v["pos"] = [(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 3), (7, 7, 7)]
    # two triangles at right angles of areas 2 and 3: vertex 0 sums (0, 0, 4) + (0, -6, 0)
    nrm = SR.normals(v, [(0, 1, 2), (0, 1, 3), (4, 4, 0)])
    s = np.array([0.0, -6.0, 4.0])
    assert np.array_equal(nrm["normals"][0], (s / np.sqrt(52.0)).astype(np.float32))
    assert nrm["normals"][2].tolist() == [0, 0, 1] and nrm["normals"][3].tolist() == [0, -1, 0]
    assert nrm["normals"][4].tolist() == [0, 0, 0]
    assert nrm["stats"]["zero_normals"] == 1 and nrm["stats"]["degenerate_triangles"] == 1


def test_header_declares_and_native_binds_the_calls():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        header = f.read()
    bound = {name for name, _, _ in N.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound and hasattr(N.lib, name)
    assert "#define DP_ABI_VERSION 2" in header
    assert ctypes.sizeof(N.DpMeshSmoothOptions) == 20
    assert ctypes.sizeof(N.DpMeshAdjacencyStats) == 8 * 11 and ctypes.sizeof(N.DpMeshSmoothStats) == 8 * 15
    assert ctypes.sizeof(N.DpMeshNormalsStats) == 8 * 6
    o = N.DpMeshSmoothOptions()
    N.lib.dp_default_mesh_smooth_options(ctypes.byref(o))
    assert (o.iterations, getattr(o, "lambda"), o.mu, o.flags, o.reserved) == \
        (10, 0.5, float(np.float32(-0.53)), 0, 0)


def test_check_mesh_smooth_args_accepts_and_fills_the_struct():
    o = pmvs.check_mesh_smooth_args()
    assert (o.iterations, getattr(o, "lambda"), o.mu, o.flags) == (10, 0.5, float(np.float32(-0.53)), 0)
    o = pmvs.check_mesh_smooth_args(0, 1.0, 0.0, True)
    assert (o.iterations, getattr(o, "lambda"), o.mu, o.flags) == (0, 1.0, 0.0, N.DP_SMOOTH_FREE_BOUNDARY)
    pmvs.check_mesh_smooth_args(iterations=np.int64(1000), lam=np.float32(0.25), mu=-2)


@pytest.mark.parametrize("bad", [
    dict(iterations=-1), dict(iterations=1001), dict(iterations=1.5), dict(iterations=True), dict(iterations=None),
    dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan")), dict(lam="0.5"), dict(lam=1e-60),
    dict(mu=0.1), dict(mu=float("nan")), dict(mu=float("-inf")), dict(mu=None),
    dict(free_boundary=1), dict(free_boundary=None),
])
def test_check_mesh_smooth_args_rejects(bad):
    with pytest.raises(ValueError):
        pmvs.check_mesh_smooth_args(**bad)


def test_pmvs_mesh_checks_smooth_before_any_work():
    p = pmvs.PMVS.__new__(pmvs.PMVS)
    p._ran = True
    with pytest.raises(ValueError, match="mesh_smooth"):
        p.mesh(smooth=dict(iterations=-1))
    with pytest.raises(TypeError):
        p.mesh(smooth=dict(lambda_=0.5))


def legacy_mesh_ply(path, vertices, triangles):
    """the writer as it was before normals: the bytes a file without normals must keep"""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {len(vertices)}\n")
        for n in ("x", "y", "z"):
            f.write(f"property float {n}\n")
        for n in ("red", "green", "blue"):
            f.write(f"property uchar {n}\n")
        f.write(f"element face {len(triangles)}\n")
        f.write("property list uchar int vertex_indices\n")
        f.write("end_header\n")
        for v in vertices:
            x, y, z = (float(c) for c in v["pos"])
            r, g, b = (int(c) for c in v["rgb"])
            f.write(f"{x:.9g} {y:.9g} {z:.9g} {r} {g} {b}\n")
        for t in triangles:
            f.write(f"3 {int(t[0])} {int(t[1])} {int(t[2])}\n")


def test_write_mesh_ply_with_and_without_normals(tmp_path):
    tris = np.array(TETRA, np.int32)
    v = SR.random_vertices(4, 3)
    a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    pmvs.write_mesh_ply(a, v, tris)
    legacy_mesh_ply(b, v, tris)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    nrm = SR.normals(v, tris)["normals"]
    pmvs.write_mesh_ply(c, v, tris, nrm)
    with open(c) as f:
        lines = f.read().split("\n")
    assert lines[:13] == ["ply", "format ascii 1.0", "element vertex 4", "property float x", "property float y",
                          "property float z", "property uchar red", "property uchar green", "property uchar blue",
                          "property float nx", "property float ny", "property float nz", "element face 4"]
    assert lines[13:15] == ["property list uchar int vertex_indices", "end_header"]
    for k in range(4):
        f9 = lines[15 + k].split()
        assert len(f9) == 9
        assert np.array_equal(np.array(f9[:3], np.float32), v["pos"][k]) and [int(x) for x in f9[3:6]] == v["rgb"][k].tolist()
        assert np.array_equal(np.array(f9[6:], np.float32), nrm[k])
    assert lines[19] == "3 0 1 2"
    with pytest.raises(ValueError):
        pmvs.write_mesh_ply(c, v, tris, nrm[:3])
