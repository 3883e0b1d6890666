"""dp_tsdf_integrate / dp_tsdf_mesh without a GPU: the CPU reference
(tests/tsdf_ref.py, restated from the spec in include/densepoints.h) against
analytic geometry -- a sphere seen from all around and a plane --, and the
host-side pieces: bindings, struct layouts, the PLY writer, argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import pmvs, synth
from densepoints_amd._native import MESH_VERTEX_DTYPE, DpMeshStats, DpTsdfOptions, DpTsdfStats

import tsdf_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_default_tsdf_options", "dp_tsdf_integrate", "dp_tsdf_integrate_device", "dp_tsdf_mesh",
       "dp_tsdf_mesh_device")
BACKGROUND = 5.0  # projective depth of the pixels that see nothing: far behind every volume used here


def ray_depths(P, W, H, hit):
    """the projective depth of every pixel of a W x H view with projection P:
    X = C + t M^-1 (x, y, 1) has row_2(P, X) = t, so hit(C, dirs) -- the ray
    parameter of the surface, NaN where the ray misses -- is the depth itself"""
    M, p4 = P[:, :3], P[:, 3]
    C = -np.linalg.solve(M, p4)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.einsum("ij,jhw->ihw", np.linalg.inv(M), np.stack([x, y, np.ones_like(x)]))
    t = hit(C, dirs)
    return np.where(np.isfinite(t) & (t > 0), t, BACKGROUND).astype(np.float32)


class SphereCase:
    """a sphere of 12 voxels radius, off the lattice, seen by 12 of the synthetic
    scene's cameras spread over 170 degrees of polar angle (all around it), each
    320 x 240 with a seeded random image; pixels that miss it see a background far
    behind the volume.  trunc is 4 voxels: every voxel outside the sphere and every
    voxel less than trunc inside it is observed, and the voxels deeper inside are
    seen by no view -- they have to be: a truncation that reaches the centre lets
    the thin chords of grazing rays count voxels behind the limb as inside, which
    moves the surface by more than the bound below.  The unobserved core holds no
    sign change, so the mesh is still closed."""
    R, VOXEL, DIM, TRUNC = 0.3, 0.025, (32, 32, 32), 0.1
    CENTRE = np.array([0.013, -0.021, 0.008])
    ORIGIN = (-0.4, -0.4, -0.4)

    def __init__(self):
        V, W, H = 12, 320, 240
        cfg = synth.config(V, W, H, 1, spread_deg=170.0)
        self.P = synth.cameras(cfg)
        rng = np.random.default_rng(20261020)
        self.images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(V)]
        self.vw = TR.Views(self.P, [W] * V, [H] * V, self.images)

        def hit(C, d):
            oc = C - self.CENTRE
            a = (d * d).sum(axis=0)
            b = np.einsum("i,ihw->hw", oc, d)
            disc = b * b - a * (oc @ oc - self.R ** 2)
            with np.errstate(invalid="ignore"):
                return np.where(disc > 0, (-b - np.sqrt(disc)) / a, np.nan)

        self.depth = [ray_depths(self.P[v], W, H, hit) for v in range(V)]
        self.vol = TR.integrate(self.vw, self.depth, origin=self.ORIGIN, voxel=self.VOXEL, dim=self.DIM,
                                trunc=self.TRUNC)
        self.mesh = TR.mesh(self.vol["tsdf"], self.vol["weight"], self.vol["rgb"], origin=self.ORIGIN,
                            voxel=self.VOXEL, dim=self.DIM)


class PlaneCase:
    """the plane z = 0 seen by the four cameras of scene plane4 (640 x 480, all on
    its +z side), in a slab of 24 x 24 x 8 voxels around it; trunc is 3 voxels, so
    the lowest layer of voxels is behind the surface for every view"""
    VOXEL, DIM, TRUNC, ORIGIN = 0.025, (24, 24, 8), 0.075, (-0.3, -0.3, -0.1)

    def __init__(self):
        V, W, H = 4, 640, 480
        self.P = synth.cameras(synth.config(V, W, H, 0, depth_noise=0.0))
        self.vw = TR.Views(self.P, [W] * V, [H] * V)
        self.depth = [ray_depths(self.P[v], W, H, lambda C, d: -C[2] / d[2]) for v in range(V)]
        assert all((z != np.float32(BACKGROUND)).all() for z in self.depth)
        self.vol = TR.integrate(self.vw, self.depth, origin=self.ORIGIN, voxel=self.VOXEL, dim=self.DIM,
                                trunc=self.TRUNC)
        self.mesh = TR.mesh(self.vol["tsdf"], self.vol["weight"], None, origin=self.ORIGIN, voxel=self.VOXEL,
                            dim=self.DIM)


@pytest.fixture(scope="module")
def sphere():
    return SphereCase()


@pytest.fixture(scope="module")
def plane():
    return PlaneCase()


def directed_edges(tris):
    t = tris.astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def test_premises(sphere, plane):
    """checked on the reference's output before anything else: the cases exercise
    the truncation, the occlusion, partial weights and both triangle counts"""
    for case in (sphere, plane):
        st, K = case.vol["stats"], len(case.depth)
        w = case.vol["weight"]
        assert st["near_voxels"] > 0 and st["observed_voxels"] < st["voxels"]
        assert ((w > 0) & (w < K)).any()
        occluded, counted = np.array(case.vol["occluded"]), np.array(case.vol["counted"])
        assert (occluded.any(axis=0) & counted.any(axis=0)).any()
        per_tet = case.mesh["tet_triangles"]
        assert (per_tet == 1).any() and (per_tet == 2).any()
        assert len(case.mesh["triangles"]) == per_tet.sum() > 0
    # the sphere: everything outside it is observed, and what is not observed is deeper than trunc less a
    # voxel diagonal (the depth is sampled at the nearest pixel, not on the voxel's own ray)
    x, y, z = TR.voxel_centres(sphere.ORIGIN, sphere.VOXEL, sphere.DIM)
    dist = np.sqrt((x[None, None, :] - sphere.CENTRE[0]) ** 2 + (y[None, :, None] - sphere.CENTRE[1]) ** 2 +
                   (z[:, None, None] - sphere.CENTRE[2]) ** 2)
    w = sphere.vol["weight"]
    assert (w[dist > sphere.R] > 0).all()
    assert (dist[w == 0] < sphere.R - sphere.TRUNC + np.sqrt(3) * sphere.VOXEL).all()
    assert (sphere.vol["tsdf"][w == 0] == 1.0).all() and (sphere.vol["rgb"][w == 0] == 0).all()
    # the plane: the lowest layer is occluded in every view
    assert (plane.vol["weight"][0] == 0).all() and (plane.vol["weight"][2:] == 4).any()


def test_sphere_mesh_is_closed_oriented_and_on_the_sphere(sphere):
    verts, tris = sphere.mesh["vertices"], sphere.mesh["triangles"]
    assert tris.min() == 0 and tris.max() == len(verts) - 1
    # closed: every undirected edge is in exactly two triangles, once in each direction
    e = directed_edges(tris)
    keys = e[:, 0] * len(verts) + e[:, 1]
    assert len(np.unique(keys)) == len(keys)
    assert np.array_equal(np.sort(keys), np.sort(e[:, 1] * len(verts) + e[:, 0]))
    n_edges = len(keys) // 2
    assert len(verts) - n_edges + len(tris) == 2
    # the winding: every triangle of non-zero area faces away from the centre
    p = verts["pos"].astype(np.float64)
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    normal = np.cross(b - a, c - a)
    area2 = np.linalg.norm(normal, axis=1)
    out = (normal * ((a + b + c) / 3.0 - sphere.CENTRE)).sum(axis=1)
    assert (area2 > 0).sum() > 0.99 * len(tris) and (out[area2 > 0] > 0).all()
    # every vertex within one voxel diagonal of the sphere
    err = np.abs(np.linalg.norm(p - sphere.CENTRE, axis=1) - sphere.R)
    assert err.max() <= np.sqrt(3.0) * sphere.VOXEL, err.max() / sphere.VOXEL
    # colours are blends of the observed voxels' colours, which are means of random texels
    assert len({tuple(c) for c in verts["rgb"].tolist()}) > 100 and (verts["pad"] == 0).all()


def test_plane_mesh_lies_on_the_plane(plane):
    verts, tris = plane.mesh["vertices"], plane.mesh["triangles"]
    assert len(tris) > 2 * 20 * 20
    assert np.abs(verts["pos"][:, 2]).max() <= plane.VOXEL
    # an open sheet: its boundary edges are in one triangle only, no edge is in more than two
    e = directed_edges(tris)
    und = np.sort(e, axis=1)
    _, counts = np.unique(und[:, 0] * len(verts) + und[:, 1], return_counts=True)
    assert set(counts.tolist()) == {1, 2}
    # facing the cameras, which are on the +z side
    p = verts["pos"].astype(np.float64)
    normal = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])
    assert (normal[:, 2][np.linalg.norm(normal, axis=1) > 0] > 0).all()


def test_vertex_and_triangle_order(sphere):
    """vertices ascend in (k, j, i, dir), recovered from the flags; triangles in (cell, tetrahedron)"""
    flags = sphere.mesh["flags"].reshape(-1)
    assert TR.popcount8(flags).sum() == len(sphere.mesh["vertices"])
    # a vertex of an axis edge lies on that edge: its two other coordinates are the lattice point's
    xs = TR.voxel_centres(sphere.ORIGIN, sphere.VOXEL, sphere.DIM)
    L = np.flatnonzero(flags)[0]
    first = sphere.mesh["vertices"][0]["pos"]
    nx, ny, _ = sphere.DIM
    lattice = np.array([xs[0][L % nx], xs[1][(L // nx) % ny], xs[2][L // (nx * ny)]])
    assert (np.abs(first - lattice) <= sphere.VOXEL * 1.0001).all() and (first >= lattice.astype(np.float32)).all()
    # min_weight deactivates cells: fewer triangles, and a boundary appears
    cut = TR.mesh(sphere.vol["tsdf"], sphere.vol["weight"], None, origin=sphere.ORIGIN, voxel=sphere.VOXEL,
                  dim=sphere.DIM, min_weight=6)
    assert 0 < cut["stats"]["triangles"] < sphere.mesh["stats"]["triangles"]
    assert cut["stats"]["active_cells"] < sphere.mesh["stats"]["active_cells"]
    assert (cut["vertices"]["rgb"] == 0).all()


def parse_ply(path):
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    head = lines[:end]
    assert head[:2] == ["ply", "format ascii 1.0"]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in head if h.startswith("element face")][0].split()[2])
    props = [h.split()[1:] for h in head if h.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"],
                     ["uchar", "blue"], ["list", "uchar", "int", "vertex_indices"]]
    body = lines[end + 1:]
    assert body[-1] == "" and len(body) == nv + nf + 1
    v = np.array([ln.split() for ln in body[:nv]], dtype=np.float64).reshape(nv, 6)
    f = np.array([ln.split() for ln in body[nv:nv + nf]], dtype=np.int64).reshape(nf, 4)
    return v, f


def test_write_mesh_ply_round_trips(sphere, tmp_path):
    verts, tris = sphere.mesh["vertices"].astype(MESH_VERTEX_DTYPE), sphere.mesh["triangles"]
    path = str(tmp_path / "mesh.ply")
    dp.write_mesh_ply(path, verts, tris)
    v, f = parse_ply(path)
    assert np.array_equal(v[:, :3].astype(np.float32), verts["pos"]) and np.array_equal(v[:, 3:], verts["rgb"])
    assert (f[:, 0] == 3).all() and np.array_equal(f[:, 1:], tris)
    dp.write_mesh_ply(path, verts[:0], tris[:0])
    v, f = parse_ply(path)
    assert len(v) == 0 and len(f) == 0


def test_header_declares_and_native_binds_the_tsdf_calls():
    txt = open(os.path.join(ROOT, "include", "densepoints.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, txt), f"{sym} not declared"
        assert sym in bound and hasattr(N.lib, sym)
    assert [len(bound[s]) for s in NEW] == [1, 9, 10, 10, 13]
    for struct, cls in (("dp_tsdf_options", DpTsdfOptions), ("dp_tsdf_stats", DpTsdfStats),
                        ("dp_mesh_stats", DpMeshStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S)
        assert re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", m.group(1)) == [name for name, _ in cls._fields_]
    m = re.search(r"typedef struct dp_mesh_vertex \{(.*?)\} dp_mesh_vertex;", txt, flags=re.S)
    assert re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", m.group(1)) == list(MESH_VERTEX_DTYPE.names)
    assert ctypes.sizeof(DpTsdfOptions) == 40 and ctypes.sizeof(DpTsdfStats) == 40 and ctypes.sizeof(DpMeshStats) == 32
    assert MESH_VERTEX_DTYPE.itemsize == 16 and MESH_VERTEX_DTYPE == TR.VERTEX and dp.MESH_VERTEX_DTYPE is MESH_VERTEX_DTYPE
    assert re.search(r"#define DP_ABI_VERSION 2\b", txt)
    to = DpTsdfOptions((ctypes.c_float * 3)(1, 2, 3), 4.0, (ctypes.c_int32 * 3)(5, 6, 7), 8.0, 9, 10)
    N.lib.dp_default_tsdf_options(ctypes.byref(to))
    assert (list(to.origin), to.voxel, list(to.dim), to.trunc, to.min_weight, to.flags) == ([0, 0, 0], 0, [0, 0, 0], 0, 1, 0)


GOOD = dict(views=None, origin=(0.0, 0.0, 0.0), voxel=0.1, dim=(4, 5, 6), trunc=0.3, min_weight=1)


def test_check_tsdf_args_accepts_and_fills_the_struct():
    to, vid = dp.check_tsdf_args(6, **dict(GOOD, views=[4, 1], origin=(1, -2, 0.5), min_weight=64))
    assert vid.dtype == np.int32 and vid.tolist() == [4, 1]
    assert (list(to.origin), list(to.dim), to.min_weight, to.flags) == ([1.0, -2.0, 0.5], [4, 5, 6], 64, 0)
    assert (to.voxel, to.trunc) == (np.float32(0.1), np.float32(0.3))
    assert dp.check_tsdf_args(3, **GOOD)[1].tolist() == [0, 1, 2]
    dp.check_tsdf_args(1, **dict(GOOD, dim=(1024, 1024, 1024)))
    dp.check_tsdf_args(1, **dict(GOOD, dim=(2, 2, 2)))


@pytest.mark.parametrize("bad", [
    dict(origin=(0, 0)), dict(origin=(0, np.nan, 0)), dict(origin=(0, 0, np.inf)), dict(origin=None),
    dict(voxel=0), dict(voxel=-1.0), dict(voxel=np.nan), dict(voxel=np.inf), dict(voxel=1e39), dict(voxel="1"),
    dict(trunc=0), dict(trunc=-0.1), dict(trunc=np.nan), dict(trunc=np.inf), dict(trunc=1e-60),
    dict(dim=(4, 5)), dict(dim=(1, 5, 6)), dict(dim=(4, 1025, 6)), dict(dim=(4.5, 5, 6)), dict(dim=8),
    dict(min_weight=0), dict(min_weight=65), dict(min_weight=1.5), dict(min_weight=True),
    dict(views=[]), dict(views=[0, 0]), dict(views=[3]), dict(views=[-1]), dict(views=list(range(65))),
], ids=lambda b: "-".join("%s=%s" % i for i in b.items())[:40])
def test_check_tsdf_args_rejects(bad):
    with pytest.raises(ValueError):
        dp.check_tsdf_args(70 if bad.get("views") and len(bad["views"]) > 64 else 3, **dict(GOOD, **bad))


def test_mesh_volume_bounds_the_patches():
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [np.nan, 0, 0]])
    vol = pmvs.mesh_volume(pos, dim=10)
    assert vol["voxel"] == pytest.approx(0.1) and vol["trunc"] == pytest.approx(0.4)
    assert vol["origin"] == pytest.approx((-0.4, -0.4, -0.4)) and vol["dim"] in ((18, 13, 11), (19, 14, 11), (18, 13, 10))
    hi = np.array(vol["origin"]) + np.array(vol["dim"]) * vol["voxel"]
    assert (hi >= np.array([1.0, 0.5, 0.25]) + vol["trunc"] - 1e-9).all()
    vol = pmvs.mesh_volume(pos, voxel=0.05, dim=10, trunc=0.1)
    assert (vol["voxel"], vol["trunc"]) == (0.05, 0.1) and vol["dim"][0] in (24, 25)
    assert max(pmvs.mesh_volume(pos, voxel=1e-4)["dim"]) == 1024
    for kw in (dict(dim=1), dict(dim=1025), dict(voxel=-1.0), dict(trunc=0.0)):
        with pytest.raises(ValueError):
            pmvs.mesh_volume(pos, **kw)
    with pytest.raises(ValueError):
        pmvs.mesh_volume(pos[:1])      # one point: no extent
    with pytest.raises(ValueError):
        pmvs.mesh_volume(pos[2:])      # nothing finite


def test_pmvs_mesh_needs_a_run():
    with pytest.raises(ValueError):
        dp.PMVS().mesh()
