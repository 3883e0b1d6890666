"""CPU reference of dp_mesh_adjacency / dp_mesh_smooth / dp_mesh_normals,
restated in numpy from the spec in include/densepoints.h: sets and integer
counts for the adjacency, plain Python loops for the ordered fp64 sums (numpy's
own sums are pairwise: not the spec's order).  Also the meshes the CPU and the
GPU tests share."""
import numpy as np

from mesh_ref import VERTEX_DTYPE, as_triangles, random_vertices  # noqa: F401

ADJ_COUNTS = ("vertices_in", "triangles_in", "invalid_triangles", "degenerate_triangles", "isolated_vertices", "edges",
              "boundary_edges", "nonmanifold_edges", "boundary_vertices", "max_valence")
SMOOTH_COUNTS = ADJ_COUNTS + ("movable_vertices", "pinned_vertices", "steps")
NORMAL_COUNTS = ("vertices_in", "triangles_in", "invalid_triangles", "degenerate_triangles", "zero_normals")
BOUNDARY, NONMANIFOLD = 1, 2


def classes(triangles, n_vertices):
    """(valid, degenerate, proper) per triangle"""
    tris = as_triangles(triangles)
    valid = ((tris >= 0) & (tris < int(n_vertices))).all(axis=1)
    same = (tris[:, 0] == tris[:, 1]) | (tris[:, 1] == tris[:, 2]) | (tris[:, 0] == tris[:, 2])
    return valid, valid & same, valid & ~same


def adjacency(triangles, n_vertices):
    """dict(offsets, neighbours, edge_triangles, vertex_flags, stats)"""
    tris, nv = as_triangles(triangles), int(n_vertices)
    valid, degenerate, proper = classes(tris, nv)
    count = [dict() for _ in range(nv)]  # count[u][v] = the proper triangles that name u and v
    for a, b, c in tris[proper].tolist():
        for u, v in ((a, b), (a, c), (b, a), (b, c), (c, a), (c, b)):
            count[u][v] = count[u].get(v, 0) + 1
    off = np.zeros(nv + 1, np.int32)
    nbr, cnt = [], []
    flags = np.zeros(nv, np.uint8)
    for v in range(nv):
        row = sorted(count[v])
        nbr += row
        cnt += [count[v][w] for w in row]
        off[v + 1] = len(nbr)
        flags[v] = (BOUNDARY if any(count[v][w] == 1 for w in row) else 0) | \
                   (NONMANIFOLD if any(count[v][w] > 2 for w in row) else 0)
    nbr, cnt = np.array(nbr, np.int32).reshape(-1), np.array(cnt, np.int32).reshape(-1)
    rows = np.diff(off.astype(np.int64))
    stats = dict(vertices_in=nv, triangles_in=len(tris), invalid_triangles=int((~valid).sum()),
                 degenerate_triangles=int(degenerate.sum()), isolated_vertices=int((rows == 0).sum()),
                 edges=len(nbr) // 2, boundary_edges=int((cnt == 1).sum()) // 2,
                 nonmanifold_edges=int((cnt > 2).sum()) // 2, boundary_vertices=int((flags & BOUNDARY != 0).sum()),
                 max_valence=int(rows.max()) if nv else 0)
    return dict(offsets=off, neighbours=nbr, edge_triangles=cnt, vertex_flags=flags, stats=stats)


def step(pos, adj, f, pin):
    """one STEP with factor f (a float32 option widened to fp64) of the float32 positions"""
    off, nbr, flags = adj["offsets"], adj["neighbours"], adj["vertex_flags"]
    f = np.float64(np.float32(f))
    new = pos.copy()
    p64 = pos.astype(np.float64)
    for v in range(len(pos)):
        lo, hi = int(off[v]), int(off[v + 1])
        if hi == lo or (pin and flags[v] & BOUNDARY):
            continue
        for c in range(3):
            S = np.float64(0.0)
            for j in nbr[lo:hi]:
                S = S + p64[j, c]
            m = S / np.float64(hi - lo)
            x = p64[v, c]
            new[v, c] = np.float32(x + f * (m - x))
    return new


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, free_boundary=False):
    """dict(vertices, stats)"""
    verts, tris = np.asarray(vertices, dtype=VERTEX_DTYPE).reshape(-1).copy(), as_triangles(triangles)
    adj = adjacency(tris, len(verts))
    pos = np.ascontiguousarray(verts["pos"], np.float32).reshape(-1, 3)
    steps = 0
    for _ in range(int(iterations)):
        pos = step(pos, adj, lam, not free_boundary)
        steps += 1
        if np.float32(mu) != 0:
            pos = step(pos, adj, mu, not free_boundary)
            steps += 1
    verts["pos"] = pos
    st = adj["stats"]
    pinned = 0 if free_boundary else st["boundary_vertices"]
    stats = dict(st, pinned_vertices=pinned, movable_vertices=st["vertices_in"] - st["isolated_vertices"] - pinned,
                 steps=steps)
    return dict(vertices=verts, stats=stats)


def normals(vertices, triangles):
    """dict(normals (n x 3 float32), stats)"""
    verts, tris = np.asarray(vertices, dtype=VERTEX_DTYPE).reshape(-1), as_triangles(triangles)
    nv = len(verts)
    valid, degenerate, proper = classes(tris, nv)
    p = verts["pos"].astype(np.float64).reshape(-1, 3)
    s = np.zeros((nv, 3), np.float64)
    for t in np.flatnonzero(proper):  # ascending triangle index
        i0, i1, i2 = (int(i) for i in tris[t])
        e1, e2 = p[i1] - p[i0], p[i2] - p[i0]
        g = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        for v in (i0, i1, i2):
            for c in range(3):
                s[v, c] = s[v, c] + g[c]
    out = np.zeros((nv, 3), np.float32)
    zero = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for v in range(nv):
            l2 = (s[v, 0] * s[v, 0] + s[v, 1] * s[v, 1]) + s[v, 2] * s[v, 2]
            if not (l2 > 0) or not np.isfinite(l2):
                zero += 1
                continue
            length = np.sqrt(l2)
            out[v] = [np.float32(s[v, c] / length) for c in range(3)]
    stats = dict(vertices_in=nv, triangles_in=len(tris), invalid_triangles=int((~valid).sum()),
                 degenerate_triangles=int(degenerate.sum()), zero_normals=zero)
    return dict(normals=out, stats=stats)


# ---- measures of the orderings the CPU test claims ---------------------------------

def roughness(pos, adj):
    """the mean squared umbrella length: |mean of the neighbours - v|^2 over the non-empty rows"""
    off, nbr = adj["offsets"], adj["neighbours"]
    p = np.asarray(pos, np.float64)
    total, rows = 0.0, 0
    for v in range(len(p)):
        lo, hi = int(off[v]), int(off[v + 1])
        if hi > lo:
            d = p[nbr[lo:hi]].mean(axis=0) - p[v]
            total += float(d @ d)
            rows += 1
    return total / rows


def volume(pos, triangles):
    """the signed volume a closed mesh encloses"""
    p, t = np.asarray(pos, np.float64), as_triangles(triangles)
    return float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0)


# ---- meshes ------------------------------------------------------------------------

def fan(n):
    """a centre (vertex 0) with n rim vertices and n - 1 triangles: the centre's row is n long"""
    return np.array([(0, 1 + i, 2 + i) for i in range(n - 1)], np.int32), n + 1


def grid_sheet(n):
    """an n x n grid of vertices, two triangles per cell: an open sheet"""
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return tris, n * n


def grid_vertices(n, seed, noise=0.2):
    rng = np.random.default_rng(seed)
    v = random_vertices(n * n, seed)
    y, x = np.mgrid[0:n, 0:n]
    pos = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1) + noise * rng.standard_normal((n * n, 3))
    v["pos"] = pos.astype(np.float32)
    return v


def strip(nv):
    """a triangle strip over nv vertices: nv - 2 triangles"""
    i = np.arange(nv - 2, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], 1).astype(np.int32), nv


def sphere_volume(dim=16, radius=0.3, centre=(0.013, -0.021, 0.008)):
    """an analytic TSDF of a sphere off the lattice in a dim^3 volume around the
    origin (every voxel observed once): a volume as Engine.tsdf_mesh reads it,
    and the centre"""
    voxel = 0.8 / dim
    trunc = 4 * voxel
    x = -0.4 + voxel * np.arange(dim)
    dist = np.sqrt((x[None, None, :] - centre[0]) ** 2 + (x[None, :, None] - centre[1]) ** 2 +
                   (x[:, None, None] - centre[2]) ** 2)
    tsdf = np.clip((dist - radius) / trunc, -1.0, 1.0).astype(np.float32)
    return dict(tsdf=tsdf, weight=np.ones((dim,) * 3, np.int32), origin=(-0.4, -0.4, -0.4), voxel=voxel,
                dim=(dim, dim, dim), trunc=trunc), np.array(centre)


def noisy(vertices, sigma, seed):
    """the records with Gaussian noise of standard deviation sigma on the positions"""
    v = np.asarray(vertices, dtype=VERTEX_DTYPE).copy()
    rng = np.random.default_rng(seed)
    v["pos"] = (v["pos"].astype(np.float64) + sigma * rng.standard_normal(v["pos"].shape)).astype(np.float32)
    return v
