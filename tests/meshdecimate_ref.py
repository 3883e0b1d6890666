"""CPU reference of dp_mesh_decimate, restated from the spec in
include/densepoints.h: dictionaries and sorted lists for the clusters, a set for
the duplicate triples, scalar float64 operations in the stated order for the
mean and the quadric (no np.linalg, no np.cross, no vectorised sum).  Also the
meshes the CPU and the GPU tests share."""
import numpy as np

from mesh_ref import VERTEX_DTYPE, as_triangles, random_vertices  # noqa: F401
from meshsmooth_ref import classes

COUNTS = ("vertices_in", "triangles_in", "invalid_triangles", "degenerate_triangles", "unused_vertices",
          "clamped_vertices", "clusters", "orphan_clusters", "max_cluster", "collapsed_triangles",
          "duplicate_triangles", "quadric_vertices", "mean_vertices", "vertices_out", "triangles_out")
DET_EPS = np.float64(1e-6)
K_LO, K_HI = -2**20, 2**20 - 1
F64 = np.float64


def cell_of(p, origin, cell):
    """((k_z, k_y, k_x), clamped) of the float32 position p: the cells' order is the tuples' order"""
    k, clamped = [0, 0, 0], False
    with np.errstate(all="ignore"):
        for c in range(3):
            q = np.floor((F64(p[c]) - origin[c]) / cell)
            if not (q >= K_LO):
                k[c], clamped = K_LO, True
            elif q > K_HI:
                k[c], clamped = K_HI, True
            else:
                k[c] = int(q)
    return (k[2], k[1], k[0]), clamped


def quadric_offset(tri_list, tris, pos, m):
    """the nine sums over the triangles of tri_list (ascending) around m, the
    solvability test and the offset x; None when the cluster is not solvable"""
    Axx = Axy = Axz = Ayy = Ayz = Azz = bx = by = bz = F64(0.0)
    for t in tri_list:
        i0, i1, i2 = (int(i) for i in tris[t])
        p0, p1, p2 = ([F64(x) for x in pos[i]] for i in (i0, i1, i2))
        e1 = [p1[c] - p0[c] for c in range(3)]
        e2 = [p2[c] - p0[c] for c in range(3)]
        g = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        r = [p0[c] - m[c] for c in range(3)]
        d = (g[0] * r[0] + g[1] * r[1]) + g[2] * r[2]
        Axx = Axx + g[0] * g[0]
        Axy = Axy + g[0] * g[1]
        Axz = Axz + g[0] * g[2]
        Ayy = Ayy + g[1] * g[1]
        Ayz = Ayz + g[1] * g[2]
        Azz = Azz + g[2] * g[2]
        bx = bx + d * g[0]
        by = by + d * g[1]
        bz = bz + d * g[2]
    c00 = Ayy * Azz - Ayz * Ayz
    c01 = Axz * Ayz - Axy * Azz
    c02 = Axy * Ayz - Axz * Ayy
    c11 = Axx * Azz - Axz * Axz
    c12 = Axy * Axz - Axx * Ayz
    c22 = Axx * Ayy - Axy * Axy
    det = (Axx * c00 + Axy * c01) + Axz * c02
    t = ((Axx + Ayy) + Azz) / F64(3.0)
    if not (np.isfinite(det) and det > DET_EPS * ((t * t) * t)):
        return None
    return (((c00 * bx + c01 * by) + c02 * bz) / det, ((c01 * bx + c11 * by) + c12 * bz) / det,
            ((c02 * bx + c12 * by) + c22 * bz) / det)


def decimate(verts, tris, cell, origin=(0.0, 0.0, 0.0), quadric=False):
    """dict(vertices, triangles, vertex_map, triangle_map, stats, placement): the
    outputs of dp_mesh_decimate; placement holds, per output vertex, "quadric",
    "unsolvable" or "outside" (the last two are the mean)"""
    verts, tris = np.asarray(verts, dtype=VERTEX_DTYPE).reshape(-1), as_triangles(tris)
    nv, nt = len(verts), len(tris)
    valid, degenerate, proper = classes(tris, nv)
    cell = F64(np.float32(cell))
    origin = [F64(np.float32(o)) for o in origin]
    pos = np.ascontiguousarray(verts["pos"], np.float32).reshape(-1, 3)
    used = np.zeros(nv, bool)
    used[tris[proper].ravel()] = True
    # clusters: the used vertices of one cell, ascending; numbered by ascending cell
    members, clamped_vertices = {}, 0
    for v in np.flatnonzero(used).tolist():
        k, clamped = cell_of(pos[v], origin, cell)
        clamped_vertices += int(clamped)
        members.setdefault(k, []).append(v)
    cells = sorted(members)
    K = len(cells)
    cluster = np.full(nv, -1, np.int64)
    for c, k in enumerate(cells):
        cluster[members[k]] = c
    # triangles: collapsed, duplicate or kept; the triangles of every cluster
    kept, seen, collapsed, duplicate = [], set(), 0, 0
    named = [[] for _ in range(K)]
    survives = np.zeros(K, bool)
    for t in np.flatnonzero(proper).tolist():
        A, B, C = (int(cluster[i]) for i in tris[t])
        for c in dict.fromkeys((A, B, C)):  # once per cluster
            named[c].append(t)
        if A == B or B == C or A == C:
            collapsed += 1
            continue
        canon = min((A, B, C), (B, C, A), (C, A, B))
        if canon in seen:
            duplicate += 1
            continue
        seen.add(canon)
        kept.append(t)
        survives[[A, B, C]] = True
    number = np.where(survives, np.cumsum(survives) - 1, -1)
    vmap = np.full(nv, -1, np.int32)
    vmap[used] = number[cluster[used]]
    tmap = np.full(nt, -1, np.int32)
    tmap[kept] = np.arange(len(kept))
    tout = number[cluster[tris[kept]]].astype(np.int32).reshape(-1, 3)
    # the records of the surviving clusters
    out = np.zeros(int(survives.sum()), VERTEX_DTYPE)
    placement = []
    with np.errstate(all="ignore"):
        for c in np.flatnonzero(survives).tolist():
            mem = members[cells[c]]
            n = len(mem)
            m = []
            for a in range(3):
                S = F64(0.0)
                for v in mem:
                    S = S + F64(pos[v, a])
                m.append(S / F64(n))
            rec = out[number[c]]
            for ch in range(3):
                R = sum(int(verts["rgb"][v, ch]) for v in mem)
                rec["rgb"][ch] = (2 * R + n) // (2 * n)
            how, p = "unsolvable", [np.float32(m[a]) for a in range(3)]
            if quadric:
                x = quadric_offset(named[c], tris, pos, m)
                if x is not None:
                    cand = [np.float32(m[a] + x[a]) for a in range(3)]
                    if all(np.isfinite(q) for q in cand) and cell_of(cand, origin, cell)[0] == cells[c]:
                        how, p = "quadric", cand
                    else:
                        how = "outside"
            rec["pos"] = p
            placement.append(how if quadric else "mean")
    nq = placement.count("quadric")
    stats = dict(vertices_in=nv, triangles_in=nt, invalid_triangles=int((~valid).sum()),
                 degenerate_triangles=int(degenerate.sum()), unused_vertices=int((~used).sum()),
                 clamped_vertices=clamped_vertices, clusters=K, orphan_clusters=int((~survives).sum()),
                 max_cluster=max((len(members[k]) for k in cells), default=0), collapsed_triangles=collapsed,
                 duplicate_triangles=duplicate, quadric_vertices=nq, mean_vertices=len(out) - nq,
                 vertices_out=len(out), triangles_out=len(kept))
    return dict(vertices=out, triangles=tout, vertex_map=vmap, triangle_map=tmap, stats=stats, placement=placement)


# ---- meshes ------------------------------------------------------------------------

def colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)


def uv_sphere(stacks=24, slices=48, radius=1.0, seed=1):
    """a UV sphere: (stacks + 1) rows of `slices` vertices (the seam column is
    shared; a pole row is `slices` vertices at one point), two triangles per quad,
    wound outwards.  Returns (vertices, triangles)."""
    i, j = np.mgrid[0:stacks + 1, 0:slices]
    theta, phi = np.pi * i / stacks, 2.0 * np.pi * j / slices
    verts = np.zeros((stacks + 1) * slices, VERTEX_DTYPE)
    verts["pos"] = (radius * np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)],
                                      -1)).reshape(-1, 3).astype(np.float32)
    verts["rgb"] = colours(len(verts), seed)
    idx = np.arange((stacks + 1) * slices).reshape(stacks + 1, slices)
    a, b = idx[:-1], np.roll(idx[:-1], -1, axis=1)
    c, d = idx[1:], np.roll(idx[1:], -1, axis=1)
    tris = np.stack([np.stack([a, c, b], -1), np.stack([b, c, d], -1)], 2).reshape(-1, 3)
    return verts, np.ascontiguousarray(tris, np.int32)


def cube(n=8, seed=2):
    """the surface of [0, 1]^3 with n x n quads per face, the vertices of the
    faces' common edges shared, two triangles per quad, wound outwards.  Returns
    (vertices, triangles)."""
    index, pts, tris = {}, [], []

    def vertex(p):
        if p not in index:
            index[p] = len(pts)
            pts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for s in range(n):
                for t in range(n):
                    quad = []
                    for ds, dt in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, s + ds, t + dt
                        quad.append(vertex(tuple(p)))
                    if side == 0:  # u x w is +axis: the low face looks the other way
                        quad.reverse()
                    tris += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    verts = np.zeros(len(pts), VERTEX_DTYPE)
    verts["pos"] = (np.array(pts, np.float64) / n).astype(np.float32)
    verts["rgb"] = colours(len(verts), seed)
    return verts, np.array(tris, np.int32)


PLANTED = dict(cell=1.0, origin=(0.0, 0.0, 0.0))


def planted_mesh():
    """What the sphere and the cube lack, at cell 1, origin 0.  Vertices 0-2 and
    3-5: two triangles on different vertices in the same three cells, same winding
    (the second is a duplicate); 6-8 in those cells again, wound the other way
    (kept); 9-11: a tiny triangle inside an otherwise empty cell (collapsed, an
    orphan cluster); an invalid and a degenerate triangle; vertex 12 unused; 13
    beyond 2^20 cells (clamped) and 14 at a negative coordinate (floor, not
    truncation: cell -1), both named by one more triangle with vertex 0."""
    p = [(0.2, 0.2, 0.2), (1.3, 0.1, 0.4), (0.3, 1.6, 0.2),
         (0.7, 0.6, 0.1), (1.8, 0.7, 0.3), (0.1, 1.2, 0.9),
         (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5),
         (5.1, 5.1, 5.1), (5.2, 5.1, 5.1), (5.1, 5.2, 5.1),
         (3.5, 3.5, 3.5), (3.0e6, 0.5, 0.5), (-0.5, 0.5, 0.5)]
    tris = [(0, 1, 2), (4, 5, 3), (6, 8, 7), (9, 10, 11), (0, 1, 15), (-1, 1, 2), (2, 2, 1), (0, 13, 14)]
    verts = np.zeros(len(p), VERTEX_DTYPE)
    verts["pos"] = np.array(p, np.float32)
    verts["rgb"] = colours(len(p), 3)
    return verts, np.array(tris, np.int32)
