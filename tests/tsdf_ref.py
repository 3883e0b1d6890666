"""CPU reference of dp_tsdf_integrate and dp_tsdf_mesh, restated from the spec
text in include/densepoints.h (not from the kernels): fp64 in the header's
order, numpy evaluating the voxels (cells, edges) elementwise, each with the
same single-rounding operations."""
import itertools
import math

import numpy as np

from fuse_ref import Views, dot, is_depth, row, same_bytes  # noqa: F401  (the shared pieces of the spec)

# dp_mesh_vertex as the header lays it out
VERTEX = np.dtype([("pos", "<f4", 3), ("rgb", "u1", 3), ("pad", "u1")])
assert VERTEX.itemsize == 16

# the seven edge directions in the header's order, and their index by the bits dx | dy << 1 | dz << 2
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
DIR_OF_BITS = {d[0] | d[1] << 1 | d[2] << 2: n for n, d in enumerate(DIRS)}
# the six tetrahedra of a cell: the permutations of the axes in lexicographic order
PERMS = list(itertools.permutations(range(3)))
# the header's triangle table of an EVEN tetrahedron: inside mask -> triangles,
# each three edges named by their two corner numbers
TABLE = {
    1: ["01 02 03"], 2: ["01 13 12"], 3: ["02 03 13", "02 13 12"], 4: ["02 12 23"],
    5: ["01 23 03", "01 12 23"], 6: ["01 13 23", "01 23 02"], 7: ["03 13 23"], 8: ["03 23 13"],
    9: ["01 02 23", "01 23 13"], 10: ["01 23 12", "01 03 23"], 11: ["02 23 12"],
    12: ["02 12 13", "02 13 03"], 13: ["01 12 13"], 14: ["01 03 02"],
}
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def perm_is_odd(p):
    return sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2 == 1


def tet_corners(p):
    """the four corner offsets (x, y, z) of tetrahedron (a, b, c)"""
    q = [[0, 0, 0]]
    for axis in p:
        nxt = list(q[-1])
        nxt[axis] += 1
        q.append(nxt)
    return q


def view_scale(vw, v):
    """g_v of the spec"""
    m2 = vw.P[v][2][:3]
    return math.sqrt(dot(m2, m2))


def voxel_centres(origin, voxel, dim):
    """X (three fp64 arrays broadcastable to [nz][ny][nx]) of the voxel centres"""
    o, s = [np.float64(np.float32(c)) for c in origin], np.float64(np.float32(voxel))
    nx, ny, nz = dim
    x = o[0] + (np.arange(nx, dtype=np.float64) + 0.5) * s
    y = o[1] + (np.arange(ny, dtype=np.float64) + 0.5) * s
    z = o[2] + (np.arange(nz, dtype=np.float64) + 0.5) * s
    return x, y, z


def integrate(vw, depth, views=None, *, origin, voxel, dim, trunc):
    """{"tsdf" f32, "weight" int32, "rgb" uint32 ([nz][ny][nx]), "counted" (per
    requested view a bool volume: the view counted), "occluded" (the same: the view
    reached step 5 and was rejected there), "stats"}"""
    views = list(range(vw.V)) if views is None else [int(v) for v in views]
    assert 1 <= len(views) <= 64 and len(depth) == len(views)
    nx, ny, nz = [int(d) for d in dim]
    x, y, z = voxel_centres(origin, voxel, dim)
    shape = (nz, ny, nx)
    X = [np.broadcast_to(x[None, None, :], shape), np.broadcast_to(y[None, :, None], shape),
         np.broadcast_to(z[:, None, None], shape)]
    tr = np.float64(np.float32(trunc))
    tsum = np.zeros(shape, np.float64)
    w = np.zeros(shape, np.int64)
    s = [np.zeros(shape, np.int64) for _ in range(3)]
    counted, occluded = [], []
    for k, v in enumerate(views):
        P, g = vw.P[v], view_scale(vw, v)
        assert g > 0 and math.isfinite(g)
        zp = np.ascontiguousarray(depth[k], np.float32)
        assert zp.shape == (vw.H[v], vw.W[v])
        with np.errstate(all="ignore"):
            d = row(P, 2, X)
            ok = d > 0.0
            uu = row(P, 0, X) / d
            vv = row(P, 1, X) / d
            ok &= (np.abs(uu) < 2e9) & (np.abs(vv) < 2e9)
            xi = np.where(ok, np.rint(uu), -1.0).astype(np.int64)
            yi = np.where(ok, np.rint(vv), -1.0).astype(np.int64)
            ok &= (xi >= 0) & (xi < vw.W[v]) & (yi >= 0) & (yi < vw.H[v])
            xi, yi = np.where(ok, xi, 0), np.where(ok, yi, 0)
            zs = zp[yi, xi]
            ok &= is_depth(zs)
            sdf = (zs.astype(np.float64) - d) / g
            occ = ok & (sdf < -tr)
            cnt = ok & ~occ
            t = np.where(sdf >= tr, 1.0, sdf / tr)
            tsum = np.where(cnt, tsum + t, tsum)
        w += cnt
        if vw.images is not None:
            texel = vw.images[v][yi, xi].astype(np.int64)  # B, G, R
            for c in range(3):
                s[c] += np.where(cnt, texel[..., 2 - c], 0)
        counted.append(cnt)
        occluded.append(occ)
    seen = w > 0
    wd = np.where(seen, w, 1)
    with np.errstate(all="ignore"):
        tsdf = np.where(seen, (tsum / wd.astype(np.float64)).astype(np.float32), np.float32(1.0)).astype(np.float32)
    ch = [np.where(seen, (c + wd // 2) // wd, 0) for c in s]
    rgb = (ch[0] | ch[1] << 8 | ch[2] << 16).astype(np.uint32)
    st = dict(voxels=nx * ny * nz, observations=int(w.sum()), observed_voxels=int(seen.sum()),
              near_voxels=int((seen & (np.abs(tsdf) < np.float32(1.0))).sum()))
    return dict(views=views, tsdf=tsdf, weight=w.astype(np.int32), rgb=rgb, counted=counted, occluded=occluded,
                stats=st, origin=tuple(float(np.float32(c)) for c in origin), voxel=float(np.float32(voxel)),
                dim=(nx, ny, nz), trunc=float(np.float32(trunc)))


def popcount8(a):
    a = a.astype(np.int64)
    return sum((a >> b) & 1 for b in range(8))


def mesh(tsdf, weight, rgb=None, *, origin, voxel, dim, min_weight=1):
    """{"vertices" (VERTEX array), "triangles" (n x 3 int32), "flags" (the 7-bit
    edge flags per lattice point), "tet_triangles" (triangles per tetrahedron, cells
    x 6), "stats"}"""
    nx, ny, nz = [int(d) for d in dim]
    tsdf = np.ascontiguousarray(tsdf, np.float32).reshape(nz, ny, nx)
    weight = np.ascontiguousarray(weight, np.int32).reshape(nz, ny, nx)
    with np.errstate(invalid="ignore"):
        inside = tsdf < np.float32(0)
    good = weight >= int(min_weight)
    cz, cy, cx = nz - 1, ny - 1, nx - 1

    def corner(a, o):
        """a at the cells' corner with offset o = (x, y, z)"""
        return a[o[2]:o[2] + cz, o[1]:o[1] + cy, o[0]:o[0] + cx]

    active = np.ones((cz, cy, cx), bool)
    for o in itertools.product((0, 1), repeat=3):
        active &= corner(good, o)
    flags = np.zeros((nz, ny, nx), np.uint8)
    masks = []
    for p in PERMS:
        q = tet_corners(p)
        m = np.zeros((cz, cy, cx), np.int64)
        for i in range(4):
            m |= corner(inside, q[i]).astype(np.int64) << i
        masks.append(np.where(active, m, 0))
        for lo, hi in TET_EDGES:
            crossing = active & (corner(inside, q[lo]) != corner(inside, q[hi]))
            bits = (q[hi][0] - q[lo][0]) | (q[hi][1] - q[lo][1]) << 1 | (q[hi][2] - q[lo][2]) << 2
            corner(flags, q[lo])[...] |= (crossing.astype(np.uint8) << DIR_OF_BITS[bits]).astype(np.uint8)
    flat = flags.reshape(-1)
    count = popcount8(flat)
    vbase = np.cumsum(count) - count
    # vertices in ascending (k, j, i, dir)
    bit = (flat[:, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1
    L, dr = np.nonzero(bit)
    i0, j0, k0 = L % nx, (L // nx) % ny, L // (nx * ny)
    dv = np.array(DIRS, np.int64)[dr]
    i1, j1, k1 = i0 + dv[:, 0], j0 + dv[:, 1], k0 + dv[:, 2]
    xs = voxel_centres(origin, voxel, dim)
    a = tsdf[k0, j0, i0].astype(np.float64)
    b = tsdf[k1, j1, i1].astype(np.float64)
    verts = np.zeros(len(L), VERTEX)
    with np.errstate(all="ignore"):
        s = a / (a - b)
        for c, (ia, ib) in enumerate(((i0, i1), (j0, j1), (k0, k1))):
            XA, XB = xs[c][ia], xs[c][ib]
            verts["pos"][:, c] = (XA + s * (XB - XA)).astype(np.float32)
        if rgb is not None:
            word = np.ascontiguousarray(rgb, np.uint32).reshape(nz, ny, nx)
            wa, wb = word[k0, j0, i0].astype(np.int64), word[k1, j1, i1].astype(np.int64)
            for c in range(3):
                ca, cb = ((wa >> 8 * c) & 255).astype(np.float64), ((wb >> 8 * c) & 255).astype(np.float64)
                verts["rgb"][:, c] = np.rint(ca + s * (cb - ca)).astype(np.uint8)
    # triangles in ascending cell (k, j, i), tetrahedron, triangle
    kk, jj, ii = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    tri = np.zeros((cz, cy, cx, 6, 2, 3), np.int64)
    valid = np.zeros((cz, cy, cx, 6, 2), bool)
    for t, p in enumerate(PERMS):
        q = tet_corners(p)
        edge_id = {}
        for lo, hi in TET_EDGES:
            Lo = ((kk + q[lo][2]) * ny + (jj + q[lo][1])) * nx + (ii + q[lo][0])
            bits = (q[hi][0] - q[lo][0]) | (q[hi][1] - q[lo][1]) << 1 | (q[hi][2] - q[lo][2]) << 2
            below = (1 << DIR_OF_BITS[bits]) - 1
            edge_id["%d%d" % (lo, hi)] = vbase[Lo] + popcount8(flat[Lo] & below)
        for m, rows in TABLE.items():
            sel = masks[t] == m
            for r, text in enumerate(rows):
                e = text.split()
                if perm_is_odd(p):
                    e = [e[0], e[2], e[1]]
                valid[..., t, r] |= sel
                for c in range(3):
                    tri[..., t, r, c] = np.where(sel, edge_id[e[c]], tri[..., t, r, c])
    triangles = tri[valid].astype(np.int32).reshape(-1, 3)
    st = dict(active_cells=int(active.sum()), vertices=len(verts), triangles=len(triangles))
    return dict(vertices=verts, triangles=triangles, flags=flags, tet_triangles=valid.sum(axis=-1).reshape(-1, 6),
                stats=st)
