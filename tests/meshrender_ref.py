"""CPU reference of dp_mesh_render, restated from the spec text in
include/densepoints.h (not from the kernels): fp64 in the header's order, one
(triangle, view) pair at a time over its box (numpy evaluates the box's pixels
elementwise, each with the same single-rounding operations).  Also the meshes
and cameras the mesh-render tests share."""
import math

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("triangles", "invalid_triangles", "pairs", "clipped_pairs", "culled_pairs", "pixel_tests", "covered_pixels")
VERTEX_DTYPE = np.dtype([("pos", np.float32, 3), ("rgb", np.uint8, 3), ("pad", np.uint8)])
CULL_BACK = 1


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def row(P, r, X):
    return ((P[r][0] * X[0] + P[r][1] * X[1]) + P[r][2] * X[2]) + P[r][3]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Cameras:
    """P (as Python floats), W, H of every view"""

    def __init__(self, P, W, H):
        self.P = [[[float(x) for x in r] for r in np.asarray(Pv, np.float64).reshape(3, 4)] for Pv in P]
        self.W, self.H = [int(w) for w in W], [int(h) for h in H]
        self.V = len(self.P)

    def centre(self, v):
        """the camera centre (numpy; for the tests' geometry, not the spec's)"""
        P = np.array(self.P[v])
        return -np.linalg.solve(P[:, :3], P[:, 3])


def view_det(P):
    p = [x for r in P for x in r]
    return (p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8])) + p[2] * (p[4] * p[9] - p[5] * p[8])


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def make_pair(P, W, H, m, X, cull_back):
    """(result, record): result is "pair", "clipped", "culled" or None; the
    record dict(r, D, front, x0, x1, y0, y1) of a pair"""
    h = [[row(P, r, Xk) for r in range(3)] for Xk in X]
    front = sum(1 for hk in h if hk[2] > 0.0)
    if front < 3:
        return ("clipped" if front > 0 else None), None
    r = [cross(h[(k + 1) % 3], h[(k + 2) % 3]) for k in range(3)]
    D = (h[0][0] * r[0][0] + h[0][1] * r[0][1]) + h[0][2] * r[0][2]
    if not math.isfinite(D) or D == 0.0:
        return None, None
    is_front = (D > 0.0 and m < 0.0) or (D < 0.0 and m > 0.0)
    if cull_back and not is_front:
        return "culled", None
    with np.errstate(all="ignore"):
        u = [float(np.float64(hk[0]) / np.float64(hk[2])) for hk in h]
        w = [float(np.float64(hk[1]) / np.float64(hk[2])) for hk in h]
    if not all(abs(x) < 2.0e9 for x in u + w):
        return None, None
    x0, x1 = max(0, math.floor(min(u))), min(W - 1, math.ceil(max(u)))
    y0, y1 = max(0, math.floor(min(w))), min(H - 1, math.ceil(max(w)))
    if x0 > x1 or y0 > y1:
        return None, None
    return "pair", dict(r=r, D=D, front=is_front, x0=x0, x1=x1, y0=y0, y1=y1)


def face_normal(X):
    e = [X[1][j] - X[0][j] for j in range(3)]
    f = [X[2][j] - X[0][j] for j in range(3)]
    N = cross(e, f)
    s = math.sqrt(dot(N, N))
    if not (math.isfinite(s) and s > 0.0):
        return np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        return np.array([np.float64(c) / np.float64(s) for c in N]).astype(np.float32)


def render(cams, vertices, triangles, views=None, cull_back=False):
    """dict(views, depth, index, normal, stats, pairs): the planes per requested
    view, the integer statistics and the pair records (with triangle and view)"""
    pos = np.asarray(vertices)["pos"] if np.asarray(vertices).dtype.names else np.asarray(vertices, np.float32)
    pos = pos.reshape(-1, 3)
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    nv = len(pos)
    views = list(range(cams.V)) if views is None else [int(v) for v in views]
    ms = [view_det(cams.P[v]) for v in views]
    assert all(math.isfinite(m) and m != 0.0 for m in ms)
    zbuf = [np.full((cams.H[v], cams.W[v]), EMPTY, np.uint64) for v in views]
    st = dict.fromkeys(COUNTS, 0)
    pairs, taking = [], {}
    for t, tri in enumerate(tris):
        if not all(0 <= int(i) < nv for i in tri):
            st["invalid_triangles"] += 1
            continue
        p = pos[tri]
        if not np.isfinite(p).all():
            continue
        st["triangles"] += 1
        X = [[float(c) for c in pk] for pk in p]
        taking[t] = X
        for k, v in enumerate(views):
            res, pr = make_pair(cams.P[v], cams.W[v], cams.H[v], ms[k], X, cull_back)
            if res == "clipped":
                st["clipped_pairs"] += 1
            elif res == "culled":
                st["culled_pairs"] += 1
            if res != "pair":
                continue
            st["pairs"] += 1
            st["pixel_tests"] += (pr["x1"] - pr["x0"] + 1) * (pr["y1"] - pr["y0"] + 1)
            pairs.append(dict(pr, triangle=t, view=v))
            xs = np.arange(pr["x0"], pr["x1"] + 1, dtype=np.float64)[None, :]
            ys = np.arange(pr["y0"], pr["y1"] + 1, dtype=np.float64)[:, None]
            r, D = pr["r"], pr["D"]
            with np.errstate(all="ignore"):
                l = [(np.float64(rk[0]) * xs + np.float64(rk[1]) * ys) + np.float64(rk[2]) for rk in r]
                if D > 0.0:
                    cov = (l[0] >= 0.0) & (l[1] >= 0.0) & (l[2] >= 0.0)
                else:
                    cov = (l[0] <= 0.0) & (l[1] <= 0.0) & (l[2] <= 0.0)
                w = (l[0] + l[1]) + l[2]
                cov &= w != 0.0
                z = (np.float64(D) / np.where(cov, w, 1.0)).astype(np.float32)
                cov &= np.isfinite(z) & (z > 0)
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
            box = zbuf[k][pr["y0"]:pr["y1"] + 1, pr["x0"]:pr["x1"] + 1]
            np.minimum(box, np.where(cov, key, EMPTY), out=box)
    out = dict(views=views, depth=[], index=[], normal=[], stats=st, pairs=pairs)
    normal_of = {}
    for z in zbuf:
        hit = z != EMPTY
        idx = np.where(hit, (z & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        depth = np.where(hit, (z >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
        nrm = np.zeros(z.shape + (3,), np.float32)
        for t in np.unique(idx[hit]):
            if t not in normal_of:
                normal_of[t] = face_normal(taking[int(t)])
            nrm[idx == t] = normal_of[t]
        st["covered_pixels"] += int(hit.sum())
        out["depth"].append(depth)
        out["index"].append(idx)
        out["normal"].append(nrm)
    return out


# ---- the meshes and cameras the tests share ------------------------------------

def as_vertices(pos):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["pos"] = np.asarray(pos, np.float32).reshape(-1, 3)
    return v


def look_at(eye, target, f, W, H, up=(0.0, 0.0, 1.0)):
    """K [R | -R eye] of a camera at eye looking at target, focal length f pixels,
    principal point at the image centre"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, (-R @ eye)[:, None]], 1)


SPHERE_SIZES = [(96, 64), (67, 45), (33, 21), (96, 64), (45, 67)]


def sphere_cameras(centre, sizes=SPHERE_SIZES, distance=1.1):
    """cameras of unequal, odd sizes around the TSDF sphere (radius 0.3), all
    outside it; the sphere fills about two thirds of the shorter side"""
    Ps = []
    for k, (W, H) in enumerate(sizes):
        a = 2.0 * math.pi * k / len(sizes) + 0.3
        eye = np.asarray(centre) + distance * np.array([math.cos(a) * 0.9, math.sin(a) * 0.9, 0.436 * (-1) ** k])
        Ps.append(look_at(eye, centre, 1.2 * min(W, H), W, H))
    return Ps


def tsdf_sphere():
    """the sphere of a 16^3 volume meshed by the TSDF reference: (vertices,
    triangles, centre, voxel), about a thousand outward-wound triangles"""
    import meshsmooth_ref as SR
    import tsdf_ref as TR

    vol, centre = SR.sphere_volume(16)
    m = TR.mesh(vol["tsdf"], vol["weight"], None, origin=vol["origin"], voxel=vol["voxel"], dim=vol["dim"])
    return m["vertices"].astype(VERTEX_DTYPE), SR.as_triangles(m["triangles"]), centre, vol["voxel"]


def planted_cameras():
    """(P, W, H): power-of-two intrinsics and integer centres as tests/partcases.py
    builds them, all at the origin looking down +z: 96 x 64 with f = 32, 67 x 45
    with f = 16, and the first mirrored in x (its left 3x3 has a negative
    determinant, so the facing rule needs m_v)"""
    from partcases import Cam

    a, b = Cam(0, 96, 64, 32.0, 32.0, 32.0), Cam(0, 67, 45, 16.0, 16.0, 16.0)
    mirrored = a.P.copy()
    mirrored[0] = [-32.0, 0.0, 64.0, 0.0]
    return [a.P, b.P, mirrored], [96, 67, 96], [64, 45, 64]


def planted_mesh():
    """(vertices, triangles, names): names maps a label to its triangle indices.
    Every vertex is cam.at(u, v, depth) of the first planted camera with integer
    (u, v) and a power-of-two depth, so its projections there are exact."""
    from partcases import Cam

    cam = Cam(0, 96, 64, 32.0, 32.0, 32.0)
    pos, tris, names = [], [], {}

    def tri(label, *pts):
        """pts: (u, v, depth), or a ready position as an array"""
        ids = []
        for p in pts:
            pos.append(tuple(p) if isinstance(p, np.ndarray) else cam.at(*p))
            ids.append(len(pos) - 1)
        tris.append(ids)
        names.setdefault(label, []).append(len(tris) - 1)
        return ids

    # a quad of two front-facing triangles sharing the diagonal (8, 8)-(24, 24)
    # in opposite directions, by shared vertex indices
    q = tri("quad", (8, 8, 2.0), (8, 24, 2.0), (24, 24, 2.0))
    pos.append(cam.at(24, 8, 2.0))
    tris.append([q[0], q[2], len(pos) - 1])
    names["quad"].append(len(tris) - 1)
    # two coincident front-facing triangles
    tri("coincident", (30, 8, 2.0), (30, 20, 2.0), (44, 20, 2.0))
    tri("coincident", (30, 8, 2.0), (30, 20, 2.0), (44, 20, 2.0))
    # edge-on: three points on one image line, D == 0 exactly
    tri("edge_on", (40, 30, 1.0), (50, 30, 2.0), (60, 30, 4.0))
    # one vertex behind the camera, one on the camera plane, all behind
    tri("one_behind", (50, 40, 2.0), (50, 50, 2.0), (60, 50, -1.0))
    tri("on_plane", (50, 40, 2.0), (50, 50, 2.0), np.array([0.5, 0.25, 0.0]))
    tri("all_behind", (50, 40, -2.0), (50, 50, -2.0), (60, 50, -1.0))
    # back-facing (the quad's winding reversed), alone in its region
    tri("back", (50, 8, 2.0), (62, 20, 2.0), (50, 20, 2.0))
    # wholly outside the frame of every planted camera; partly outside
    tri("outside", (200, 8, 2.0), (200, 20, 2.0), (230, 20, 2.0))
    tri("partly_outside", (-20, 40, 2.0), (-20, 70, 2.0), (20, 70, 2.0))
    # a box narrower than a wave: 3 x 3 pixels
    tri("tiny", (70, 8, 2.0), (70, 10, 2.0), (72, 10, 2.0))
    # a NaN position
    tri("nan", (70, 30, 2.0), (70, 40, 2.0), np.array([float("nan"), 0.0, 2.0]))
    nv = len(pos)
    for bad in ([0, 1, nv], [-1, 1, 2], [0, 2**31 - 1, 2], [-2**31, 0, 1]):
        tris.append(bad)
        names.setdefault("invalid", []).append(len(tris) - 1)
    return as_vertices(pos), np.array(tris, np.int32), names


def full_view_triangle(depth=8.0):
    """one front-facing triangle that covers the whole 96 x 64 planted view"""
    from partcases import Cam

    cam = Cam(0, 96, 64, 32.0, 32.0, 32.0)
    return as_vertices([cam.at(-16, -16, depth), cam.at(-16, 240, depth), cam.at(400, -16, depth)]), \
        np.array([[0, 1, 2]], np.int32)


def quad(depth=2.0, tilt=0.5):
    """a planar quad of two triangles in front of the first planted camera, tilted
    about the y axis: (vertices, triangles, plane point, plane normal)"""
    c = np.array([[-1.0, -0.7], [-1.0, 0.7], [1.0, 0.7], [1.0, -0.7]])
    pos = np.stack([c[:, 0], c[:, 1], depth + tilt * c[:, 0]], 1)
    v = as_vertices(pos)
    p = v["pos"].astype(np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), p[0], n / np.linalg.norm(n)
