"""CPU reference of dp_mesh_colour, restated from the spec text in
include/densepoints.h (not from the kernel): fp64 in the header's order, one
(vertex, view) pair at a time, every operation a single IEEE rounding (Python
floats and numpy float64 scalars).  Also the images and planted scenes the
mesh-colour tests share."""
import math

import numpy as np

COUNTS = ("vertices", "projected_pairs", "occluded_pairs", "grazing_pairs", "visible_pairs", "coloured_vertices",
          "unseen_vertices")
VERTEX_DTYPE = np.dtype([("pos", np.float32, 3), ("rgb", np.uint8, 3), ("pad", np.uint8)])
FLT_MAX = 3.402823466e+38


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def row(P, r, X):
    return ((P[4 * r] * X[0] + P[4 * r + 1] * X[1]) + P[4 * r + 2] * X[2]) + P[4 * r + 3]


def div(a, b):
    """a / b as IEEE does it: no exception on a zero or an overflow"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def is_depth(z):
    return z > 0.0 and z <= FLT_MAX


def view_table(P):
    """(P as 12 floats, A, det, C) of dp_fuse_maps's view table and the camera
    centre backproject(v, 0, 0, 0)"""
    P = [float(x) for x in np.asarray(P, np.float64).reshape(12)]
    h = [P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]]
    A = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
         h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
         h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    det = (h[0] * A[0] + h[1] * A[3]) + h[2] * A[6]
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("a view's det is 0 or not finite")
    C = [div((A[3 * j] * (0.0 - P[3]) + A[3 * j + 1] * (0.0 - P[7])) + A[3 * j + 2] * (0.0 - P[11]), det)
         for j in range(3)]
    if not all(math.isfinite(c) for c in C):
        raise ValueError("a view's centre is not finite")
    return P, A, det, C


def observe(P, W, H, X):
    """steps 1-3 of dp_fuse_maps's observe: (d, u, v, xi, yi) or None"""
    d = row(P, 2, X)
    if not d > 0.0:
        return None
    u, v = div(row(P, 0, X), d), div(row(P, 1, X), d)
    if not (abs(u) < 2.0e9 and abs(v) < 2.0e9):
        return None
    xi, yi = int(np.rint(u)), int(np.rint(v))
    if not (0 <= xi < W and 0 <= yi < H):
        return None
    return d, u, v, xi, yi


def clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def sample(img, u, v, xi, yi, bilinear):
    """step 5: the R, G, B values of a BGR8 image H x W x 3 (channel 0 = B)"""
    H, W = img.shape[:2]

    def t(x, y, ch):
        return float(img[y, x, 2 - ch])

    if not bilinear:
        return [t(xi, yi, ch) for ch in range(3)]
    x0, y0 = math.floor(u), math.floor(v)
    fx, fy = u - float(x0), v - float(y0)
    xa, xb = clamp(x0, 0, W - 1), clamp(x0 + 1, 0, W - 1)
    ya, yb = clamp(y0, 0, H - 1), clamp(y0 + 1, 0, H - 1)
    out = []
    for ch in range(3):
        top = (1.0 - fx) * t(xa, ya, ch) + fx * t(xb, ya, ch)
        bot = (1.0 - fx) * t(xa, yb, ch) + fx * t(xb, yb, ch)
        out.append((1.0 - fy) * top + fy * bot)
    return out


def colour(P, images, vertices, depth, views=None, normals=None, depth_tol=0.01, min_cos=0.2, bilinear=False,
           clear_unseen=False):
    """dict(vertices, seen, best, views, stats): P and images (BGR8, H x W x 3) of
    ALL views at the current level, depth one plane per requested view"""
    verts = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE).reshape(-1)
    views = list(range(len(images))) if views is None else [int(v) for v in views]
    assert 1 <= len(views) <= 64 and len(set(views)) == len(views) and len(depth) == len(views)
    tab = [view_table(P[v]) for v in views]
    tol, mc = float(np.float32(depth_tol)), float(np.float32(min_cos))
    out = verts.copy()
    seen, best = np.zeros(len(verts), np.uint64), np.full(len(verts), -1, np.int32)
    st = dict.fromkeys(COUNTS, 0)
    for i, vx in enumerate(verts):
        if not np.isfinite(vx["pos"]).all():
            continue
        st["vertices"] += 1
        X = [float(c) for c in vx["pos"]]
        has_normal = False
        if normals is not None:
            n = [float(c) for c in np.asarray(normals, np.float32).reshape(-1, 3)[i]]
            with np.errstate(all="ignore"):
                l2 = float(dot([np.float64(c) for c in n], [np.float64(c) for c in n]))
            has_normal = math.isfinite(l2) and l2 > 0.0
        wsum, s, mask, bk, bw = 0.0, [0.0, 0.0, 0.0], 0, -1, 0.0
        for k, v in enumerate(views):
            Pv, _, _, C = tab[k]
            img = images[v]
            H, W = img.shape[:2]
            assert depth[k].shape == (H, W) and depth[k].dtype == np.float32
            with np.errstate(all="ignore"):
                ob = observe([np.float64(p) for p in Pv], W, H, [np.float64(x) for x in X])
            if ob is None:
                continue
            d, u, w, xi, yi = (float(ob[0]), float(ob[1]), float(ob[2]), ob[3], ob[4])
            z = float(depth[k][yi, xi])
            if not is_depth(z):
                continue
            st["projected_pairs"] += 1
            with np.errstate(all="ignore"):
                visible = bool(np.float64(d) - np.float64(z) <= np.float64(tol) * np.float64(d))
            if not visible:
                st["occluded_pairs"] += 1
                continue
            wgt = 1.0
            if has_normal:
                with np.errstate(all="ignore"):
                    ray = [np.float64(X[j]) - np.float64(C[j]) for j in range(3)]
                    q = float(dot(ray, ray) * np.float64(l2))
                    ok = math.isfinite(q) and q > 0.0
                    if ok:
                        c = float((np.float64(0.0) - dot([np.float64(a) for a in n], ray)) / np.sqrt(np.float64(q)))
                        ok = c > 0.0 and c >= mc
                if not ok:
                    st["grazing_pairs"] += 1
                    continue
                wgt = c
            val = sample(img, u, w, xi, yi, bilinear)
            for ch in range(3):
                s[ch] = s[ch] + wgt * val[ch]
            wsum = wsum + wgt
            mask |= 1 << k
            if wgt > bw:
                bw, bk = wgt, k
            st["visible_pairs"] += 1
        seen[i], best[i] = mask, bk
        if mask:
            st["coloured_vertices"] += 1
            out["rgb"][i] = [int(min(255.0, float(np.rint(div(s[ch], wsum))))) for ch in range(3)]
        else:
            st["unseen_vertices"] += 1
            if clear_unseen:
                out["rgb"][i] = 0
    return dict(vertices=out, seen=seen, best=best, views=views, stats=st)


# ---- the images and planted scenes the tests share ------------------------------

def hash_image(v, W, H):
    """a BGR8 image H x W x 3 whose every byte is a different deterministic hash
    of (v, x, y, channel)"""
    y, x = np.mgrid[0:H, 0:W].astype(np.uint64)
    out = np.zeros((H, W, 3), np.uint8)
    for ch in range(3):
        h = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ np.uint64((v * 3 + ch + 1) * 83492791)
        h = (h ^ (h >> np.uint64(13))) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)
        out[..., ch] = ((h >> np.uint64(11)) & np.uint64(255)).astype(np.uint8)
    return out


def as_vertices(pos, rgb=(9, 8, 7)):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["pos"] = np.asarray(pos, np.float32).reshape(-1, 3)
    v["rgb"] = rgb
    return v


def planted():
    """The planted planes: dict(P, images, depth, vertices, normals, names).
    Views: 0 = 96 x 64, f = 32 at the origin looking down +z; 1 = 8 x 8, f = 4,
    the same centre; 2 = view 0 mirrored in x (negative determinant); 3 = 16 x 8,
    f = 4.  The intrinsics are powers of two and every vertex is cam.at(u, v,
    depth) with u, v multiples of 1/2 and a power-of-two depth, so d, u and v
    are exact.  names maps a label to its vertex."""
    from partcases import Cam

    c0, c1, c3 = Cam(0, 96, 64, 32.0, 32.0, 32.0), Cam(0, 8, 8, 4.0, 4.0, 4.0), Cam(0, 16, 8, 4.0, 8.0, 4.0)
    mirrored = c0.P.copy()
    mirrored[0] = [-32.0, 0.0, 64.0, 0.0]
    P = [c0.P, c1.P, mirrored, c3.P]
    sizes = [(96, 64), (8, 8), (96, 64), (16, 8)]
    images = [hash_image(v, w, h) for v, (w, h) in enumerate(sizes)]
    depth = [np.zeros((h, w), np.float32) for w, h in sizes]
    pos, nrm, names = [], [], {}

    def vertex(label, p, n=(0.0, 0.0, -1.0)):
        names[label] = len(pos)
        pos.append(tuple(float(c) for c in p))
        nrm.append(n)

    def plane(v, u, w, z):
        """pixel (u, w) of view v; in the mirrored view column 64 - (u - 32)"""
        depth[v][w, u] = z

    # d = 4, z = 3, depth_tol = 0.25: d - z == tol * d exactly, <= against <
    vertex("tol_edge", c0.at(10, 10, 4.0))
    plane(0, 10, 10, 3.0)
    # ... and one ulp of f32 nearer: occluded
    vertex("tol_over", c0.at(12, 10, 4.0))
    plane(0, 12, 10, float(np.nextafter(np.float32(3.0), np.float32(0.0))))
    # z farther than d: the test is one-sided, visible however far
    vertex("behind_surface", c0.at(14, 10, 4.0))
    plane(0, 14, 10, 64.0)
    # x.5 rounds half-even: u = 20.5 -> 20, u = 21.5 -> 22; only the even pixels hold a depth
    vertex("half_even_down", c0.at(20.5, 10, 4.0))
    vertex("half_even_up", c0.at(21.5, 10, 4.0))
    plane(0, 20, 10, 4.0)
    plane(0, 22, 10, 4.0)
    # u = W - 0.5 rounds to W: outside, although column W - 1 holds a depth
    vertex("outside", c0.at(95.5, 12, 4.0))
    plane(0, 95, 12, 4.0)
    # behind the camera; not finite; an empty pixel
    vertex("behind_camera", c0.at(30, 10, -4.0))
    plane(0, 30, 10, 4.0)
    vertex("nan", (float("nan"), 0.0, 4.0))
    vertex("inf", (0.25, float("inf"), 4.0))
    vertex("empty_pixel", c0.at(40, 10, 4.0))
    # a normal at right angles to the ray: c == 0, refused even with min_cos = 0
    p = c0.at(32, 32, 4.0)  # on the axis: the ray is (0, 0, 4)
    vertex("right_angle", p, (1.0, 0.0, 0.0))
    plane(0, 32, 32, 4.0)
    # a zero normal: weight 1; a normal facing away: grazing
    vertex("zero_normal", c0.at(34, 32, 4.0), (0.0, 0.0, 0.0))
    plane(0, 34, 32, 4.0)
    vertex("facing_away", c0.at(36, 32, 4.0), (0.0, 0.0, 1.0))
    plane(0, 36, 32, 4.0)
    # seen by views 0 and 1 (both at the origin): pixel (48, 40) of view 0 is
    # pixel (6, 5) of view 1; the two texels are planted for rint(1.5), rint(2.5)
    vertex("two_views", c0.at(48, 40, 4.0), (0.0, 0.0, 0.0))
    plane(0, 48, 40, 4.0)
    plane(1, 6, 5, 4.0)
    images[0][40, 48] = [2, 1, 1]  # B, G, R
    images[1][5, 6] = [3, 2, 2]    # means: R 1.5 -> 2, G 1.5 -> 2, B 2.5 -> 2
    # the small views' last pixel and the wide view's last column
    vertex("corner_8x8", c1.at(7, 7, 2.0), (0.0, 0.0, 0.0))
    plane(1, 7, 7, 2.0)
    vertex("wide_last_column", c3.at(15, 3, 2.0), (0.0, 0.0, 0.0))
    plane(3, 15, 3, 2.0)
    # the mirrored view sees what view 0 sees, at the mirrored column
    for label in ("tol_edge", "tol_over", "behind_surface", "right_angle", "zero_normal", "facing_away"):
        X = pos[names[label]]
        u0, w = 32.0 + 32.0 * X[0] / X[2], 32.0 + 32.0 * X[1] / X[2]
        um = 64.0 - 32.0 * X[0] / X[2]
        assert u0 == int(u0) and um == int(um) and w == int(w)
        plane(2, int(um), int(w), float(depth[0][int(w), int(u0)]))
    return dict(P=P, images=images, depth=depth, sizes=sizes, vertices=as_vertices(pos),
                normals=np.asarray(nrm, np.float32), names=names)


def last_of_64():
    """K = 64 views of 8 x 8 at the origin, f = 4; one vertex at the centre pixel
    that only the last view's plane holds: dict(P, images, depth, vertices)"""
    from partcases import Cam

    cam = Cam(0, 8, 8, 4.0, 4.0, 4.0)
    P = [cam.P for _ in range(64)]
    images = [hash_image(v, 8, 8) for v in range(64)]
    depth = [np.zeros((8, 8), np.float32) for _ in range(64)]
    depth[63][4, 4] = 2.0
    return dict(P=P, images=images, depth=depth, vertices=as_vertices([cam.at(4, 4, 2.0)]))
