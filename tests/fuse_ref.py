"""CPU reference of dp_fuse_maps, restated from the spec text in
include/densepoints.h (not from the kernels): fp64 in the header's order, one
(pixel's view, observing view) pair at a time, numpy evaluating the pixels
elementwise, each with the same single-rounding operations."""
import numpy as np

# dp_fused_point as the header lays it out
POINT = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3), ("n_views", "u1"), ("view", "<i4"),
                  ("x", "<i4"), ("y", "<i4")], align=True)
NO_SUPPRESS = 1
F32_MAX = np.float32(3.4028234663852886e38)


def row(P, r, X):
    return ((P[r][0] * X[0] + P[r][1] * X[1]) + P[r][2] * X[2]) + P[r][3]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def is_depth(z):
    with np.errstate(invalid="ignore"):
        return (z > np.float32(0)) & (z <= F32_MAX)


class Views:
    """P, W, H (and optionally the BGR8 images) of every view at the level the
    fusion runs on, with the per-view table of the spec: the adjugate and the
    determinant of the left 3x3 of P"""

    def __init__(self, P, W, H, images=None):
        self.P = [[[float(x) for x in r] for r in np.asarray(Pv, np.float64).reshape(3, 4)] for Pv in P]
        self.W, self.H = [int(w) for w in W], [int(h) for h in H]
        self.images = images
        self.V = len(self.P)
        self.A, self.det = [], []
        for Pv in self.P:
            h = [Pv[0][0], Pv[0][1], Pv[0][2], Pv[1][0], Pv[1][1], Pv[1][2], Pv[2][0], Pv[2][1], Pv[2][2]]
            A = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                 h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                 h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
            self.A.append(A)
            self.det.append((h[0] * A[0] + h[1] * A[3]) + h[2] * A[6])


def backproject(vw, v, x, y, z):
    """X (three fp64 arrays) of pixels (x, y) of view v with f32 depths z"""
    P, A, det = vw.P[v], vw.A[v], vw.det[v]
    with np.errstate(all="ignore"):
        zd = z.astype(np.float64)
        b0 = zd * x.astype(np.float64) - P[0][3]
        b1 = zd * y.astype(np.float64) - P[1][3]
        b2 = zd - P[2][3]
        return [((A[3 * j] * b0 + A[3 * j + 1] * b1) + A[3 * j + 2] * b2) / det for j in range(3)]


def observe(vw, s, X, depth_s, tol, nr=None, normal_s=None, cs=None):
    """steps 1-6 for the points X in view s: (matched, consistent, xi, yi, zs)"""
    P = vw.P[s]
    with np.errstate(all="ignore"):
        d = row(P, 2, X)
        ok = d > 0.0
        u = row(P, 0, X) / d
        v = row(P, 1, X) / d
        ok &= (np.abs(u) < 2e9) & (np.abs(v) < 2e9)
        xi = np.where(ok, np.rint(u), -1.0).astype(np.int64)
        yi = np.where(ok, np.rint(v), -1.0).astype(np.int64)
        ok &= (xi >= 0) & (xi < vw.W[s]) & (yi >= 0) & (yi < vw.H[s])
        xi, yi = np.where(ok, xi, 0), np.where(ok, yi, 0)
        zs = depth_s[yi, xi]
        matched = ok & (zs > np.float32(0))
        good = matched & (np.abs(zs.astype(np.float64) - d) <= np.float64(tol) * d)
        if nr is not None:
            ns = [normal_s[yi, xi, j].astype(np.float64) for j in range(3)]
            c = dot(nr, ns)
            good &= (c >= 0.0) & (c * c >= (cs * cs) * (dot(nr, nr) * dot(ns, ns)))
    return matched, good, xi, yi, zs


def fuse(vw, depth, normal=None, views=None, depth_tol=0.01, min_views=2, min_normal_cos=0.5, flags=0):
    """{"points" (POINT array), "mask", "fusable", "emitted" (lists of H x W planes
    in the order of `views`), "stats"}"""
    views = list(range(vw.V)) if views is None else [int(v) for v in views]
    K = len(views)
    assert 1 <= K <= 64 and len(depth) == K and (normal is None or len(normal) == K)
    tol, cs = np.float64(np.float32(depth_tol)), np.float64(np.float32(min_normal_cos))
    depth = [np.ascontiguousarray(d, np.float32) for d in depth]
    st = dict(depth_pixels=0, matched_pairs=0, consistent_pairs=0, fusable=0, emitted=0)
    px, masks, obs = [], [], []
    # pass 1: the masks (a function of the planes alone)
    for k, r in enumerate(views):
        ys, xs = np.nonzero(is_depth(depth[k]))  # row-major: ascending (y, x)
        z = depth[k][ys, xs]
        X = backproject(vw, r, xs, ys, z)
        nr = [normal[k][ys, xs, j].astype(np.float64) for j in range(3)] if normal is not None else None
        m = np.zeros(len(xs), np.uint64)
        seen = {}
        for kp, s in enumerate(views):
            if kp == k:
                continue
            matched, good, xi, yi, zs = observe(vw, s, X, depth[kp], tol, nr,
                                                normal[kp] if normal is not None else None, cs)
            m |= good.astype(np.uint64) << np.uint64(kp)
            seen[kp] = (good, xi, yi, zs)
            st["matched_pairs"] += int(matched.sum())
            st["consistent_pairs"] += int(good.sum())
        st["depth_pixels"] += len(xs)
        px.append((ys, xs, z, X, nr))
        masks.append(m)
        obs.append(seen)
    counts = [np.array([bin(int(v)).count("1") for v in m], np.int64) for m in masks]
    fus_plane, mask_plane = [], []
    for k in range(K):
        ys, xs = px[k][0], px[k][1]
        f = np.zeros(depth[k].shape, bool)
        f[ys, xs] = counts[k] >= int(min_views)
        mp = np.zeros(depth[k].shape, np.uint64)
        mp[ys, xs] = masks[k]
        fus_plane.append(f)
        mask_plane.append(mp)
        st["fusable"] += int(f.sum())
    # suppression (a function of the masks alone) and the emitted points
    out, emit_plane = [], []
    for k, r in enumerate(views):
        ys, xs, z, X, nr = px[k]
        emit = counts[k] >= int(min_views)
        if not flags & NO_SUPPRESS:
            for kp in range(k):
                good, xi, yi, _ = obs[k][kp]
                emit &= ~(good & fus_plane[kp][yi, xi])
        acc = [c.copy() for c in X]
        nsum = [c.copy() for c in nr] if nr is not None else None
        with np.errstate(all="ignore"):
            for kp in sorted(obs[k]):
                good, xi, yi, zs = obs[k][kp]
                Y = backproject(vw, views[kp], xi, yi, zs)
                for j in range(3):
                    acc[j] = np.where(good, acc[j] + Y[j], acc[j])
                    if nsum is not None:
                        nsum[j] = np.where(good, nsum[j] + normal[kp][yi, xi, j].astype(np.float64), nsum[j])
            m = 1 + counts[k]
            p = np.zeros(int(emit.sum()), POINT)
            for j in range(3):
                p["pos"][:, j] = (acc[j] / m.astype(np.float64)).astype(np.float32)[emit]
            if nsum is not None:
                q = dot(nsum, nsum)
                root = np.sqrt(q)
                for j in range(3):
                    p["normal"][:, j] = np.where(q > 0.0, nsum[j] / root, 0.0).astype(np.float32)[emit]
        if vw.images is not None:
            p["rgb"] = vw.images[r][ys[emit], xs[emit]][:, ::-1]  # BGR8 -> R, G, B
        p["n_views"] = m[emit]
        p["view"], p["x"], p["y"] = r, xs[emit], ys[emit]
        out.append(p)
        e = np.zeros(depth[k].shape, bool)
        e[ys, xs] = emit
        emit_plane.append(e)
        st["emitted"] += len(p)
    return dict(views=views, points=np.concatenate(out) if out else np.zeros(0, POINT), mask=mask_plane,
                fusable=fus_plane, emitted=emit_plane, stats=st)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
