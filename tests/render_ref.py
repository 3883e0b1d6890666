"""CPU reference of dp_render_maps, restated from the spec text in
include/densepoints.h (not from the kernels): fp64 in the header's order, one
(patch, view) pair at a time over its candidate box (numpy evaluates the box's
pixels elementwise, each with the same single-rounding operations)."""
import math

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def row(P, r, X):
    return ((P[r][0] * X[0] + P[r][1] * X[1]) + P[r][2] * X[2]) + P[r][3]


def project(P, X):
    h2 = row(P, 2, X)
    with np.errstate(all="ignore"):
        return float(np.float64(row(P, 0, X)) / np.float64(h2)), float(np.float64(row(P, 1, X)) / np.float64(h2))


class Cameras:
    """P, W, H and the derived C, xr of every view (orc.view_geometry, the
    x-axis normalised as GetXAxis().normalized())."""

    def __init__(self, orc, P, W, H):
        self.P = [[[float(x) for x in r] for r in np.asarray(Pv, np.float64).reshape(3, 4)] for Pv in P]
        self.W, self.H = [int(w) for w in W], [int(h) for h in H]
        self.C, self.xr = [], []
        for Pv in P:
            rc, C, _, _, xa = orc.view_geometry(np.asarray(Pv, np.float64))
            assert rc == 0
            nx = math.sqrt(dot(xa, xa))
            self.C.append([float(c) for c in C])
            self.xr.append([float(x) / nx for x in xa])
        self.V = len(self.P)


def pixel_step(P, xr, X):
    """distance of the projections of X and X + xr, and the projection of X"""
    cu, cv = project(P, X)
    qu, qv = project(P, [X[k] + xr[k] for k in range(3)])
    du, dv = qu - cu, qv - cv
    return math.sqrt(du * du + dv * dv), cu, cv


def rho_of(cams, p, grid_scale=8):
    ref = int(p["ref"])
    if ref >= cams.V:
        return 0.0
    X = [float(c) for c in p["pos"]]
    dx = pixel_step(cams.P[ref], cams.xr[ref], X)[0]
    return float(grid_scale) / dx if dx > 0.0 else 0.0


def takes_part(cams, p, grid_scale=8):
    if not (np.isfinite(p["pos"]).all() and np.isfinite(p["normal"]).all()):
        return False
    return int(p["ref"]) < cams.V and rho_of(cams, p, grid_scale) > 0.0


def make_pair(cams, v, p, R, max_radius_px, all_facing):
    """the pair record of the spec, or None: dict(A, D, s, RR, x0, x1, y0, y1, clipped)"""
    P, xr = cams.P[v], cams.xr[v]
    X = [float(c) for c in p["pos"]]
    n = [float(c) for c in p["normal"]]
    if all_facing:
        if not dot(n, [X[k] - cams.C[v][k] for k in range(3)]) > 0.0:
            return None
    elif not (int(p["vis"][v >> 6]) >> (v & 63)) & 1:
        return None
    if not row(P, 2, X) > 0.0:
        return None
    t = dot(xr, n)
    e1 = [xr[k] - t * n[k] for k in range(3)]
    s = dot(e1, e1)
    if not s >= 1e-12:
        return None
    e2 = [n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]]
    dxv, cu, cv = pixel_step(P, xr, X)
    if not (abs(cu) < 2e9 and abs(cv) < 2e9):
        return None
    Bq = (2.0 * R) * dxv + 2.0
    B = Bq if Bq < float(max_radius_px) else float(max_radius_px)
    bx0, bx1 = math.floor(cu - B), math.ceil(cu + B)
    by0, by1 = math.floor(cv - B), math.ceil(cv + B)
    x0, x1 = max(0, bx0), min(cams.W[v] - 1, bx1)
    y0, y1 = max(0, by0), min(cams.H[v] - 1, by1)
    if x0 > x1 or y0 > y1:
        return None
    h = [0.0] * 9
    for r in range(3):
        h[3 * r] = (P[r][0] * e1[0] + P[r][1] * e1[1]) + P[r][2] * e1[2]
        h[3 * r + 1] = (P[r][0] * e2[0] + P[r][1] * e2[1]) + P[r][2] * e2[2]
        h[3 * r + 2] = row(P, r, X)
    A = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
         h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
         h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    D = (h[0] * A[0] + h[1] * A[3]) + h[2] * A[6]
    return dict(A=A, D=D, s=s, RR=R * R, x0=x0, x1=x1, y0=y0, y1=y1, cu=cu, cv=cv,
                clipped=(x0, x1, y0, y1) != (bx0, bx1, by0, by1))


def raster(pr, index, zbuf):
    """the pair's covered pixels into zbuf (H x W uint64 keys), by minimum"""
    A, D = pr["A"], pr["D"]
    x = np.arange(pr["x0"], pr["x1"] + 1, dtype=np.float64)[None, :]
    y = np.arange(pr["y0"], pr["y1"] + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        a = (A[0] * x + A[1] * y) + A[2]
        b = (A[3] * x + A[4] * y) + A[5]
        w = (A[6] * x + A[7] * y) + A[8]
        sign = ((w > 0.0) & (D > 0.0)) | ((w < 0.0) & (D < 0.0))
        cover = sign & ((a * a + b * b) * pr["s"] <= pr["RR"] * (w * w))
        z = (np.float64(D) / w).astype(np.float32)
    cover &= z > np.float32(0.0)
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(index)
    sub = zbuf[pr["y0"]:pr["y1"] + 1, pr["x0"]:pr["x1"] + 1]
    sub[cover] = np.minimum(sub[cover], key[cover])
    return int(cover.sum())


def render(cams, patches, views=None, keep=None, splat_scale=1.0, max_radius_px=32, all_facing=False,
           grid_scale=8):
    """{"depth", "index", "normal", "score": lists per requested view, "stats",
    "pairs": the pair records with "view" and "index" added}"""
    views = list(range(cams.V)) if views is None else [int(v) for v in views]
    zb = {v: np.full((cams.H[v], cams.W[v]), EMPTY, dtype=np.uint64) for v in views}
    st = dict(patches=0, pairs=0, pixel_tests=0, covered_pixels=0)
    pairs = []
    for i, p in enumerate(patches):
        if keep is not None and not keep[i]:
            continue
        if not takes_part(cams, p, grid_scale):
            continue
        st["patches"] += 1
        R = float(np.float32(splat_scale)) * rho_of(cams, p, grid_scale)
        for v in sorted(views):
            pr = make_pair(cams, v, p, R, max_radius_px, all_facing)
            if pr is None:
                continue
            st["pairs"] += 1
            st["pixel_tests"] += (pr["x1"] - pr["x0"] + 1) * (pr["y1"] - pr["y0"] + 1)
            pr["hits"] = raster(pr, i, zb[v])
            pr["view"], pr["index"] = v, i
            pairs.append(pr)
    out = dict(views=views, depth=[], index=[], normal=[], score=[], pairs=pairs)
    for v in views:
        hit = zb[v] != EMPTY
        idx = np.where(hit, (zb[v] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        depth = np.where(hit, (zb[v] >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
        safe = np.where(hit, idx, 0)
        if len(patches):
            normal = np.where(hit[..., None], patches["normal"][safe], np.float32(0)).astype(np.float32)
            score = np.where(hit, patches["score"][safe], np.float32(0)).astype(np.float32)
        else:
            normal = np.zeros(hit.shape + (3,), np.float32)
            score = np.zeros(hit.shape, np.float32)
        out["depth"].append(depth)
        out["index"].append(idx)
        out["normal"].append(normal)
        out["score"].append(score)
        st["covered_pixels"] += int(hit.sum())
    out["stats"] = st
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
