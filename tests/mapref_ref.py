"""CPU reference of dp_refine_maps, restated from the spec text in
include/densepoints.h (not from the kernel): fp64 in the header's order, numpy
evaluating the pixels of one (view, candidate, source) elementwise, each with
the same single-rounding operations; the fp32 FMAs of the sampler are single
roundings too (fmaf below, the vectorised form of tests/test_fast_spec_cpu.py's)."""
import numpy as np

import fuse_ref as FR
import render_ref as RR
from fuse_ref import dot, is_depth, row

KEEP_UNSCORED = 1
COUNTS = ("depth_pixels_in", "candidates", "source_scores", "kept", "filled", "moved")
F32 = np.float32
B23 = np.float32(8388608.0)
CHUNK = 4096  # pixels sampled at a time (bounds the N-samples-wide temporaries)


def fmaf(a, b, c):
    """fmaf on float32 arrays.  a*b is exact in fp64; t = a*b + c is rounded to
    fp64 once, and TwoSum gives its error e exactly.  The fp32 rounding of t is
    the rounding of the exact sum unless t sits exactly halfway between two
    fp32 values while e != 0: then the exact sum lies on e's side of the tie."""
    s = a.astype(np.float64) * b.astype(np.float64)
    c64 = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), s.shape)
    t = s + c64
    bb = t - s
    e = (s - (t - bb)) + (c64 - bb)
    r = t.astype(np.float32)
    d = t - r.astype(np.float64)
    fix = np.nonzero((e != 0) & (d != 0))
    if len(fix[0]):
        rf, df, ef, tf = r[fix], d[fix], e[fix], t[fix]
        other = np.nextafter(rf, np.where(df > 0, F32(np.inf), F32(-np.inf)).astype(np.float32))
        tie = (other.astype(np.float64) - tf) == df
        r[fix] = np.where(tie & ((ef > 0) == (df > 0)), other, rf)
    return r


def gray_of(img):
    """BGR2GRAY of the gray planes (14-bit fixed point), as int64"""
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


class Views:
    """the level's P, W, H, the view table of dp_fuse_maps (A, det), C and xr of
    dp_render_maps, and the gray planes"""

    def __init__(self, orc, P, images):
        W, H = [im.shape[1] for im in images], [im.shape[0] for im in images]
        self.t = FR.Views(P, W, H)
        cams = RR.Cameras(orc, np.asarray(P, np.float64).reshape(-1, 3, 4), W, H)
        self.P, self.A, self.det, self.W, self.H, self.V = self.t.P, self.t.A, self.t.det, W, H, self.t.V
        self.C, self.xr = cams.C, cams.xr
        self.gray = [gray_of(im) for im in images]


def backproject_d(vw, v, x, y, zd):
    P, A, det = vw.P[v], vw.A[v], vw.det[v]
    b0 = zd * x - P[0][3]
    b1 = zd * y - P[1][3]
    b2 = zd - P[2][3]
    return [((A[3 * j] * b0 + A[3 * j + 1] * b1) + A[3 * j + 2] * b2) / det for j in range(3)]


def default_sources(vw, views, max_sources):
    out = []
    for r in views:
        near = []
        for s in views:
            if s != r:
                e = [vw.C[s][j] - vw.C[r][j] for j in range(3)]
                near.append((dot(e, e), s))
        out.append([s for _, s in sorted(near)][:max_sources])
    return out


def has_plane(z, n):
    nd = [n[..., j].astype(np.float64) for j in range(3)]
    with np.errstate(all="ignore"):
        return is_depth(z) & (dot(nd, nd) > 0.0)


def source_ncc(vw, r, s, x, y, Xc, Xi, Xj, window, Sa, Saa, A, dmin):
    """(valid, ncc) of the candidates' planes (their three points) against
    source s; A: the reference samples (M x N int64)"""
    P = vw.P[s]
    hw, N = (window - 1) // 2, window * window
    Ws, Hs = vw.W[s], vw.H[s]
    with np.errstate(all="ignore"):
        dc, di, dj = row(P, 2, Xc), row(P, 2, Xi), row(P, 2, Xj)
        ok = (dc > 0.0) & (di > 0.0) & (dj > 0.0)
        uc, vc = row(P, 0, Xc) / dc, row(P, 1, Xc) / dc
        ui, vi = row(P, 0, Xi) / di, row(P, 1, Xi) / di
        uj, vj = row(P, 0, Xj) / dj, row(P, 1, Xj) / dj
        U0, V0 = (32.0 * uc).astype(F32), (32.0 * vc).astype(F32)
        Ui, Vi = (32.0 * (ui - uc)).astype(F32), (32.0 * (vi - vc)).astype(F32)
        Uj, Vj = (32.0 * (uj - uc)).astype(F32), (32.0 * (vj - vc)).astype(F32)
        umax, vmax = 32.0 * float(Ws - 1), 32.0 * float(Hs - 1)
        for ci in (-float(hw), float(hw)):
            for cj in (-float(hw), float(hw)):
                a = (U0.astype(np.float64) + ci * Ui.astype(np.float64)) + cj * Uj.astype(np.float64)
                b = (V0.astype(np.float64) + ci * Vi.astype(np.float64)) + cj * Vj.astype(np.float64)
                ok &= (a >= 0.0) & (a <= umax) & (b >= 0.0) & (b <= vmax)
    ncc = np.full(len(x), -np.inf)
    sel = np.nonzero(ok)[0]
    g = vw.gray[s]
    t = np.arange(-hw, hw + 1, dtype=np.float32)
    ti, tj = np.tile(t, window)[None, :], np.repeat(t, window)[None, :]
    ulim, vlim = B23 + F32(32 * (Ws - 1)), B23 + F32(32 * (Hs - 1))
    for c0 in range(0, len(sel), CHUNK):
        q = sel[c0:c0 + CHUNK]
        col = lambda a: a[q][:, None]  # noqa: E731
        U = fmaf(tj, col(Uj), fmaf(ti, col(Ui), col(U0))) + B23
        V = fmaf(tj, col(Vj), fmaf(ti, col(Vi), col(V0))) + B23
        U = np.minimum(np.maximum(U, B23), ulim)
        V = np.minimum(np.maximum(V, B23), vlim)
        iu, iv = (U - B23).astype(np.int64), (V - B23).astype(np.int64)
        xs, fx, yv, fy = iu >> 5, iu & 31, iv >> 5, iv & 31
        x1, y1 = np.minimum(xs + 1, Ws - 1), np.minimum(yv + 1, Hs - 1)
        b = ((32 - fx) * (32 - fy) * g[yv, xs] + fx * (32 - fy) * g[yv, x1] + (32 - fx) * fy * g[y1, xs] +
             fx * fy * g[y1, x1] + 32) >> 6
        a = A[q]
        Sb, Sbb, Sab = b.sum(1), (b * b).sum(1), (a * b).sum(1)
        num = N * Sab - Sa[q] * Sb
        va = N * Saa[q] - Sa[q] * Sa[q]
        vb = N * Sbb - Sb * Sb
        den = np.sqrt(va.astype(np.float64) * vb.astype(np.float64))
        ncc[q] = num.astype(np.float64) / np.where(den > dmin, den, dmin)
    return ok, ncc


def refine(vw, depth, normal, views=None, sources=None, window=7, sweep=2, step_px=1.0, reach=(1, 4), max_sources=4,
           top_k=2, min_ncc=0.5, flags=0, denom_min=0.1, only=None):
    """{"depth", "normal", "score", "choice": lists of planes in the order of
    `views`, "stats", "valid": per view the number of valid sources of candidate
    0 (-1 where it is void by its plane), "ncand": per view the number of
    non-void candidates}.  `only` (a list of H x W bool masks,
    for the CPU tests): the pixels to refine; the others come out empty and are
    not counted."""
    views = list(range(vw.V)) if views is None else [int(v) for v in views]
    K = len(views)
    assert 1 <= K <= 64 and len(depth) == K and len(normal) == K
    assert window % 2 == 1 and 3 <= window <= 11 and 1 <= top_k <= max_sources <= 8
    src = default_sources(vw, views, max_sources) if sources is None else \
        [[int(s) for s in row_ if s >= 0] for row_ in sources]
    step, thr = np.float64(np.float32(step_px)), np.float64(np.float32(min_ncc))
    N, hw = window * window, (window - 1) // 2
    dmin = ((denom_min * 256.0) * float(N)) * float(N)
    depth = [np.ascontiguousarray(d, np.float32) for d in depth]
    normal = [np.ascontiguousarray(n, np.float32) for n in normal]
    offsets = [(dx_, dy_) for d in reach if d > 0 for dx_, dy_ in ((-d, 0), (d, 0), (0, -d), (0, d))]
    st = dict.fromkeys(COUNTS, 0)
    out = dict(views=views, depth=[], normal=[], score=[], choice=[], valid=[], ncand=[])
    for k, r in enumerate(views):
        W, H = vw.W[r], vw.H[r]
        pick = np.ones((H, W), bool) if only is None or only[k] is None else only[k]
        y, x = np.nonzero(pick)
        M = len(x)
        z, n = depth[k][y, x], normal[k][y, x]
        own_depth = is_depth(z)
        own = has_plane(z, n)
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        P, A_, det = vw.P[r], vw.A[r], vw.det[r]
        g = vw.gray[r]
        # the reference samples and their moments: the same for every candidate
        t = np.arange(-hw, hw + 1)
        oi, oj = np.tile(t, window)[None, :], np.repeat(t, window)[None, :]
        Aref = 16 * g[np.clip(y[:, None] + oj, 0, H - 1), np.clip(x[:, None] + oi, 0, W - 1)]
        Sa, Saa = Aref.sum(1), (Aref * Aref).sum(1)
        with np.errstate(all="ignore"):
            Xo = FR.backproject(vw.t, r, x, y, z)
            d0 = row(P, 2, Xo)
            cu, cv = row(P, 0, Xo) / d0, row(P, 1, Xo) / d0
            Xq = [Xo[j] + vw.xr[r][j] for j in range(3)]
            d1 = row(P, 2, Xq)
            du, dv = row(P, 0, Xq) / d1 - cu, row(P, 1, Xq) / d1 - cv
            dx = np.sqrt(du * du + dv * dv)
            ray = [Xo[j] - vw.C[r][j] for j in range(3)]
            ln = np.sqrt(dot(ray, ray))
        cands = [(own, Xo, n)]
        for h in list(range(-sweep, 0)) + list(range(1, sweep + 1)):
            with np.errstate(all="ignore"):
                tt = (np.float64(h) * step) / dx
                Xh = [Xo[j] + (tt * ray[j]) / ln for j in range(3)]
                cands.append((own & (dx > 0.0) & (ln > 0.0), Xh, n))
        for ox, oy in offsets:
            px, py = x + ox, y + oy
            inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            pxc, pyc = np.where(inside, px, 0), np.where(inside, py, 0)
            zz, nn = depth[k][pyc, pxc], normal[k][pyc, pxc]
            with np.errstate(all="ignore"):
                cands.append((inside & has_plane(zz, nn), FR.backproject(vw.t, r, pxc, pyc, zz), nn))
        best = np.full(M, -np.inf)
        choice = np.full(M, -1, np.int64)
        wz = np.zeros(M, np.float32)
        wn = np.zeros((M, 3), np.float32)
        valid0 = np.full(M, -1, np.int64)
        ncand = np.zeros(M, np.int64)
        for ci, (live, X0, cn) in enumerate(cands):
            if not live.any():
                continue
            with np.errstate(all="ignore"):
                nd = [cn[:, j].astype(np.float64) for j in range(3)]
                m = [(A_[j] * nd[0] + A_[3 + j] * nd[1]) + A_[6 + j] * nd[2] for j in range(3)]
                c = det * dot(nd, X0) + dot(m, [P[0][3], P[1][3], P[2][3]])
                zc = c / ((m[0] * xd + m[1] * yd) + m[2])
                zf = zc.astype(np.float32)
                live = live & is_depth(zf)
                zi = c / ((m[0] * (xd + 1.0) + m[1] * yd) + m[2])
                zj = c / ((m[0] * xd + m[1] * (yd + 1.0)) + m[2])
            q = np.nonzero(live)[0]
            if not len(q):
                continue
            with np.errstate(all="ignore"):
                Xc = backproject_d(vw, r, xd[q], yd[q], zc[q])
                Xi = backproject_d(vw, r, xd[q] + 1.0, yd[q], zi[q])
                Xj = backproject_d(vw, r, xd[q], yd[q] + 1.0, zj[q])
            ncc = np.full((len(q), max(len(src[k]), top_k)), -np.inf)  # fewer sources than top_k: no candidate
            nvalid = np.zeros(len(q), np.int64)
            for si, s in enumerate(src[k]):
                ok, v = source_ncc(vw, r, s, x[q], y[q], Xc, Xi, Xj, window, Sa[q], Saa[q], Aref[q], dmin)
                ncc[:, si] = v
                nvalid += ok
            st["source_scores"] += int(nvalid.sum())
            if ci == 0:
                valid0[q] = nvalid
            desc = -np.sort(-ncc, axis=1, kind="stable")
            has = nvalid >= top_k
            with np.errstate(all="ignore"):
                S = desc[:, 0].copy()
                for t_ in range(1, top_k):
                    S = S + desc[:, t_]
                score = S / np.float64(top_k)
            st["candidates"] += int(has.sum())
            ncand[q[has]] += 1
            win = has & ((choice[q] < 0) | (score > best[q]))
            qq = q[win]
            best[qq], choice[qq], wz[qq], wn[qq] = score[win], ci, zf[qq], cn[qq]
        scored = choice >= 0
        kept = scored & (best >= thr)
        oz = np.where(kept, wz, F32(0)).astype(np.float32)
        on = np.where(kept[:, None], wn, F32(0)).astype(np.float32)
        os_ = np.where(kept, best, 0.0).astype(np.float32)
        oc = np.where(kept, choice, -1).astype(np.int32)
        if flags & KEEP_UNSCORED:
            keep = ~scored & own_depth
            oz[keep], on[keep], oc[keep] = z[keep], n[keep], -2
        planes = [np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32),
                  np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int64), np.zeros((H, W), np.int64)]
        for plane, val in zip(planes, (oz, on, os_, oc, valid0, ncand)):
            plane[y, x] = val
        for key, plane in zip(("depth", "normal", "score", "choice", "valid", "ncand"), planes):
            out[key].append(plane)
        st["depth_pixels_in"] += int(own_depth.sum())
        st["kept"] += int(kept.sum())
        st["filled"] += int((kept & ~own_depth).sum())
        st["moved"] += int((kept & (choice != 0)).sum())
    out["stats"] = st
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
