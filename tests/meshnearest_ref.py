"""CPU reference of dp_mesh_nearest: a brute-force numpy restatement of the spec
in include/densepoints.h -- the box test first, then the pairs that pass it in
fp64 in the written order (numpy's elementwise fp64 operations are one IEEE
rounding each), the inclusive radius, ties to the lowest triangle index -- with
the histogram and the statistics the spec defines (not the grid's facts or the
times)."""
import numpy as np

from cloudnearest_ref import positions, same_bits  # noqa: F401  (same_bits is part of this module's interface)

COUNTS = ("queries", "skipped_queries", "matched", "unmatched", "triangles", "invalid_triangles",
          "degenerate_triangles", "nonfinite_triangles")
# who answered for a pair: the plane, the inside of a segment, or a segment's end
LABELS = ("face", "edge_ab", "edge_bc", "edge_ca", "vertex_a", "vertex_b", "vertex_c")


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def pair_distance(q, a, b, c) -> dict:
    """The spec's distance of q[i] to the triangle (a[i], b[i], c[i]), all (m, 3)
    fp64: d2, the float32 point, the label of the part that answered and
    whether the plane passed its conditioning test."""
    with np.errstate(all="ignore"):
        ab, ac, bc, ca = b - a, c - a, c - b, a - c
        ap, bp, cp = q - a, q - b, q - c
        m = len(q)
        d2 = np.full(m, np.inf)
        pt = np.full((m, 3), np.inf, np.float32)
        label = np.full(m, -1, np.int64)
        n = cross(ab, ac)
        nn = dot(n, n)
        conditioned = nn > (dot(ab, ab) * dot(ac, ac)) * 2.0 ** -40
        use = conditioned & (dot(cross(ab, ap), n) >= 0) & (dot(cross(bc, bp), n) >= 0) & (dot(cross(ca, cp), n) >= 0)
        s = np.where(use, dot(ap, n) / np.where(use, nn, 1.0), 0.0)
        r = s[:, None] * n
        d2[use] = dot(r, r)[use]
        pt[use] = (q - r).astype(np.float32)[use]
        label[use] = 0
        for k, (st, se, sp, ends) in enumerate(((a, ab, ap, (4, 5)), (b, bc, bp, (5, 6)), (c, ca, cp, (6, 4)))):
            den = dot(se, se)
            pos = den > 0
            t = np.where(pos, dot(sp, se) / np.where(pos, den, 1.0), 0.0)
            t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
            r = sp - t[:, None] * se
            e2 = dot(r, r)
            better = e2 < d2
            d2[better] = e2[better]
            pt[better] = (st + t[:, None] * se).astype(np.float32)[better]
            label[better] = np.where(t == 0, ends[0], np.where(t == 1, ends[1], 1 + k))[better]
    return {"d2": d2, "point": pt, "label": label, "conditioned": conditioned}


def classify(vertices, triangles):
    """per triangle: 0 takes part, 1 invalid, 2 degenerate, 3 non-finite"""
    v32 = positions(vertices)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    cls = np.zeros(len(tri), np.int64)
    valid = ((tri >= 0) & (tri < len(v32))).all(axis=1)
    cls[~valid] = 1
    safe = np.where(valid[:, None], tri, 0)
    degenerate = valid & ((safe[:, 0] == safe[:, 1]) | (safe[:, 1] == safe[:, 2]) | (safe[:, 0] == safe[:, 2]))
    cls[degenerate] = 2
    if len(v32):
        finite = np.isfinite(v32[safe]).all(axis=(1, 2))
    else:
        finite = np.ones(len(tri), bool)
    cls[valid & ~degenerate & ~finite] = 3
    return cls


def nearest(queries, vertices, triangles, max_dist, hist_bins=0, chunk=256) -> dict:
    q32, v32 = positions(queries), positions(vertices)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    cls = classify(vertices, triangles)
    tid = np.flatnonzero(cls == 0)
    qpart = np.isfinite(q32).all(axis=1)
    R = float(np.float32(max_dist))
    R2 = R * R
    G = R + R * 2.0 ** -20
    nq = len(q32)
    index = np.full(nq, -1, np.int32)
    dist = np.full(nq, np.inf, np.float32)
    closest = np.full((nq, 3), np.inf, np.float32)
    best_d2 = np.full(nq, np.inf)
    label = np.full(nq, -1, np.int64)
    if len(tid):
        P32 = v32[tri[tid]]  # (T, 3 corners, 3 axes)
        P = P32.astype(np.float64)
        lo = P32.min(axis=1).astype(np.float64) - G
        hi = P32.max(axis=1).astype(np.float64) + G
        for at in range(0, nq, chunk):
            sel = np.flatnonzero(qpart[at:at + chunk]) + at
            if not len(sel):
                continue
            qq = q32[sel].astype(np.float64)
            box = ((lo[None, :, :] <= qq[:, None, :]) & (qq[:, None, :] <= hi[None, :, :])).all(axis=2)
            qi, ti = np.nonzero(box)
            if not len(qi):
                continue
            r = pair_distance(qq[qi], P[ti, 0], P[ti, 1], P[ti, 2])
            D = np.full(box.shape, np.inf)
            ok = r["d2"] <= R2
            D[qi[ok], ti[ok]] = r["d2"][ok]
            win = D.argmin(axis=1)  # the first of equal minima: the lowest index (tid ascends)
            bd2 = D[np.arange(len(sel)), win]
            hit = np.isfinite(bd2)
            where = np.full(box.shape, -1, np.int64)
            where[qi, ti] = np.arange(len(qi))
            pair = where[np.arange(len(sel)), win][hit]
            index[sel[hit]] = tid[win[hit]].astype(np.int32)
            dist[sel[hit]] = np.sqrt(bd2[hit]).astype(np.float32)
            closest[sel[hit]] = r["point"][pair]
            best_d2[sel[hit]] = bd2[hit]
            label[sel[hit]] = r["label"][pair]
    matched = index >= 0
    hist = None
    if hist_bins:
        b = np.floor(dist[matched].astype(np.float64) / R * float(hist_bins)).astype(np.int64)
        hist = np.bincount(np.minimum(hist_bins - 1, b), minlength=hist_bins).astype(np.uint64)
    nqp = int(qpart.sum())
    stats = dict(queries=nqp, skipped_queries=nq - nqp, matched=int(matched.sum()), unmatched=nqp - int(matched.sum()),
                 triangles=int((cls == 0).sum()), invalid_triangles=int((cls == 1).sum()),
                 degenerate_triangles=int((cls == 2).sum()), nonfinite_triangles=int((cls == 3).sum()))
    return {"index": index, "dist": dist, "closest": closest, "hist": hist, "stats": stats, "d2": best_d2,
            "label": label}


def seven_region_case():
    """One triangle and 28 planted queries, four for each of its seven regions
    in the order of LABELS; returns (queries, vertices, triangles, max_dist,
    the label every query must get)."""
    v = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]])
    spots = {
        0: [[1, 1, 0.5], [0.5, 2, -1], [2, 1, 2], [1, 0.25, 0]],
        1: [[2, -1, 0.5], [1, -2, 0], [3, -0.5, -1], [0.5, -0.25, 0.25]],
        2: [[3, 3, 0.25], [2.5, 2, 1], [4, 1, 0], [1.5, 3.5, -0.5]],
        3: [[-1, 2, 0], [-2, 1, 0.5], [-0.5, 3, -1], [-0.25, 0.5, 0.25]],
        4: [[-1, -1, 0], [-0.5, -2, 1], [-2, -0.25, -0.5], [-1, -1, -1]],
        5: [[6, -0.5, 0.5], [5, -1, 0], [5.5, -0.25, -1], [6, -1, 1]],
        6: [[-0.5, 6, 0], [-1, 5, 0.5], [-0.25, 5.5, -1], [-1, 6, 1]],
    }
    q = np.float32([p for k in range(7) for p in spots[k]])
    want = np.repeat(np.arange(7), 4)
    return q, v, np.int32([[0, 1, 2]]), 4.0, want
