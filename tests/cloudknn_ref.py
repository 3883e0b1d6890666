"""CPU reference of dp_cloud_knn and dp_cloud_clean: a brute-force numpy
restatement of the two specs in include/densepoints.h -- the full fp64 distance
matrix in the written order, the inclusive radius, the order (d2, index) by
np.lexsort, the balanced pairwise sum -- with the statistics the specs define
(not grid_cells, max_cell_targets or the times)."""
import numpy as np

from cloudnearest_ref import positions, same_bits  # noqa: F401

KNN_COUNTS = ("queries", "targets", "skipped_queries", "skipped_targets", "full", "partial", "empty", "neighbours")
CLEAN_COUNTS = ("points", "skipped", "eligible", "kept", "removed_sparse", "removed_far")


def pairwise_sum(x) -> float:
    """S of the spec: +0.0 up to the next power of two, then adjacent pairs"""
    x = np.asarray(x, np.float64).reshape(-1)
    size = 1
    while size < len(x):
        size *= 2
    x = np.concatenate([x, np.zeros(size - len(x))])
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


def knn_d2(queries, targets, k, max_dist, exclude_self=False, chunk=256):
    """index (n x k int32), the neighbours' d2 (n x k float64, inf = none), count
    (int32), and who takes part on either side"""
    q32, t32 = positions(queries), positions(targets)
    q, t = q32.astype(np.float64), t32.astype(np.float64)
    qpart, tpart = np.isfinite(q32).all(axis=1), np.isfinite(t32).all(axis=1)
    R = float(np.float32(max_dist))
    R2 = R * R
    nq, nt = len(q), len(t)
    assert not exclude_self or nq == nt
    index = np.full((nq, k), -1, np.int32)
    d2out = np.full((nq, k), np.inf, np.float64)
    count = np.zeros(nq, np.int32)
    tid = np.arange(nt)
    for lo in range(0, nq if nt else 0, chunk):
        hi = min(lo + chunk, nq)
        with np.errstate(invalid="ignore", over="ignore"):
            dx = q[lo:hi, None, 0] - t[None, :, 0]
            dy = q[lo:hi, None, 1] - t[None, :, 1]
            dz = q[lo:hi, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            cand = (d2 <= R2) & qpart[lo:hi, None] & tpart[None, :]
        if exclude_self:
            cand[np.arange(hi - lo), np.arange(lo, hi)] = False
        for r in range(hi - lo):
            who = tid[cand[r]]
            if not len(who):
                continue
            order = np.lexsort((who, d2[r, who]))[:k]  # the last key is the primary one
            c = len(order)
            index[lo + r, :c] = who[order]
            d2out[lo + r, :c] = d2[r, who[order]]
            count[lo + r] = c
    return index, d2out, count, qpart, tpart


def knn(queries, targets, k, max_dist, exclude_self=False) -> dict:
    index, d2, count, qpart, tpart = knn_d2(queries, targets, k, max_dist, exclude_self)
    dist = np.sqrt(d2).astype(np.float32)
    nqp, ntp = int(qpart.sum()), int(tpart.sum())
    c = count[qpart]
    stats = dict(queries=nqp, targets=ntp, skipped_queries=len(qpart) - nqp, skipped_targets=len(tpart) - ntp,
                 full=int((c == k).sum()), partial=int(((c > 0) & (c < k)).sum()), empty=int((c == 0).sum()),
                 neighbours=int(count.sum()))
    return {"index": index, "dist": dist, "count": count, "stats": stats}


def clean(points, k, max_dist, std_mul=2.0, min_neighbours=1, radius_only=False) -> dict:
    """`points`: packed n x 3 or a structured array whose records move whole"""
    points = np.asarray(points)
    _, d2, count, part, _ = knn_d2(points, points, k, max_dist, exclude_self=True)
    n = len(count)
    d = np.sqrt(d2)
    m = np.full(n, np.inf, np.float64)
    for i in range(n):
        c = int(count[i])
        if c:
            s = d[i, 0]
            for j in range(1, c):
                s = s + d[i, j]
            m[i] = s / np.float64(c)
    eligible = part & (count >= min_neighbours)
    N = int(eligible.sum())
    mu = sigma = T = 0.0
    if not radius_only and N > 0:
        x = np.where(eligible, m, 0.0)
        mu = pairwise_sum(x) / np.float64(N)
        dev = np.where(eligible, m, mu) - mu
        y = np.where(eligible, dev * dev, 0.0)
        var = pairwise_sum(y) / np.float64(N - 1) if N >= 2 else np.float64(0.0)
        sigma = np.sqrt(var)
        T = mu + np.float64(np.float32(std_mul)) * sigma
    keep = eligible & (True if radius_only else (m <= T))
    where = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    stats = dict(points=int(part.sum()), skipped=n - int(part.sum()), eligible=N, kept=int(keep.sum()),
                 removed_sparse=int((part & ~eligible).sum()), removed_far=int((eligible & ~keep).sum()))
    with np.errstate(over="ignore"):
        mean32 = m.astype(np.float32)
    return {"keep": keep.astype(np.uint8), "mean_dist": mean32, "map": where, "points": points[keep].copy(),
            "stats": stats, "mu": float(mu), "sigma": float(sigma), "threshold": float(T)}
