"""CPU reference of dp_cloud_nearest: a brute-force numpy restatement of the
spec in include/densepoints.h -- fp64 in the written order, the inclusive radius,
ties to the lowest index -- with the histogram, the statistics the spec defines
(not grid_cells, max_cell_targets or the times) and cloud_compare."""
import numpy as np

COUNTS = ("queries", "targets", "skipped_queries", "skipped_targets", "matched", "unmatched")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def positions(cloud) -> np.ndarray:
    """the n x 3 float32 positions of a packed or a structured cloud"""
    cloud = np.asarray(cloud)
    if cloud.dtype.names:
        cloud = cloud["pos"]
    return np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)


def nearest(queries, targets, max_dist, hist_bins=0, chunk=256) -> dict:
    q32, t32 = positions(queries), positions(targets)
    q, t = q32.astype(np.float64), t32.astype(np.float64)
    qpart, tpart = np.isfinite(q32).all(axis=1), np.isfinite(t32).all(axis=1)
    R = float(np.float32(max_dist))
    R2 = R * R
    nq = len(q)
    index = np.full(nq, -1, np.int32)
    dist = np.full(nq, np.inf, np.float32)
    tid = np.flatnonzero(tpart)
    tt = t[tid]
    if len(tid):
        for lo in range(0, nq, chunk):
            sel = np.flatnonzero(qpart[lo:lo + chunk]) + lo
            if not len(sel):
                continue
            qq = q[sel]
            dx = qq[:, None, 0] - tt[None, :, 0]
            dy = qq[:, None, 1] - tt[None, :, 1]
            dz = qq[:, None, 2] - tt[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 <= R2, d2, np.inf)
            best = d2.argmin(axis=1)  # the first of equal minima: the lowest index (tid ascends)
            bd2 = d2[np.arange(len(sel)), best]
            hit = np.isfinite(bd2)
            index[sel[hit]] = tid[best[hit]].astype(np.int32)
            dist[sel[hit]] = np.sqrt(bd2[hit]).astype(np.float32)
    matched = index >= 0
    hist = None
    if hist_bins:
        b = np.floor(dist[matched].astype(np.float64) / R * float(hist_bins)).astype(np.int64)
        hist = np.bincount(np.minimum(hist_bins - 1, b), minlength=hist_bins).astype(np.uint64)
    nqp, ntp = int(qpart.sum()), int(tpart.sum())
    stats = dict(queries=nqp, targets=ntp, skipped_queries=nq - nqp, skipped_targets=len(t) - ntp,
                 matched=int(matched.sum()), unmatched=nqp - int(matched.sum()))
    return {"index": index, "dist": dist, "hist": hist, "stats": stats}


def quantile(sorted_d, p):
    m = len(sorted_d)
    if m == 0:
        return float("nan")
    pos = p * (m - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, m - 1)
    return float(sorted_d[lo] + (sorted_d[hi] - sorted_d[lo]) * (pos - lo))


def side(res, tau) -> dict:
    d = np.sort(res["dist"][res["index"] >= 0].astype(np.float64))
    n, within = res["stats"]["queries"], int((d <= tau).sum())
    return {"n": n, "matched": res["stats"]["matched"], "within_tau": within, "ratio": within / n if n else 0.0,
            "mean": float(np.sum(d) / len(d)) if len(d) else float("nan"), "median": quantile(d, 0.5),
            "p90": quantile(d, 0.9)}


def compare(recon, truth, tau, max_dist=None) -> dict:
    max_dist = 10.0 * tau if max_dist is None else max_dist
    acc, com = side(nearest(recon, truth, max_dist), tau), side(nearest(truth, recon, max_dist), tau)
    p, r = acc["ratio"], com["ratio"]
    return {"accuracy": acc, "completeness": com, "fscore": 2.0 * p * r / (p + r) if p + r > 0 else 0.0}


def assert_compare(got, want, rel=1e-9):
    """two cloud_compare results: the integers exactly, the floats to `rel`"""
    assert set(got) == set(want)
    for name in ("accuracy", "completeness"):
        g, w = got[name], want[name]
        assert set(g) == set(w) == {"n", "matched", "within_tau", "ratio", "mean", "median", "p90"}, name
        for k in ("n", "matched", "within_tau"):
            assert g[k] == w[k], (name, k)
        for k in ("ratio", "mean", "median", "p90"):
            assert (np.isnan(g[k]) and np.isnan(w[k])) or abs(g[k] - w[k]) <= rel * abs(w[k]), (name, k, g[k], w[k])
    assert abs(got["fscore"] - want["fscore"]) <= rel * abs(want["fscore"])
