"""The stages of seed generation after the detector, restated in plain numpy
from the reference's modules/features/matcher.cpp:185-450 and the orders
include/densepoints.h states -- not from oracle/or_seeds.c, which it checks
(tests/test_seedstage_cpu.py), nor from the kernels.

    DefaultPairsList          every pair (i < j), i-major             (185-204)
    MatchKeypoints, kNN       brute-force Hamming top-2, ties by (distance,
                              index); kept iff d0 < ratio * d1 in float (206-226)
    MatchKeypoints, FLANN     the exact nearest neighbour, kept iff d0 < 30
                              in float                                 (227-240)
    DirectEpipolarMatching    every (query, train) with dist <= max    (267-317)
    FilterMatches             a kept match is erased iff dist > max    (319-372)
    GetAllMatches             per pair the FIRST match in list order: from the
                              query side the lowest train index (q2t), from the
                              train side the lowest query index (t2q)  (374-413)
    TriangulateMatches        per (view, keypoint) with a match: itself, then
                              one observation per pair in list order, each as
                              cv::Point (rounded half to even)         (415-450)

knnMatch with k = 2 leaves the second entry undefined on fewer than two train
rows and match() has nothing to return on none: the product defines both as
"no match" (include/densepoints.h), and so does this file.

Two operations are taken as callables, both pinned against numpy elsewhere
(tests/test_seeds_cpu.py): the fundamental matrix of a pair, whose bits decide
an epipolar distance at its bound, and the DLT of an observation list."""
import numpy as np

KNN, FLANN = 0, 1
_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def hamming(q, t):
    """(nq x nt) Hamming distances of byte rows"""
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    out = np.zeros((len(q), len(t)), dtype=np.int32)
    for a in range(0, len(q), 256):
        out[a:a + 256] = _POP[q[a:a + 256, None, :] ^ t[None, :, :]].sum(axis=2)
    return out


def top2(q, t):
    """(idx2, dist2) of the two nearest train rows of every query by
    (distance, index); -1 where the train set has no such row"""
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, dtype=np.int32)
    dist = np.full((nq, 2), -1, dtype=np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    d = hamming(q, t).astype(np.int64)
    key = d * nt + np.arange(nt, dtype=np.int64)[None, :]
    order = np.sort(key, axis=1)[:, :2]
    k = order.shape[1]
    idx[:, :k] = order % nt
    dist[:, :k] = order // nt
    return idx, dist


def epipolar_distance(F, x1, y1, x2, y2):
    """Distance (float) of (x2, y2) to the epipolar line of (x1, y1), arrays
    broadcast: LineFromFundamentalMatrix (fundamental_matrix.cpp:37-53: the
    line F (x1, y1, 1) in fp64, its y at x = 0 and at x = 1 stored as float) and
    ParametrizedLine::Through(...).distance() in fp64, the result a float."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    px, py = np.asarray(x1, dtype=np.float32).astype(np.float64), np.asarray(y1, dtype=np.float32).astype(np.float64)
    qx, qy = np.asarray(x2, dtype=np.float32).astype(np.float64), np.asarray(y2, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        l0 = (F[0] * px + F[1] * py) + F[2]
        l1 = (F[3] * px + F[4] * py) + F[5]
        l2 = (F[6] * px + F[7] * py) + F[8]
        y_1 = (-l2 / l1).astype(np.float32).astype(np.float64)
        y_2 = ((-l2 - l0) / l1).astype(np.float32).astype(np.float64)
        dy0 = y_2 - y_1
        nrm = np.sqrt(1.0 + dy0 * dy0)
        dx, dy = 1.0 / nrm, dy0 / nrm
        fx, fy = qx - 0.0, qy - y_1
        dt = dx * fx + dy * fy
        vx, vy = fx - dt * dx, fy - dt * dy
        return np.sqrt(vx * vx + vy * vy).astype(np.float32)


def ratio_pass(dist2, nt, matcher_type, ratio):
    """the kNN ratio test / FLANN's distance test of every query, in float"""
    d0 = dist2[:, 0].astype(np.float32)
    d1 = dist2[:, 1].astype(np.float32)
    if matcher_type == FLANN:
        return (d0 < np.float32(30.0)) if nt >= 1 else np.zeros(len(d0), dtype=bool)
    if nt < 2:
        return np.zeros(len(d0), dtype=bool)
    return d0 < np.float32(ratio) * d1


def match_pair(F, kq, kt, dq, dt, opts):
    """One pair: q2t, t2q, (ratio matches, matches) and what decided them
    (info: top-2, the ratio mask and the distances that were tested)"""
    nq, nt = len(kq), len(kt)
    max_dist = np.float32(opts.get("max_epipolar_distance", 1.5))
    q2t = np.full(nq, -1, dtype=np.int32)
    t2q = np.full(nt, -1, dtype=np.int32)
    info = {}
    if opts.get("epipolar_matching", False):
        if nq == 0 or nt == 0:
            info.update(dist=np.zeros((nq, nt), dtype=np.float32), accepted=np.zeros((nq, nt), dtype=bool))
            return q2t, t2q, (0, 0), info
        dist = epipolar_distance(F, kq["x"][:, None], kq["y"][:, None], kt["x"][None, :], kt["y"][None, :])
        ok = dist <= max_dist  # matcher.cpp:288: a NaN distance is no match
        info.update(dist=dist, accepted=ok)
        has_q, has_t = ok.any(axis=1), ok.any(axis=0)
        q2t[has_q] = ok.argmax(axis=1)[has_q]
        t2q[has_t] = ok.argmax(axis=0)[has_t]
        n = int(ok.sum())
        return q2t, t2q, (n, n), info
    idx2, dist2 = top2(dq, dt)
    rp = ratio_pass(dist2, nt, opts.get("matcher_type", KNN), opts.get("nn_match_ratio", 0.7))
    qi = np.flatnonzero(rp)
    ti = idx2[qi, 0]
    dist = epipolar_distance(F, kq["x"][qi], kq["y"][qi], kt["x"][ti], kt["y"][ti])
    keep = ~(dist > max_dist)  # matcher.cpp:343: erased iff greater, so a NaN distance stays
    info.update(idx2=idx2, dist2=dist2, ratio_pass=rp, queries=qi, dist=dist, accepted=keep)
    q2t[qi[keep]] = ti[keep]
    for q, t in zip(qi[keep], ti[keep]):  # ascending q: the first in list order stays
        if t2q[t] < 0:
            t2q[t] = q
    return q2t, t2q, (len(qi), int(keep.sum())), info


def run(P, counts, kp, desc, opts, fundamental, triangulate):
    """All stages on planted keypoints: counts[v] keypoints per view (structured
    rows with x and y, view-major), desc one byte row each.  Returns pairs,
    q2t / t2q / info per pair, counts, tracks -- per (view, keypoint) with a
    match the list of (view, keypoint, x, y) it is triangulated from, itself
    first -- and the points."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    V = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    view = lambda a, v: a[off[v]:off[v + 1]]
    out = {"pairs": [], "q2t": [], "t2q": [], "info": []}
    ratio_matches = matches = 0
    for i in range(V):
        for j in range(i + 1, V):
            F = fundamental(P[i], P[j])
            q2t, t2q, (nr, nm), info = match_pair(F, view(kp, i), view(kp, j), view(desc, i), view(desc, j), opts)
            out["pairs"].append((i, j))
            out["q2t"].append(q2t)
            out["t2q"].append(t2q)
            out["info"].append(info)
            ratio_matches += nr
            matches += nm
    rx = np.rint(kp["x"].astype(np.float32)).astype(np.float32)  # cv::Point(Point2f): cvRound, half to even
    ry = np.rint(kp["y"].astype(np.float32)).astype(np.float32)
    tracks = []
    for v in range(V):
        for k in range(counts[v]):
            obs = [(v, k, float(rx[off[v] + k]), float(ry[off[v] + k]))]
            for p, (a, b) in enumerate(out["pairs"]):
                if a == v:
                    o, ov = out["q2t"][p][k], b
                elif b == v:
                    o, ov = out["t2q"][p][k], a
                else:
                    continue
                if o >= 0:
                    obs.append((ov, int(o), float(rx[off[ov] + o]), float(ry[off[ov] + o])))
            if len(obs) >= 2:
                tracks.append(obs)
    if tracks:
        points = triangulate([[P[o[0]] for o in t] for t in tracks], [[(o[2], o[3]) for o in t] for t in tracks])
    else:
        points = np.zeros((0, 3))
    out["tracks"] = tracks
    out["points"] = points
    out["counts"] = {"pairs": len(out["pairs"]), "ratio_matches": ratio_matches, "matches": matches,
                     "points": len(tracks)}
    return out
