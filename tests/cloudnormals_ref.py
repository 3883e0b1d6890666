"""CPU reference of dp_cloud_normals: the spec in include/densepoints.h restated
in numpy with fp64 scalars -- cloudknn_ref.knn for the neighbourhoods, the mean
and the six scatter sums term by term in rank order, the cyclic Jacobi sweeps of
the 3 x 3 matrix written out scalar by scalar, the canonical sign and the
orientation -- returning the dict the Engine returns (without grid_cells,
max_cell_targets and the times)."""
import os
import re

import numpy as np

from cloudnearest_ref import positions, same_bits  # noqa: F401
from cloudknn_ref import knn

COUNTS = ("points", "skipped", "estimated", "sparse", "degenerate", "flipped", "unoriented")
PAIRS = ((0, 1), (0, 2), (1, 2))
ORIENT_NONE, ORIENT_VIEWPOINT, ORIENT_DIRECTION = 0, 1, 2

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "densepoints.h")) as _f:
    SWEEPS = int(re.search(r"#define DP_CLOUD_NORMALS_SWEEPS (\d+)", _f.read()).group(1))

F = np.float64


def off_mass(N) -> float:
    """sqrt(sum of N_pq^2, p < q)"""
    return float(np.sqrt(sum(N[p][q] * N[p][q] for p, q in PAIRS)))


def jacobi(N, sweeps=SWEEPS, trace=None):
    """the header's cyclic Jacobi on a 3 x 3 list of lists; returns (N, V).
    trace: a list that gets the off-diagonal mass after every sweep"""
    N = [[F(v) for v in row] for row in N]
    V = [[F(1.0) if r == k else F(0.0) for k in range(3)] for r in range(3)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = N[p][q]
            if apq == 0.0:
                continue
            with np.errstate(over="ignore"):
                theta = (N[q][q] - N[p][p]) / (F(2.0) * apq)
                t = F(1.0 if theta >= 0 else -1.0) / (np.abs(theta) + np.sqrt(theta * theta + F(1.0)))
            c = F(1.0) / np.sqrt(t * t + F(1.0))
            s = t * c
            k = 3 - p - q
            u, w = N[k][p], N[k][q]
            N[k][p] = N[p][k] = c * u - s * w
            N[k][q] = N[q][k] = s * u + c * w
            h = t * apq
            N[p][p] = N[p][p] - h
            N[q][q] = N[q][q] + h
            N[p][q] = N[q][p] = F(0.0)
            for k in range(3):
                u, w = V[k][p], V[k][q]
                V[k][p] = c * u - s * w
                V[k][q] = s * u + c * w
        if trace is not None:
            trace.append(off_mass(N))
    return N, V


def scatter(p64, order=None):
    """the mean and the six sums of the rows of p64 (c x 3 float64) in the given
    order (None = as they stand, the spec's rank order): (m, [xx, xy, xz, yy, yz, zz], T)"""
    rows = list(range(len(p64))) if order is None else list(order)
    c = len(rows)
    m = []
    for a in range(3):
        s = p64[rows[0], a]
        for j in rows[1:]:
            s = s + p64[j, a]
        m.append(s / F(c))
    C = []
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        s = None
        for j in rows:
            term = (p64[j, a] - m[a]) * (p64[j, b] - m[b])
            s = term if s is None else s + term
        C.append(s)
    return m, C, (C[0] + C[3]) + C[5]


def eigen(C, T, sweeps=SWEEPS, trace=None):
    """the unit eigenvector with the canonical sign (three float64) and the variation (float32)"""
    N, V = jacobi([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]], sweeps, trace)
    j = 0
    for k in (1, 2):
        if N[k][k] < N[j][j]:
            j = k
    v = [V[k][j] for k in range(3)]
    length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    u = [x / length for x in v]
    variation = np.float32((N[j][j] if N[j][j] > 0 else F(0.0)) / T)  # fmax(N_jj, 0.0): +0.0 unless N_jj > 0
    a = 0
    for k in (1, 2):
        if np.abs(u[k]) > np.abs(u[a]):
            a = k
    if u[a] < 0:
        u = [-x for x in u]
    return u, variation


def toward_entries(toward, n):
    """one xyz or n of them as an n x 3 float32 array"""
    w = np.asarray(toward, np.float32)
    return np.broadcast_to(w.reshape(-1, 3), (n, 3)) if w.size == 3 else w.reshape(n, 3)


def normals(points, k, max_dist, min_neighbours=3, orient=ORIENT_NONE, toward=None, sweeps=SWEEPS, traces=None,
            order=None) -> dict:
    """`points`: packed n x 3 or a structured array with pos.  toward: one xyz or
    n x 3 float32 (required with an orient mode).  traces: a list that gets the
    per-sweep off-diagonal masses and T of every estimated point.  order: a
    function of a row's length giving another summation order (None = rank order)"""
    p32 = positions(points)
    n = len(p32)
    res = knn(points, points, k, max_dist)
    index, count = res["index"], res["count"].copy()
    part = np.isfinite(p32).all(axis=1)
    normal = np.zeros((n, 3), np.float32)
    variation = np.full(n, np.inf, np.float32)
    w32 = toward_entries(toward, n) if orient else None
    st = dict.fromkeys(COUNTS, 0)
    st["points"] = int(part.sum())
    st["skipped"] = n - st["points"]
    p64 = p32.astype(F)
    for i in range(n):
        if not part[i]:
            continue
        c = int(count[i])
        if c < min_neighbours:
            st["sparse"] += 1
            continue
        nb = p64[index[i, :c]]
        _, C, T = scatter(nb, None if order is None else order(c))
        if T == 0.0:
            st["degenerate"] += 1
            continue
        st["estimated"] += 1
        tr = [] if traces is not None else None
        u, variation[i] = eigen(C, T, sweeps, tr)
        if traces is not None:
            traces.append((tr, float(T)))
        if orient:
            w = w32[i].astype(F)
            x = p64[i]
            with np.errstate(invalid="ignore", over="ignore"):
                if orient == ORIENT_VIEWPOINT:
                    s = ((w[0] - x[0]) * u[0] + (w[1] - x[1]) * u[1]) + (w[2] - x[2]) * u[2]
                else:
                    s = (w[0] * u[0] + w[1] * u[1]) + w[2] * u[2]
            if np.isfinite(w32[i]).all() and s < 0:
                u = [-v for v in u]
                st["flipped"] += 1
            elif not np.isfinite(w32[i]).all() or s == 0:
                st["unoriented"] += 1
        normal[i] = np.array(u, F).astype(np.float32)
    return {"normal": normal, "variation": variation, "count": count, "stats": st}


def normal_error(recon_normals, truth_normals, index, dist, tau) -> dict:
    """cloud_normal_error restated: the unsigned angle, in degrees and fp64,
    between a query's normal and its matched truth normal over the queries with
    index >= 0, dist <= tau and both normals finite and non-zero"""
    a = np.asarray(recon_normals, F).reshape(-1, 3)
    t = np.asarray(truth_normals, F).reshape(-1, 3)
    index, dist = np.asarray(index), np.asarray(dist)
    angles = []
    for i in range(len(a)):
        if index[i] < 0 or not dist[i] <= tau:
            continue
        b = t[index[i]]
        if not (np.isfinite(a[i]).all() and np.isfinite(b).all() and a[i].any() and b.any()):
            continue
        dot = np.abs((a[i, 0] * b[0] + a[i, 1] * b[1]) + a[i, 2] * b[2])
        la = np.sqrt((a[i, 0] * a[i, 0] + a[i, 1] * a[i, 1]) + a[i, 2] * a[i, 2])
        lb = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        angles.append(np.degrees(np.arccos(min(F(1.0), dot / (la * lb)))))
    d = np.sort(np.array(angles, F))

    def quantile(p):
        pos = p * (len(d) - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, len(d) - 1)
        return float(d[lo] + (d[hi] - d[lo]) * (pos - lo))

    if not len(d):
        return {"n": 0, "mean_deg": float("nan"), "median_deg": float("nan"), "p90_deg": float("nan")}
    return {"n": len(d), "mean_deg": float(np.array(angles, F).mean()), "median_deg": quantile(0.5),
            "p90_deg": quantile(0.9)}
