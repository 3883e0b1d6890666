"""CPU reference of dp_cloud_transform and dp_cloud_align: a brute-force
restatement of the two specs in include/densepoints.h in numpy with fp64
scalars -- the transform's expression, cloudnearest_ref.nearest for the matches,
cloudknn_ref.pairwise_sum for every sum, Horn's matrix and the cyclic Jacobi
sweeps written out scalar by scalar -- returning the dicts the Engine returns
(without grid_cells, max_cell_targets and the times)."""
import re
import os

import numpy as np

from cloudnearest_ref import nearest, positions, same_bits  # noqa: F401
from cloudknn_ref import pairwise_sum

COUNTS = ("queries", "targets", "skipped_queries", "skipped_targets", "matched", "unmatched", "iterations_run",
          "stop_reason")
STOP_ITERATIONS, STOP_RMS, STOP_PAIRS, STOP_DEGENERATE, STOP_EMPTY = range(5)
STEP_DTYPE = np.dtype([("matched", "<i8"), ("rms", "<f8")])
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
IDENTITY = np.eye(3, 4)

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "densepoints.h")) as _f:
    SWEEPS = int(re.search(r"#define DP_CLOUD_ALIGN_SWEEPS (\d+)", _f.read()).group(1))

F = np.float64


def transform_positions(p32, M):
    """fl32(A x + t) of the finite rows of an n x 3 float32 array; the others as they are"""
    M = np.asarray(M, F).reshape(3, 4)
    p32 = np.ascontiguousarray(p32, np.float32).reshape(-1, 3)
    out = p32.copy()
    part = np.isfinite(p32).all(axis=1)
    x, y, z = (p32[part, k].astype(F) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            out[part, r] = (((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]).astype(np.float32)
    return out


def transform(points, matrix, normals=False):
    """dp_cloud_transform: `points` packed n x 3 or a structured array with pos
    (and, with normals, normal); the records are returned whole"""
    points = np.asarray(points)
    M = np.asarray(matrix, F).reshape(3, 4)
    if not points.dtype.names:
        assert not normals
        return transform_positions(points, M)
    out = points.copy().reshape(-1)
    out["pos"] = transform_positions(points["pos"], M)
    if normals:
        n = points["normal"].reshape(-1, 3).astype(F)
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.stack([(M[r, 0] * n[:, 0] + M[r, 1] * n[:, 1]) + M[r, 2] * n[:, 2] for r in range(3)], axis=1)
            length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            good = np.isfinite(length) & (length > 0)
            new = (v[good] / length[good, None]).astype(np.float32)
        nn = out["normal"].reshape(-1, 3).copy()
        nn[good] = new
        out["normal"] = nn
    return out


def channel_sums(terms):
    """the pairwise sum of every column of an n x C array of terms"""
    terms = np.asarray(terms, F)
    return [pairwise_sum(terms[:, ch]) for ch in range(terms.shape[1])]


def tree_levels(terms):
    """The same sums as the device makes them: levels of 2^8, each block the
    balanced tree of its 256 terms (+0.0 padded); a list of C values"""
    x = np.asarray(terms, F)
    if x.ndim == 1:
        x = x[:, None]
    while True:
        blocks = (len(x) + 255) // 256
        pad = np.zeros((blocks * 256 - len(x), x.shape[1]))
        y = np.concatenate([x, pad]).reshape(blocks, 256, -1)
        while y.shape[1] > 1:
            y = y[:, 0::2] + y[:, 1::2]
        x = y[:, 0]
        if blocks == 1:
            return [float(v) for v in x[0]]


def jacobi(N, sweeps=SWEEPS):
    """the header's cyclic Jacobi on a 4 x 4 list of lists; returns (N, V)"""
    N = [[F(v) for v in row] for row in N]
    V = [[F(1.0) if r == k else F(0.0) for k in range(4)] for r in range(4)]
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
            for k in range(4):
                if k != p and k != q:
                    u, w = N[k][p], N[k][q]
                    N[k][p] = N[p][k] = c * u - s * w
                    N[k][q] = N[q][k] = s * u + c * w
            h = t * apq
            N[p][p] = N[p][p] - h
            N[q][q] = N[q][q] + h
            N[p][q] = N[q][p] = F(0.0)
            for k in range(4):
                u, w = V[k][p], V[k][q]
                V[k][p] = c * u - s * w
                V[k][q] = s * u + c * w
    return N, V


def horn_matrix(S):
    N = [[F(0.0)] * 4 for _ in range(4)]
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    N[0][1] = N[1][0] = S[1][2] - S[2][1]
    N[0][2] = N[2][0] = S[2][0] - S[0][2]
    N[0][3] = N[3][0] = S[0][1] - S[1][0]
    N[1][2] = N[2][1] = S[0][1] + S[1][0]
    N[1][3] = N[3][1] = S[2][0] + S[0][2]
    N[2][3] = N[3][2] = S[1][2] + S[2][1]
    return N


def solve(S, Sx, mux, muq, with_scale, sweeps=SWEEPS, info=None):
    """step 5: (M as 3 x 4 float64, scale), or None where the spec stops as degenerate"""
    if Sx == 0.0:
        return None
    N, V = jacobi(horn_matrix(S), sweeps)
    if info is not None:
        info["N"] = N
    j = 0
    for k in range(1, 4):
        if N[k][k] > N[j][j]:
            j = k
    v = [V[k][j] for k in range(4)]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        length = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
        q0, q1, q2, q3 = (x / length for x in v)
        two = F(2.0)
        R = [[((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3, two * (q1 * q2 - q0 * q3), two * (q1 * q3 + q0 * q2)],
             [two * (q1 * q2 + q0 * q3), ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3, two * (q2 * q3 - q0 * q1)],
             [two * (q1 * q3 - q0 * q2), two * (q2 * q3 + q0 * q1), ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3]]
        scale = F(1.0)
        if with_scale:
            g = R[0][0] * S[0][0]
            for k in range(1, 9):
                a, b = k // 3, k % 3
                g = g + R[b][a] * S[a][b]
            scale = g / Sx
        M = np.zeros((3, 4), F)
        for r in range(3):
            for k in range(3):
                M[r, k] = scale * R[r][k]
            M[r, 3] = muq[r] - ((M[r, 0] * mux[0] + M[r, 1] * mux[1]) + M[r, 2] * mux[2])
    if not (np.isfinite(scale) and scale > 0 and np.isfinite(M).all()):
        return None
    return M, float(scale)


def one_pass(x32, t32, M, max_dist):
    """steps 1 to 4: the search's result, m, the means, S (3 x 3 list), Sx, the record's rms"""
    y32 = transform_positions(x32, M)
    near = nearest(y32, t32, max_dist)
    idx = near["index"]
    hit = idx >= 0
    m = int(hit.sum())
    n = len(x32)
    x = x32.astype(F)
    q = np.zeros((n, 3), F)
    q[hit] = t32[idx[hit]].astype(F)
    terms = np.zeros((n, 6), F)
    terms[hit, :3] = x[hit] + 0.0
    terms[hit, 3:] = q[hit] + 0.0
    sums = channel_sums(terms) if n else [0.0] * 6
    mu = [F(s) / F(m) if m else F(0.0) for s in sums]
    mux, muq = mu[:3], mu[3:]
    terms = np.zeros((n, 11), F)
    if m:
        dx = x[hit] - np.array(mux)
        dq = q[hit] - np.array(muq)
        e = y32[hit].astype(F) - q[hit]
        for k in range(9):
            terms[hit, k] = dx[:, k // 3] * dq[:, k % 3] + 0.0
        terms[hit, 9] = ((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]) + 0.0
        terms[hit, 10] = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + 0.0
    sums = [F(s) for s in (channel_sums(terms) if n else [0.0] * 11)]
    S = [[sums[3 * a + b] for b in range(3)] for a in range(3)]
    rms = float(np.sqrt(sums[10] / F(m))) if m else 0.0
    return near, m, mux, muq, S, sums[9], rms


def align(source, target, max_dist, iterations=30, scale=False, init=None, rms_tol=0.0, min_pairs=3,
          correspondences=False, sweeps=SWEEPS, info=None) -> dict:
    x32, t32 = positions(source), positions(target)
    M = IDENTITY.copy() if init is None else np.asarray(init, F).reshape(3, 4).copy()
    trace = np.zeros(iterations + 1, STEP_DTYPE)
    out_scale, updates, reason, prev = 1.0, 0, STOP_ITERATIONS, 0.0
    for k in range(iterations + 1):
        near, m, mux, muq, S, Sx, rms = one_pass(x32, t32, M, max_dist)
        trace[k] = (m, rms)
        if k == iterations:
            break
        if m < min_pairs:
            reason = STOP_PAIRS
            break
        if k > 0 and rms_tol > 0 and abs(F(rms) - F(prev)) <= rms_tol:
            reason = STOP_RMS
            break
        prev = rms
        new = solve(S, Sx, mux, muq, scale, sweeps, info)
        if new is None:
            reason = STOP_DEGENERATE
            break
        M, out_scale = new
        updates += 1
    if len(x32) == 0 or len(t32) == 0:
        reason = STOP_EMPTY
    stats = dict(near["stats"], iterations_run=updates, stop_reason=reason)
    return {"matrix": M, "scale": out_scale, "trace": trace, "index": near["index"] if correspondences else None,
            "dist": near["dist"] if correspondences else None, "stats": stats}


def det3(M):
    return float(np.linalg.det(np.asarray(M)[:, :3]))
