"""Planted keypoints for the stages of seed generation after the detector
(dp_probe_seed_stages / or_seeds_from_keypoints): the pair and job plan, the
multi-job kNN, match_kernel, epipolar_match_kernel, the t2q table and
triang_kernel.  On rendered scenes a detector decides what these stages see:
about a hundred matches, no train keypoint with two queries, no value on a
bound.  Here every case is built for one edge, deterministic and seeded.

build(name) returns a Case (cached): P (V x 3 x 4), counts (keypoints per
view), kp (KEYPOINT_DTYPE, view-major), desc (n x 32 or n x 64 bytes), options
(the matcher options that differ from the defaults) and meta (what was planted,
for tests/test_seedcases_cpu.py, which asserts on the numpy restatement
tests/seedstage_ref.py that each case reaches what it is for).  NAMES lists
them in the order small -> large."""
import functools

import numpy as np

from densepoints_amd._native import KEYPOINT_DTYPE

KNN, FLANN = 0, 1


class Case:
    def __init__(self, name, P, counts, kp, desc, options=None, meta=None):
        self.name = name
        self.P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3, 4)
        self.counts = [int(c) for c in counts]
        self.kp = np.ascontiguousarray(kp, dtype=KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(desc, dtype=np.uint8)
        self.options = dict(options or {})
        self.meta = dict(meta or {})
        assert len(self.P) == len(self.counts) and sum(self.counts) == len(self.kp) == len(self.desc)
        assert self.desc.ndim == 2 and self.desc.shape[1] in (32, 64)

    @property
    def V(self):
        return len(self.counts)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    @property
    def size(self):
        return len(self.kp)


# ---- cameras ---------------------------------------------------------------
def intrinsics(f=1000.0, cx=640.0, cy=480.0):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def translated(K, t):
    """K [I | t]"""
    return K @ np.hstack([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)])


def horizontal_rig(V, K=None):
    """view v at (v, 0, 0), all looking down +z: the epipolar line of (x, y) is
    the row y in every other view"""
    K = intrinsics() if K is None else K
    return np.stack([translated(K, (-float(v), 0.0, 0.0)) for v in range(V)])


def ring_rig(V, radius=5.0, K=None):
    """V cameras on a circle around the origin at alternating heights, looking at it"""
    K = intrinsics(800.0) if K is None else K
    out = []
    for v in range(V):
        a = 2.0 * np.pi * v / V
        C = np.array([radius * np.cos(a), radius * np.sin(a), 0.6 if v % 2 else -0.4])
        z = -C / np.linalg.norm(C)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        out.append(K @ np.hstack([R, (-R @ C).reshape(3, 1)]))
    return np.stack(out)


def project(P, X):
    h = np.asarray(X) @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3]


# ---- descriptors -----------------------------------------------------------
def pack(bits):
    """0/1 rows -> byte rows; bit b is bit b % 8 of byte b // 8"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), axis=-1, bitorder="little")


def unpack(rows):
    return np.unpackbits(np.asarray(rows, dtype=np.uint8), axis=-1, bitorder="little")


def hadamard(width):
    """the 8 * width Sylvester-Hadamard rows as bit rows: row 0 is all zeros and
    two different rows differ in exactly half of their bits"""
    n = 8 * width
    i = np.arange(n)
    par = i[:, None] & i[None, :]
    bits = np.zeros((n, n), dtype=np.uint8)
    while par.any():
        bits ^= (par & 1).astype(np.uint8)
        par >>= 1
    return bits


def flipped(bits, d, rng, limit=None):
    """a copy of a bit row with d bits flipped, below bit `limit`"""
    out = bits.copy()
    out[rng.choice(limit or len(bits), size=d, replace=False)] ^= 1
    return out


def keypoints(xy):
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    kp = np.zeros(len(xy), dtype=KEYPOINT_DTYPE)
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    kp["response"] = 1.0
    return kp


# ---- 1. tracks12 -----------------------------------------------------------
# empty, one-row and two-row views in the middle and at the end of the list
TRACKS12_COUNTS = [300, 257, 129, 0, 300, 33, 2, 1, 300, 31, 300, 0]


def _tracks(name, counts, n_points, width, seed):
    rng = np.random.default_rng(seed)
    V = len(counts)
    P = ring_rig(V)
    X = rng.uniform(-1.0, 1.0, size=(n_points, 3))
    nbits = 486 if width == 64 else 256  # the 64-byte rows as AKAZE's M-LDB: bits >= 486 are zero
    code = np.zeros((n_points, 8 * width), dtype=np.uint8)
    code[:, :nbits] = rng.integers(0, 2, size=(n_points, nbits), dtype=np.uint8)
    kps, descs, ids = [], [], []
    for v in range(V):
        # point 0 stays in every view that has keypoints; the order differs per view
        pid = np.zeros(0, dtype=np.int64)
        if counts[v]:
            rest = rng.permutation(np.arange(1, n_points))[: counts[v] - 1]
            pid = rng.permutation(np.concatenate([[0], rest]))
        # integer coordinates; every tenth keypoint 2 px off its place, for the epipolar filter to find
        xy = np.rint(project(P[v], X[pid]))
        xy[5::10] += rng.choice([-2.0, 2.0], size=(len(xy[5::10]), 2))
        kps.append(keypoints(xy))
        descs.append(pack(np.stack([flipped(code[i], int(rng.integers(0, 11)), rng, nbits) for i in pid]))
                     if counts[v] else np.zeros((0, width), dtype=np.uint8))
        ids.append(pid)
    return Case(name, P, counts, np.concatenate(kps), np.concatenate(descs), {},
                {"point_ids": ids, "nbits": nbits})


# ---- 2. ratio_edges --------------------------------------------------------
# (best, second) Hamming distances planted per query.  10 d0 == 7 d1 is false in
# float at nn_match_ratio 0.7f (0.7f * 10 rounds up to 7) and 10 d0 == 8 d1 at
# 0.8f (0.8f * 10 rounds down to 8, where the product in double stays above 8).
RATIO_PLANTED = [(7, 10), (14, 20), (21, 30), (28, 40), (35, 50), (70, 100), (69, 100), (0, 1), (0, 0),
                 (8, 10), (16, 20), (24, 30), (32, 40), (40, 50), (80, 100), (79, 100)]
TIE_GAP = 200  # equal rows this far apart: another 128-row stage of the kNN kernel


def _row_y(n, y=240.0):
    return np.full(n, y)


def _ratio_edges(name, width, ratio, seed=5):
    """views 0 -> 1 hold the planted distances; view 2 is [all zeros, all ones
    but 77 bits], which the all-ones and all-zeros queries of view 0 see at
    (77, 8 width) and (0, 8 width - 77): popcnt(q) at both ends"""
    rng = np.random.default_rng(seed)
    H = hadamard(width)
    n = 8 * width
    nt = 236
    train = H[n - 1 - np.arange(nt)].copy()  # fillers (rows >= 20): half the bits from every query
    query, planted = [], []
    for i, (d0, d1) in enumerate(RATIO_PLANTED):
        h = H[i + 1]
        query.append(h)
        a = 2 * i
        b = a + TIE_GAP if d0 == d1 else a + 1
        train[a] = flipped(h, d0, rng)
        train[b] = flipped(h, d1, rng)
        planted.append((i, a, d0, d1))
    ones = np.ones(n, dtype=np.uint8)
    query += [ones, np.zeros(n, dtype=np.uint8)]
    nq = len(query)
    view2 = np.stack([np.zeros(n, dtype=np.uint8), flipped(ones, 77, rng)])
    kp = np.concatenate([keypoints(np.stack([700.0 + 3 * np.arange(nq), _row_y(nq)], axis=1)),
                         keypoints(np.stack([20.0 + np.arange(nt), _row_y(nt)], axis=1)),
                         keypoints([[5.0, 240.0], [9.0, 240.0]])])
    return Case(name, horizontal_rig(3), [nq, nt, 2], kp, pack(np.concatenate([np.stack(query), train, view2])),
                {"nn_match_ratio": ratio}, {"planted": planted, "ratio10": int(round(ratio * 10)), "nbits": n,
                                            "extreme_queries": (nq - 2, nq - 1)})


def _flann_edges(name, width=32, seed=6):
    """best distances 29 (kept) and 30 (dropped); equal best rows TIE_GAP apart;
    a one-row train view (2) with a query at 29 and one at 30 from its row; an
    empty view (3)"""
    rng = np.random.default_rng(seed)
    H = hadamard(width)
    n = 8 * width
    nt = 241
    train = H[n - 1 - np.arange(nt)].copy()  # fillers (rows >= 15)
    query, planted = [], []
    for i, d0 in enumerate([29, 30, 0, 29, 30, 1]):
        h = H[i + 1]
        query.append(h)
        train[3 * i + 1] = flipped(h, d0, rng)
        planted.append((i, 3 * i + 1, d0))
    h = H[9]  # two rows at 29 from it, the same row twice
    query.append(h)
    train[40] = train[40 + TIE_GAP] = flipped(h, 29, rng)
    planted.append((len(query) - 1, 40, 29))
    one = H[10]
    lone = [(len(query), 29), (len(query) + 1, 30)]
    query += [flipped(one, 29, rng), flipped(one, 30, rng)]
    nq = len(query)
    kp = np.concatenate([keypoints(np.stack([700.0 + 3 * np.arange(nq), _row_y(nq)], axis=1)),
                         keypoints(np.stack([20.0 + np.arange(nt), _row_y(nt)], axis=1)),
                         keypoints([[5.0, 240.0]])])
    return Case(name, horizontal_rig(4), [nq, nt, 1, 0], kp, pack(np.concatenate([np.stack(query), train, one[None]])),
                {"matcher_type": FLANN}, {"planted": planted, "lone": lone})


# ---- 3. contended_t2q ------------------------------------------------------
def _contended(name, width=32, seed=7):
    """3000 queries (12 kNN blocks) nearest to train row 5, 150 each to rows 0
    and nt - 1; the first queries of each group lie 10 px off the epipolar line"""
    rng = np.random.default_rng(seed)
    H = hadamard(width)
    nt = 40
    train = H[1:nt + 1]
    groups = [(5, 3000, 3), (0, 150, 2), (nt - 1, 150, 4)]
    q_bits, q_xy, meta = [], [], []
    q0 = 0
    for row, cnt, off_line in groups:
        for k in range(cnt):
            q_bits.append(flipped(train[row], int(rng.integers(0, 4)), rng))
            q_xy.append((700.0 + (k % 500), 250.0 if k < off_line else 240.0))
        meta.append({"row": row, "first": q0, "count": cnt, "off_line": off_line})
        q0 += cnt
    kp = np.concatenate([keypoints(q_xy), keypoints(np.stack([20.0 + 5 * np.arange(nt), _row_y(nt)], axis=1))])
    return Case(name, horizontal_rig(2), [q0, nt], kp, pack(np.concatenate([np.stack(q_bits), train])), {},
                {"groups": meta})


# ---- 4. epipolar_edges -----------------------------------------------------
def edge_rows(y):
    """train rows 0, +1.5, just above +1.5, -1.5, just below +1.5, just below -1.5 px from the row y"""
    f = np.float32
    up, dn = f(y + 1.5), f(y - 1.5)
    return np.array([f(y), up, np.nextafter(up, f(np.inf)), dn, np.nextafter(up, f(-np.inf)),
                     np.nextafter(dn, f(-np.inf))], dtype=np.float32)


def _epipolar_knn(name, width=32):
    """six queries on the row 100, each the exact descriptor of one train row"""
    H = hadamard(width)
    ys = edge_rows(100.0)
    n = len(ys)
    code = H[1:n + 1]
    kp = np.concatenate([keypoints(np.stack([800.0 + 10 * np.arange(n), np.full(n, 100.0)], axis=1)),
                         keypoints(np.stack([100.0 + 10 * np.arange(n), ys], axis=1))])
    return Case(name, horizontal_rig(2), [n, n], kp, pack(np.concatenate([code, code])), {}, {"rows": ys})


def _epipolar_direct(name, width=32, seed=8, block=600):
    """epipolar_matching = 1: a block x block set in which every train row is
    on every query's line (the row 300), and the edge rows around the row 100"""
    rng = np.random.default_rng(seed)
    ys = edge_rows(100.0)
    n = len(ys)
    q_xy = np.concatenate([np.stack([700.0 + np.arange(block // 2), np.full(block // 2, 300.0)], axis=1),
                           np.stack([800.0 + 10 * np.arange(n), np.full(n, 100.0)], axis=1),
                           np.stack([700.0 + np.arange(block - block // 2), np.full(block - block // 2, 300.0)], axis=1)])
    t_xy = np.concatenate([np.stack([100.0 + 10 * np.arange(3), ys[:3]], axis=1),
                           np.stack([20.0 + np.arange(block), np.full(block, 300.0)], axis=1),
                           np.stack([130.0 + 10 * np.arange(n - 3), ys[3:]], axis=1)])
    kp = np.concatenate([keypoints(q_xy), keypoints(t_xy)])
    desc = rng.integers(0, 256, size=(len(kp), width), dtype=np.uint8)
    return Case(name, horizontal_rig(2), [len(q_xy), len(t_xy)], kp, desc, {"epipolar_matching": True},
                {"rows": ys, "block": block, "edge_queries": np.arange(block // 2, block // 2 + n),
                 "edge_trains": np.concatenate([np.arange(3), 3 + block + np.arange(n - 3)])})


# ---- 5. nan_line -----------------------------------------------------------
def _nan_line(name, direct, width=32, seed=9, n_points=40):
    """views 0 and 1 differ by a purely vertical translation: the second
    coefficient of every epipolar line is 0 and every distance NaN; view 2 is
    an ordinary one"""
    rng = np.random.default_rng(seed)
    K = intrinsics()
    P = np.stack([translated(K, (0, 0, 0)), translated(K, (0, 1, 0)), translated(K, (-1, 0, 0.25))])
    X = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(6, 12, n_points)], axis=1)
    code = rng.integers(0, 2, size=(n_points, 8 * width), dtype=np.uint8)
    kps, descs = [], []
    for v in range(3):
        pid = rng.permutation(n_points)
        kps.append(keypoints(np.rint(project(P[v], X[pid]))))
        descs.append(pack(np.stack([flipped(code[i], int(rng.integers(0, 6)), rng) for i in pid])))
    return Case(name, P, [n_points] * 3, np.concatenate(kps), np.concatenate(descs),
                {"epipolar_matching": True} if direct else {}, {})


# ---- 6. half_pixels --------------------------------------------------------
HALF_QUERY = [(4.5, 0.5), (5.5, 2.5), (6.5, 1.5), (8191.5, 8191.5), (8.5, -0.5), (9.5, -1.5), (12.5, 7.5), (13.0, 9.0)]


def _half_pixels(name, width=32):
    """x.5 coordinates with even and odd integer parts (cv::Point rounds half
    to even): each query's train keypoint lies 4 px to its left on its row"""
    H = hadamard(width)
    q = np.array(HALF_QUERY, dtype=np.float64)
    t = q - np.array([4.0, 0.0])
    code = H[1:len(q) + 1]
    return Case(name, horizontal_rig(2), [len(q), len(t)], np.concatenate([keypoints(q), keypoints(t)]),
                pack(np.concatenate([code, code])), {}, {})


# ---- 7. far_points ---------------------------------------------------------
def _far_points(name, V, width=32, seed=10):
    """points at 10^2 .. 10^6 baselines under a focal length of 2^21 px: the
    disparities run from 20972 px down to 2 px"""
    rng = np.random.default_rng(seed)
    f = float(1 << 21)
    P = horizontal_rig(V, np.array([[f, 0.0, 0.0], [0.0, f, 0.0], [0.0, 0.0, 1.0]]))
    depth = np.repeat(10.0 ** np.arange(2, 7), 6)
    n = len(depth)
    uv = rng.integers(-3000, 3001, size=(n, 2)).astype(np.float64)
    X = np.stack([uv[:, 0] * depth / f, uv[:, 1] * depth / f, depth], axis=1)
    code = hadamard(width)[1:n + 1]
    kps = [keypoints(np.rint(project(P[v], X))) for v in range(V)]
    return Case(name, P, [n] * V, np.concatenate(kps), pack(np.concatenate([code] * V)), {}, {"depth": depth})


_BUILDERS = {
    "epipolar_knn": lambda n: _epipolar_knn(n),
    "half_pixels": lambda n: _half_pixels(n),
    "far_points2": lambda n: _far_points(n, 2),
    "far_points3": lambda n: _far_points(n, 3),
    "nan_line_knn": lambda n: _nan_line(n, False),
    "nan_line_direct": lambda n: _nan_line(n, True),
    "flann_edges": lambda n: _flann_edges(n),
    "ratio_edges_07": lambda n: _ratio_edges(n, 32, 0.7),
    "ratio_edges_08": lambda n: _ratio_edges(n, 32, 0.8),
    "ratio_edges_07_wide": lambda n: _ratio_edges(n, 64, 0.7),
    "ratio_edges_08_wide": lambda n: _ratio_edges(n, 64, 0.8),
    "tracks12_full": lambda n: _tracks(n, [40] * 12, 40, 32, 3),
    "epipolar_direct": lambda n: _epipolar_direct(n),
    "tracks12": lambda n: _tracks(n, TRACKS12_COUNTS, 300, 32, 1),
    "tracks12_wide": lambda n: _tracks(n, TRACKS12_COUNTS, 300, 64, 2),
    "contended_t2q": lambda n: _contended(n),
}
NAMES = list(_BUILDERS)  # small -> large


@functools.lru_cache(maxsize=None)
def build(name):
    return _BUILDERS[name](name)


_REFERENCE, _ORACLE = {}, {}


def reference(orc, name):
    """the numpy restatement's result on a case (seedstage_ref.run), computed once"""
    import seedstage_ref as SR

    if name not in _REFERENCE:
        c = build(name)
        _REFERENCE[name] = SR.run(c.P, c.counts, c.kp, c.desc, c.options, orc.fundamental_matrix, orc.triangulate)
    return _REFERENCE[name]


def oracle(orc, name):
    """or_seeds_from_keypoints on a case, computed once"""
    if name not in _ORACLE:
        c = build(name)
        _ORACLE[name] = orc.seeds_from_keypoints(c.P, c.counts, c.kp, c.desc, orc.matcher_options(**c.options))
    return _ORACLE[name]
