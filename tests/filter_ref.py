"""The patch filter (include/densepoints.h, dp_filter_patches) stated once more,
independently of both C implementations: plain Python over numpy scalars, one
IEEE operation per line in the header's order, no vectorised shortcuts.  It is
the high-precision statement that oracle/oracle.c (or_filter_patches) and the
HIP kernels (csrc/dp_filter.hip) are judged by; there is no reference binary
(pmvs.h:27 is undefined, modules/filtering empty).

filter_trace() also returns the intermediate results (front maps, candidates
per cell, both sides of both thresholds) that tests/filtercases.py checks its
premises against."""
import numpy as np

F64 = np.float64
INT64_MAX = 2 ** 63 - 1


def _proj(P, X):
    """(u, w, depth) of X in the view with projection P: ((p0 x + p1 y) + p2 z)
    + p3 per row, then one division each (inf / NaN where depth is 0)."""
    h = [((P[r, 0] * X[0] + P[r, 1] * X[1]) + P[r, 2] * X[2]) + P[r, 3] for r in range(3)]
    return h[0] / h[2], h[1] / h[2], h[2]


def _cell_index(v, scale):
    """Organizer coordinate: truncation toward zero, anything <= -1 (or NaN)
    out of bounds, so (-scale, 0) is cell 0."""
    q = v / scale
    if not q > -1.0:
        return -1
    if q >= 9.0e18:
        return INT64_MAX
    return int(q)


def _mask_views(vis, V=128):
    """V(p): the bits of vis below V, ascending (bits at or beyond V name no view)."""
    return [w * 64 + b for w in range(2) for b in range(64) if (int(vis[w]) >> b) & 1 and w * 64 + b < V]


def _popcount(vis):
    return bin(int(vis[0])).count("1") + bin(int(vis[1])).count("1")


def f32_bits(d):
    return int(np.array([d], np.float32).view(np.uint32)[0])


def filter_trace(P, W, H, xr, patches, passes=3, frac=0.25, gs=8, count_unmasked=False):
    """The filter and its intermediate results.  count_unmasked = True is NOT
    the spec: it counts every bit of vis in |V(p)| (the reading the header
    rejects) and exists so a case can show that the two readings differ."""
    with np.errstate(all="ignore"):
        return _filter_trace(np.asarray(P, dtype=F64).reshape(-1, 3, 4), W, H, xr, patches, int(passes), F64(frac), int(gs),
                             count_unmasked)


def filter_spec(P, W, H, xr, patches, passes=3, frac=0.25, gs=8):
    return filter_trace(P, W, H, xr, patches, passes, frac, gs)["keep"]


def _filter_trace(P, W, H, xr, patches, passes, frac, gs, count_unmasked):
    n = len(patches)
    V = len(P)
    gsf = F64(gs)
    gw = [int(w) // gs for w in W]
    gh = [int(h) // gs for h in H]
    pos = [tuple(F64(c) for c in p["pos"]) for p in patches]      # f32, widened
    nrm = [tuple(F64(c) for c in p["normal"]) for p in patches]
    score = [F64(np.float32(p["score"])) for p in patches]        # f32, widened
    views = [_mask_views(p["vis"], V) for p in patches]
    nv = [_popcount(p["vis"]) if count_unmasked else len(views[i]) for i, p in enumerate(patches)]
    cells = {}

    def cell(v, i):
        if (v, i) not in cells:
            with np.errstate(all="ignore"):
                u, w, _ = _proj(P[v], pos[i])
            r, c = _cell_index(w, gsf), _cell_index(u, gsf)
            cells[(v, i)] = (r, c) if 0 <= c < gw[v] and 0 <= r < gh[v] else None
        return cells[(v, i)]

    def depth(v, i):
        with np.errstate(all="ignore"):
            return np.float32(_proj(P[v], pos[i])[2])

    def rho(i):
        rv = int(patches[i]["ref"])
        if rv >= V:
            return F64(0.0)
        u0, w0, _ = _proj(P[rv], pos[i])
        u1, w1, _ = _proj(P[rv], tuple(pos[i][k] + F64(xr[rv][k]) for k in range(3)))
        du, dw = u1 - u0, w1 - w0
        dx = np.sqrt(du * du + dw * dw)
        return gsf / dx if dx > 0.0 else F64(0.0)

    def nb(i, q, r2):
        d = [pos[q][k] - pos[i][k] for k in range(3)]
        a = (d[0] * nrm[i][0] + d[1] * nrm[i][1]) + d[2] * nrm[i][2]
        b = (d[0] * nrm[q][0] + d[1] * nrm[q][1]) + d[2] * nrm[q][2]
        return bool(abs(a) + abs(b) < r2)

    def front(alive):
        cands = {}
        for i in range(n):
            if not alive[i]:
                continue
            for v in views[i]:
                c = cell(v, i)
                if c is None:
                    continue
                d = depth(v, i)
                if not d > 0:
                    continue
                cands.setdefault((v, c), []).append((f32_bits(d) << 32) | i)
        return {k: min(keys) for k, keys in cands.items()}, cands

    tr = {"V": V, "gw": gw, "gh": gh, "views": views, "cell": cell, "depth": depth, "front": {}, "cands": {},
          "vis_terms": [None] * n, "nbr_terms": [None] * n}
    rhos = [rho(i) for i in range(n)]
    tr["rho"] = rhos
    alive = [1] * n
    if passes & 1:
        f, tr["cands"][1] = front(alive)
        tr["front"][1] = f
        keep = []
        for i in range(n):
            occ = F64(0.0)
            for v in views[i]:
                c = cell(v, i)
                if c is None or (v, c) not in f:
                    continue
                q = f[(v, c)] & 0xFFFFFFFF
                if q == i or nb(i, q, F64(2.0) * rhos[i]):
                    continue
                occ = occ + score[q]
            lhs = F64(nv[i]) * score[i]
            tr["vis_terms"][i] = (lhs, occ)
            keep.append(0 if lhs < occ else 1)
        alive = keep
    tr["after1"] = list(alive)
    if passes & 2:
        f, tr["cands"][2] = front(alive)
        tr["front"][2] = f
        keep = []
        for i in range(n):
            if not alive[i]:
                keep.append(0)
                continue
            tot = near = 0
            for v in views[i]:
                c = cell(v, i)
                if c is None:
                    continue
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        r, cc = c[0] + dr, c[1] + dc
                        if not (0 <= r < gh[v] and 0 <= cc < gw[v]) or (v, (r, cc)) not in f:
                            continue
                        q = f[(v, (r, cc))] & 0xFFFFFFFF
                        if q == i:
                            continue
                        tot += 1
                        near += nb(i, q, F64(2.0) * rhos[i])
            tr["nbr_terms"][i] = (near, tot)
            keep.append(0 if tot > 0 and F64(near) < frac * F64(tot) else 1)
        alive = keep
    tr["keep"] = np.array(alive, dtype=np.uint8)
    return tr


def with_occluders(orc, P, patches, k=25, pull=0.3, score=0.99):
    """For each of the first k patches and each view it is visible in, a copy
    pulled toward that view's camera (same ray: same cell, in front, not a
    neighbour) with a high score, appended after the originals."""
    extra = []
    for p in patches[:k]:
        X = p["pos"].astype(np.float64)
        for v in _mask_views(p["vis"]):
            C = orc.view_geometry(P[v])[1]
            e = p.copy()
            e["pos"] = (C + (1.0 - pull) * (X - C)).astype(np.float32)
            e["score"] = np.float32(score)
            extra.append(e)
    return np.concatenate([patches, np.array(extra, dtype=patches.dtype)])


def first_differences(got, want, patches, k=5):
    """the first differing indices and their records, for a failure message"""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    lines = [f"{bad.size} of {len(want)} flags differ, first {bad[:k].tolist()}"]
    for i in bad[:k]:
        p = patches[i]
        lines.append(f"  [{i}] got {got[i]} want {want[i]} pos {p['pos'].tolist()} ref {p['ref']} "
                     f"vis {[hex(int(w)) for w in p['vis']]} score {p['score']!r}")
    return "\n".join(lines)
