"""Inputs for the parity refine (dp_refine.hip) at every window size and view-pass
width.  pass_width(cell) compiles one kernel per group of cells -- G views of
64 / G lanes per pass, DP_TEX_PER_LANE = 4 texels per lane:

  cells 2-5    G = 8    8 lanes per view
  cells 6-8    G = 4   16 lanes per view
  cells 9-11   G = 2   32 lanes per view, plus the four-view wide pass and the
                       split pass
  cells 12-16  G = 1   64 lanes per view

and how a cell fills the texel slots differs in kind: N = cell^2 odd (the last
u16 pair half dead), N = 64 or 256 (no dead texel), N < lanes (lanes with no
live texel at all), N = 81 or 100 in the wide pass (pairs dead in both halves).

This module builds every input once and names, per item, the cells, modes and
visible-view counts the GPU tests run (tests/test_gpu_refine_cells.py);
tests/test_refinecases_cpu.py asserts on the oracle alone that each input is
the case it is meant to be, and that the tables below cover every cell and, per
G, every kind of path.

  hf6     6 views of 320 x 240 (test_gpu_parity's scene), its first 160 seeds
  wide70  70 views of 96 x 72: visible lists reaching past view 63
  Base    30 views of 256 x 192 and, per cell, the views in which the oracle
          finds a window map for each seed (test_gpu_wide_pass's scene, whose
          search was at cell 11 only)"""
import functools

import numpy as np

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import synth

FIELDS = ("pos", "normal", "ref", "vis", "cand", "score", "evals", "flags")
DENSIFY_FIELDS = FIELDS + ("seq", "parent", "rgb")

MAX_CELL = 16
TEX_PER_LANE = 4
MAP_CHUNK = 24  # views per map chunk (texture 0 takes slot 0 of the first)
CELLS = tuple(range(2, MAX_CELL + 1))
ALL_MODES = (N.MODE_EVAL, N.MODE_FILTER, N.MODE_NM, N.MODE_SEED, N.MODE_EXPAND)
OPTIMISING = (N.MODE_NM, N.MODE_SEED, N.MODE_EXPAND)
MODE_NAME = {N.MODE_EVAL: "eval", N.MODE_FILTER: "filter", N.MODE_NM: "nm", N.MODE_SEED: "seed",
             N.MODE_EXPAND: "expand"}
MIN_PATCHES = 32

V, W, H = 30, 256, 192  # Base
NCAND = 160
N_HF6 = 160


def pass_width(cell):
    """views per pass of the kernel that runs `cell` (dp_refine.hip pass_width)"""
    for g in (8, 4, 2, 1):
        if cell * cell <= (64 // g) * TEX_PER_LANE:
            return g
    raise ValueError(cell)


def assert_same(gp, op, fields=FIELDS):
    """every field, bit for bit"""
    assert len(gp) == len(op)
    for f in fields:
        a, b = gp[f], op[f]
        if a.dtype.kind == "f":
            bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1))
        else:
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, f"field {f}: {bad.size} of {len(a)} patches differ, first {bad[:5]}: " \
                              f"{a[bad[0]]} vs {b[bad[0]]}"


# ---------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------
# item 3: visible-view counts m per cell.  A pass holds G views, texture 0 in
# slot 0 of the first, so m = k G is k full passes, m = k G + 1 leaves one view
# over, m = 24 fills a map chunk and m >= 25 opens a second one.  G = 2 runs
# wide passes of four while four are left, then narrow and split passes: the
# list of test_gpu_wide_pass (every remainder modulo four, the pair map round at
# 20, two chunks at 27) after 2 and 3, which take no wide pass at all.
_M8 = (2, 7, 8, 9, 16, 17, 24, 25)
_M4 = (2, 3, 4, 5, 8, 9, 24, 25)
_M2 = (2, 3, 4, 5, 6, 7, 8, 9, 20, 27)
_M1 = (2, 3, 24, 25)
VISIBLE_M = {4: _M8, 5: _M8, 6: _M4, 8: _M4, 9: _M2, 10: _M2, 12: _M1, 13: _M1, 16: _M1}
VISIBLE_MODES = (N.MODE_EVAL, N.MODE_NM, N.MODE_EXPAND)
VISIBLE_N = 96

# item 4: 64-bit tap addressing (a.narrow false)
WIDE_ADDR_HF6 = tuple((cell, mode) for cell in (4, 8, 9, 13) for mode in (N.MODE_NM, N.MODE_EXPAND))
WIDE_ADDR_BASE = ((9, 9), (8, 9))  # (cell, m): full passes in the non-narrow kernels
WIDE_ADDR_N = 120

# items 5-8
UNSAFE_CELLS = (5, 8, 10, 13)
UNSAFE_MODES = (N.MODE_EVAL, N.MODE_FILTER, N.MODE_NM, N.MODE_EXPAND)
PITCH_CELLS = (4, 8, 10, 13)
PITCH_MODES = (N.MODE_EVAL, N.MODE_NM, N.MODE_EXPAND)
PITCH_PAD = 40
BEYOND64_CELLS = (4, 8, 10, 13)
BEYOND64_MODES = (N.MODE_EVAL, N.MODE_NM, N.MODE_EXPAND)
EDGE_CELLS = (2, 4, 8, 10, 13)

# item 9: whole densify on refine_kernel<DP_MODE_EXPAND, G, true> (and the seed
# stage's kernel where seed_cell_size is set)
DENSIFY_OPTIONS = (
    dict(expand_cell_size=4, max_pops=200),
    dict(expand_cell_size=8, max_pops=200),
    dict(expand_cell_size=9, max_pops=200),
    dict(expand_cell_size=13, max_pops=200),
    dict(seed_cell_size=6, expand_cell_size=10),
    dict(seed_cell_size=12, expand_cell_size=14),
)
GENERATION_API_OPTIONS = DENSIFY_OPTIONS[3]

# item 10
REPEAT_CELLS = (4, 9, 13)


def options_id(kw):
    return "-".join("%s%d" % (k.split("_")[0], v) for k, v in kw.items())


def visible_kinds(cell, m):
    """the kinds of pass a visible set of m views takes in the cell's kernel"""
    g = pass_width(cell)
    kinds = set()
    if g > 1:
        if m >= g and m % g == 0:
            kinds.add("full")
        if m > g and m % g == 1:
            kinds.add("remainder")
    else:
        kinds.add("full")  # one view per pass: no pass is ever part full
    if m == MAP_CHUNK:
        kinds.add("chunk-full")
    if m > MAP_CHUNK:
        kinds.add("chunk-boundary")
    return kinds


def coverage():
    """{G: {kind: cells}} over the tables above, and the cells of items 1 and 2"""
    cov = {g: {} for g in (8, 4, 2, 1)}

    def add(cell, kind):
        cov[pass_width(cell)].setdefault(kind, set()).add(cell)

    for cell, ms in VISIBLE_M.items():
        for m in ms:
            for kind in visible_kinds(cell, m):
                add(cell, kind)
    for cell, _ in WIDE_ADDR_HF6:
        add(cell, "wide-addressing")
    for cell, m in WIDE_ADDR_BASE:
        if m >= 2 * pass_width(cell) > 2:  # two passes or more with every slot taken
            add(cell, "wide-addressing-full")
    for cell in UNSAFE_CELLS:
        add(cell, "unsafe")
    for cell in PITCH_CELLS:
        add(cell, "mixed-pitch")
    for cell in BEYOND64_CELLS:
        add(cell, "beyond-64")
    for cell in EDGE_CELLS:
        add(cell, "edge")
    for kw in DENSIFY_OPTIONS:
        add(kw["expand_cell_size"], "generation")
        if "seed_cell_size" in kw:
            add(kw["seed_cell_size"], "seed-stage")
    for cell in REPEAT_CELLS:
        add(cell, "repeat")
    return cov


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
class SceneCase:
    def __init__(self, V, W, H, kind, **kw):
        self.cfg = synth.config(V, W, H, kind, **kw)
        self.P, self.imgs, self.seeds = synth.scene_host(self.cfg)
        self.V = V
        self.views = views_of(self.P, self.imgs)


def views_of(P, imgs):
    return [dp.View(P[v], imgs[v]) for v in range(len(imgs))]


@functools.lru_cache(maxsize=None)
def scene(name) -> SceneCase:
    spec = {
        "hf6": dict(V=6, W=320, H=240, kind=1),
        "wide70": dict(V=70, W=96, H=72, kind=1, seed_stride_px=12.0),
    }[name]
    return SceneCase(**spec)


_oracle = {}


def oracle_scene(orc, name, **options):
    """the oracle's scene (cached per option set; never modified by a test)"""
    key = (name, tuple(sorted(options.items())))
    if key not in _oracle:
        sc = scene(name)
        _oracle[key] = orc.Scene(sc.P, sc.imgs, dp.Options(**options) if options else None)
    return _oracle[key]


def hf6_patches(orc):
    """the first 160 hf6 seed patches (test_refine_modes_bit_exact's input)"""
    return oracle_scene(orc, "hf6").seeds_to_patches(scene("hf6").seeds[:N_HF6])


def beyond64_patches(orc):
    """wide70's sample of test_more_than_64_views_bit_exact"""
    return oracle_scene(orc, "wide70").seeds_to_patches(scene("wide70").seeds[::7][:48])


_refs = {}


def oracle_refine(orc, key, S, pat, cell, mode):
    """(patches, accept) of the oracle's refine of `pat`, computed once per key
    and handed out as copies"""
    key = (key, cell, mode)
    if key not in _refs:
        op = pat.copy()
        oa = S.refine(op, cell, mode)
        _refs[key] = (op, oa)
    op, oa = _refs[key]
    return op.copy(), oa.copy()


# ---------------------------------------------------------------------------
# Base: 30 views, and per cell the views that map for each seed
# ---------------------------------------------------------------------------
class Base:
    """30 views of the height field; per seed, the views in which the oracle
    finds a window map at the seed's stored pose (checked pairwise: with two
    visible views the score is -1 exactly when either map fails)."""

    def __init__(self, orc, cell=11):
        self.cell = cell
        cfg = synth.config(V, W, H, 1, seed_stride_px=12.0)
        self.P, self.imgs, seeds = synth.scene_host(cfg)
        self.S = orc.Scene(self.P, self.imgs)
        pat = self.S.seeds_to_patches(seeds)
        good = np.zeros((len(pat), V), bool)
        for v in range(V):
            for t0 in (0, 1):
                if t0 == v:
                    continue
                q = pat.copy()
                q["vis"][:, 0] = np.uint64((1 << t0) | (1 << v))
                q["vis"][:, 1] = 0
                self.S.refine(q, cell, orc.MODE_EVAL)
                ok = q["score"] > -1.0
                if t0 == 0:
                    ok0 = ok
                else:
                    ok1 = ok
            # view v maps if it scores against either possible texture 0
            good[:, v] = ok0 if v != 0 else ok1
        good[:, 0] &= good[:, 1:].any(axis=1)
        self.pat, self.good = pat, good

    def qualifying(self, m):
        """seeds that map in m views or more"""
        return np.flatnonzero(self.good.sum(axis=1) >= m)

    def with_visible(self, m, n=NCAND, spread=False):
        """n patches whose visible set is m views that map at the stored pose
        (the lowest ones, or spread over the whole range)."""
        rows = self.qualifying(m)[:n]
        assert len(rows) >= 32, f"only {len(rows)} seeds map in {m} views"
        out = self.pat[rows].copy()
        for k, r in enumerate(rows):
            vs = np.flatnonzero(self.good[r])
            vs = vs[np.linspace(0, len(vs) - 1, m).round().astype(int)] if spread else vs[:m]
            assert len(set(vs.tolist())) == m
            out["vis"][k, 0] = np.uint64(sum(1 << int(v) for v in vs))
            out["vis"][k, 1] = 0
        return out


_bases = {}


def base(orc, cell=11) -> Base:
    """Base with the map search at `cell` (built once per cell)"""
    if cell not in _bases:
        _bases[cell] = Base(orc, cell)
    return _bases[cell]


def visible_case(orc, cell, m, n=VISIBLE_N):
    """item 3: (Base, n patches seeing m mapping views each)"""
    b = base(orc, cell)
    return b, b.with_visible(m, n=n)


def _unsafe_camera(X, n, s, angle):
    """A camera 0.1 s above the patch centre X (normal n, side s) that looks
    along the patch plane: its principal plane cuts the window, so two
    corners project from behind it -- the square -> quad map's W changes sign
    on the window, which TexMap::safe excludes -- and with a 30 px focal
    length all four land inside the image."""
    a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    z = np.cos(angle) * a + np.sin(angle) * b
    y = -n
    x = np.cross(y, z)
    R = np.stack([x, y, z])
    C = X + 0.1 * s * n
    K = np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]])
    return K @ np.hstack([R, -(R @ C)[:, None]])


class ExtraViews:
    """a scene made of Base's views and more: P, imgs, the oracle's scene S,
    the patches and, for the premises, what was found"""

    def __init__(self, orc, P, imgs, pat, **found):
        self.P, self.imgs, self.pat = P, imgs, pat
        self.S = orc.Scene(P, imgs)
        self.found = found


_cases = {}


def unsafe_case(orc, cell) -> ExtraViews:
    """item 5 (test_unsafe_window_in_one_slot's construction at `cell`): eight
    extra cameras, each almost inside one candidate's window plane; that
    candidate's visible set holds its camera next to seven ordinary views, so
    one slot of a pass is unsafe and the pass takes the clamped fallback.  The
    window's world size depends on the cell, so the cameras are searched per
    cell."""
    if ("unsafe", cell) in _cases:
        return _cases[("unsafe", cell)]
    b = base(orc, cell)
    pat = b.with_visible(7, n=64)
    extra, rows = [], []
    for k in range(len(pat)):
        if len(extra) == 8:
            break
        X = pat["pos"][k].astype(np.float64)
        n = pat["normal"][k].astype(np.float64)
        n /= np.linalg.norm(n)
        Pr = b.P[int(pat["ref"][k])]
        h = np.append(X, 1.0)
        depth = (Pr[2] @ h) / np.linalg.norm(Pr[2, :3])
        f = np.linalg.norm(np.cross(Pr[0, :3], Pr[2, :3])) / np.linalg.norm(Pr[2, :3]) ** 2
        s = cell * depth / f  # world size of the window
        for angle in np.linspace(0.2, 6.0, 12):
            Pc = _unsafe_camera(X, n, s, angle)
            # the oracle finds a map for it (all corners inside its image)
            S1 = orc.Scene(np.concatenate([b.P, Pc[None]]), list(b.imgs) + [b.imgs[1]])
            q = pat[k:k + 1].copy()
            t0 = dp.visible_list(q["vis"][0])[0]
            q["vis"][0, 0] = np.uint64((1 << t0) | (1 << V))
            S1.refine(q, cell, orc.MODE_EVAL)
            if q["score"][0] > -1.0:
                extra.append(Pc)
                rows.append(k)
                break
    P = np.concatenate([b.P, np.stack(extra)]) if extra else b.P
    imgs = list(b.imgs) + [b.imgs[1]] * len(extra)
    cases = pat[rows].copy()
    for i in range(len(extra)):
        cases["vis"][i, 0] |= np.uint64(1 << (V + i))
    out = ExtraViews(orc, P, imgs, cases, cameras=len(extra))
    _cases[("unsafe", cell)] = out
    return out


def padded(v):
    """item 6: the views whose image is PITCH_PAD pixels wider"""
    return v % 3 == 1


def pitch_case(orc, cell) -> ExtraViews:
    """item 6 (test_two_row_pitches_in_one_pass's views at `cell`): every third
    view's image is 40 pixels wider (same camera, padded columns), so passes mix
    two row pitches.  found["mixed"] counts the candidates whose first pass --
    the first G views of the visible list -- holds both pitches; for G = 1,
    where a pass is one view, those whose list does.  G = 2 is counted over two
    views, which is the narrow first pass and lies within the wide one."""
    if ("pitch", cell) in _cases:
        return _cases[("pitch", cell)]
    b = base(orc, cell)
    rng = np.random.default_rng(5)
    imgs = []
    for v, im in enumerate(b.imgs):
        if padded(v):
            pad = rng.integers(0, 256, (H, PITCH_PAD, 3), dtype=np.uint8)
            im = np.ascontiguousarray(np.concatenate([im, pad], axis=1))
        imgs.append(im)
    pat = b.with_visible(9, spread=False)
    g = pass_width(cell)
    first = 9 if g == 1 else g
    mixed = sum(len({padded(x) for x in dp.visible_list(v)[:first]}) == 2 for v in pat["vis"])
    out = ExtraViews(orc, b.P, imgs, pat, mixed=mixed)
    _cases[("pitch", cell)] = out
    return out


# ---------------------------------------------------------------------------
# item 8: edge patches
# ---------------------------------------------------------------------------
def window_corners(orc, P, p, cell):
    """the four window corners of patch p at its stored pose (or_scores:
    GetProjectedXYAxisAndScale, patch.cpp:86-123) and their pixels in view ref"""
    Pr = np.asarray(P[int(p["ref"])], dtype=np.float64).reshape(3, 4)
    _, _, _, _, xr = orc.view_geometry(Pr)
    xr = xr / np.linalg.norm(xr)
    X = p["pos"].astype(np.float64)
    n = p["normal"].astype(np.float64)
    y = np.cross(n, xr)

    def proj(Y):
        h = Pr @ np.append(Y, 1.0)
        return h[:2] / h[2]

    dx = np.linalg.norm(proj(X + xr) - proj(X))
    scale = (cell // 2) / dx
    c = np.stack([X - scale * xr - scale * y, X + scale * xr - scale * y, X + scale * xr + scale * y,
                  X - scale * xr + scale * y])
    return c, np.stack([proj(q) for q in c])


def border_patch(orc, cell):
    """a hf6 seed patch moved along its reference view's x axis until its window
    touches that image's right border: a corner in the last pixel column
    (W - 1 <= u < W, so the ROI ends at column W - 1, the furthest View::
    IsPointInside admits), seen by the reference view and one more, and scoring.
    Returns (patch, the corner's u, the image width)."""
    if ("border", cell) in _cases:
        return _cases[("border", cell)]
    sc, S = scene("hf6"), oracle_scene(orc, "hf6")
    pat = S.seeds_to_patches(sc.seeds)
    Wr = sc.imgs[0].shape[1]
    found = None
    for k in range(len(pat)):
        p = pat[k:k + 1].copy()
        r = int(p["ref"][0])
        others = [v for v in dp.visible_list(p["vis"][0]) if v != r]
        if not others:
            continue
        Pr = sc.P[r].reshape(3, 4)
        _, _, _, _, xr = orc.view_geometry(Pr)
        xr = xr / np.linalg.norm(xr)
        _, uv = window_corners(orc, sc.P, p[0], cell)
        X = p["pos"][0].astype(np.float64)
        h0, h1 = Pr @ np.append(X, 1.0), Pr @ np.append(X + xr, 1.0)
        per_unit = h1[0] / h1[2] - h0[0] / h0[2]  # pixels of u per unit step along xr
        t = (Wr - 0.5 - uv[:, 0].max()) / per_unit
        p["pos"][0] = (X + t * xr).astype(np.float32)
        _, uv = window_corners(orc, sc.P, p[0], cell)
        if not Wr - 1 <= uv[:, 0].max() < Wr:
            continue
        for v in others:
            q = p.copy()
            q["vis"][0] = dp.mask_from_list(sorted((r, v)))
            chk = q.copy()
            S.refine(chk, cell, orc.MODE_EVAL)
            if chk["score"][0] > -1.0:
                found = (q, float(uv[:, 0].max()), Wr)
                break
        if found:
            break
    _cases[("border", cell)] = found
    return found


def edge_patches(orc, cell):
    """item 8: the three patches of test_edge_cases (no visible view, one
    visible view, a position off every image) and border_patch(cell)"""
    sc, S = scene("hf6"), oracle_scene(orc, "hf6")
    p = S.seeds_to_patches(sc.seeds[:3])
    p["vis"][0] = 0
    p["vis"][1] = dp.mask_from_list(dp.visible_list(p["vis"][1])[:1])
    p["pos"][2] = [50.0, 50.0, 50.0]
    found = border_patch(orc, cell)
    assert found is not None, f"cell {cell}: no hf6 seed reaches the right image border and scores"
    return np.concatenate([p, found[0]])


# ---------------------------------------------------------------------------
# item 9: whole densify
# ---------------------------------------------------------------------------
_densify = {}


def oracle_densify(orc, kw):
    """(patches, statistics) of the oracle's Scene.densify of hf6 under
    Options(**kw), computed once"""
    key = tuple(sorted(kw.items()))
    if key not in _densify:
        sc = scene("hf6")
        _densify[key] = oracle_scene(orc, "hf6", **kw).densify(sc.seeds)
    op, st = _densify[key]
    return op.copy(), dict(st)
