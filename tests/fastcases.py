"""Scenes for the performance mode's staging (dp_fast_kernel.hip stage, or_fast.c
fast_stage) at the places where its arithmetic can go wrong without a scene of
equal, even-sized, comfortably large views noticing:

  border  six views of 160 x 120 and the seeds of a dense grid whose staged
          tiles are clamped at the left, top, right and bottom image edge, whose
          left edge is rounded down to an even column, and whose window box
          misses a view by less than a pixel (the view is dropped);
  mixed   the same cameras, each view's image cropped to its own size (odd
          widths, two gray-plane pitches): one staging reads views of several
          sizes, and a tile clamped at the right edge of an odd-width view reads
          the pixel pair (W - 1, W), i.e. one padding column of the gray plane;
  budget  twenty views of 128 x 96 and four zoomed copies (the same centres, 2.7
          to 3.1 times the focal length, so that a 16 x 16 window's pixel box
          approaches the cap of 48) with visible sets of 2 .. 18 views: the
          margin loop and the budget prefix at every arena size, tiles of more
          than 1,500 words.

build(name) returns a Scene (cached); tests/test_fastcases_cpu.py asserts on the
oracle alone that each scene is the case it is named for, so that a scene that
stops being so fails instead of silently passing; tests/test_gpu_fast_edges.py
compares the kernel with the oracle on them."""
import functools

import numpy as np

import densepoints_amd as dp
from densepoints_amd import synth

BORDER_SIZE = (160, 120)
# mixed: four odd widths; 126 x 101 has a gray pitch of 128 where the others have 192
MIXED_SIZES = [(160, 120), (159, 113), (131, 120), (126, 101), (145, 97), (153, 109)]
BUDGET_SIZE = (128, 96)
BUDGET_RIG, BUDGET_ZOOMS = 20, (2.7, 2.85, 3.0, 3.1)
# (margin, tile_budget) of the budget scene's refine stagings; the arenas are
# FastLds<6656>, <8192> and <16384> (8193 is the first budget of the largest)
BUDGETS = [(7, 6656), (7, 8192), (7, 8193), (7, 16384)]
# margin 0 and this budget: one ordinary tile and its record, so the prefix keeps
# fewer than two views and the score is -1
TINY_BUDGET = 64 + 400
MAX_PATCHES = 160


def gray_pitch(W):
    """the gray plane's pitch in pixels (densepoints_amd/csrc/dp_fast.hip)"""
    return (W + 2 + 63) & ~63


class Scene:
    """P (V x 3 x 4), imgs (BGR8, H_v x W_v x 3), sizes [(W_v, H_v)], views
    (dp.View) and seeds (n x 3)"""

    def __init__(self, name, P, imgs, seeds):
        self.name, self.P, self.imgs = name, np.ascontiguousarray(P), [np.ascontiguousarray(im) for im in imgs]
        self.V = len(imgs)
        self.sizes = [(im.shape[1], im.shape[0]) for im in self.imgs]
        self.views = [dp.View(self.P[v], self.imgs[v]) for v in range(self.V)]
        self.seeds = np.ascontiguousarray(seeds)


def _rig(V, size, stride):
    cfg = synth.config(V, size[0], size[1], 1, seed_stride_px=stride)
    P, imgs, seeds = synth.scene_host(cfg)
    return cfg, P, imgs, seeds


def _border():
    _, P, imgs, seeds = _rig(6, BORDER_SIZE, 5.0)
    return Scene("border", P, imgs, seeds)


def _mixed():
    """the border scene's cameras; view v's image is its top-left W_v x H_v"""
    _, P, imgs, seeds = _rig(6, BORDER_SIZE, 5.0)
    crop = [np.ascontiguousarray(im[:h, :w]) for im, (w, h) in zip(imgs, MIXED_SIZES)]
    return Scene("mixed", P, crop, seeds)


def _zoomed(P, size, a):
    """the camera P with a times its focal length about the image centre"""
    cx, cy = 0.5 * size[0], 0.5 * size[1]
    Q = P.copy()
    Q[0] = a * P[0] + (1.0 - a) * cx * P[2]
    Q[1] = a * P[1] + (1.0 - a) * cy * P[2]
    return Q


def _budget():
    cfg, P, imgs, seeds = _rig(BUDGET_RIG, BUDGET_SIZE, 6.0)
    extra = [_zoomed(P[(5 * k + 2) % BUDGET_RIG], BUDGET_SIZE, a) for k, a in enumerate(BUDGET_ZOOMS)]
    V = BUDGET_RIG + len(extra)
    P = np.concatenate([P, np.stack(extra)])
    cfg2 = synth.config(V, BUDGET_SIZE[0], BUDGET_SIZE[1], 1, seed_stride_px=6.0)
    imgs = list(imgs) + [synth.render_host(cfg2, P, v) for v in range(BUDGET_RIG, V)]
    return Scene("budget", P, imgs, seeds)


@functools.lru_cache(maxsize=None)
def build(name) -> Scene:
    return {"border": _border, "mixed": _mixed, "budget": _budget}[name]()


_oracle = {}


def oracle_scene(orc, name, **options):
    """the oracle's scene (cached per option set; never modified by a test)"""
    key = (name, tuple(sorted(options.items())))
    if key not in _oracle:
        sc = build(name)
        _oracle[key] = orc.Scene(sc.P, sc.imgs, dp.Options(**options) if options else None)
    return _oracle[key]


def visible_list(vis):
    return [v for v in range(128) if (int(vis[v >> 6]) >> (v & 63)) & 1]


def mask_of(views):
    m = [0, 0]
    for v in views:
        m[v >> 6] |= 1 << (v & 63)
    return np.array(m, dtype=np.uint64)


def filter_views(fo):
    return fo.filter_max_views or fo.max_views


def stagings(orc, S, pat, cell, fo):
    """per patch the two stagings of its stored pose: the scoring one (margin 0,
    filter_max_views views: FAST_EVAL's, and the filter's at that pose) and the
    refine's (fo.margin, max_views views): (margin, M, m0, tiles) each"""
    ofo = orc.fast_options(fo)
    mg = min(fo.margin, 7)
    out = []
    for p in pat:
        out.append(((0,) + S.fast_stage_probe(p, cell, ofo, 0, filter_views(fo)),
                    (mg,) + S.fast_stage_probe(p, cell, ofo, mg, fo.max_views)))
    return out


def clamp_flags(sizes, margin, M, t):
    """which clamps of tile_rect a staged tile took: left, top, right, bottom,
    the even rounding of a left edge that stayed inside the image"""
    W, H = sizes[int(t["view"])]
    return dict(left=t["x0t"] == 0 and t["xa"] - M < 0,
                top=t["y0t"] == 0 and t["ya"] - M < 0,
                right=t["x0t"] + t["tw"] - 1 == W - 1 and t["xb"] + M >= W - 1,
                bottom=t["y0t"] + t["th"] - 1 == H - 1 and t["yb"] + M >= H - 1,
                odd=t["xa"] - M > 0 and (t["xa"] - M) % 2 == 1)


def tile_words(t):
    """32-bit words the device copies for a tile: (tw + 2) / 2 per row, th + 1 rows"""
    return ((int(t["tw"]) + 2) // 2) * (int(t["th"]) + 1)


# ---------------------------------------------------------------------------
# the patch sets (at most MAX_PATCHES each, chosen on the oracle's probe)
# ---------------------------------------------------------------------------
_patches = {}


def edge_patches(orc, name, cell=7):
    """border / mixed: seed patches whose stagings (the refine's at margin 2 and
    7, the scoring one at margin 0) clamp at an image edge, ten per side and
    margin, then patches that lose a visible view at the image border, then
    ordinary ones (no clamp, three or more views)"""
    if (name, cell) in _patches:
        return _patches[(name, cell)].copy()
    sc, S = build(name), oracle_scene(orc, name)
    pat = S.seeds_to_patches(sc.seeds)
    keys = ("left", "top", "right", "bottom", "odd")
    hit = {(k, mg): [] for k in keys for mg in (2, 7)}
    lost, plain = [], []
    both = [stagings(orc, S, pat, cell, dp.FastOptions(margin=mg)) for mg in (2, 7)]
    for i in range(len(pat)):
        any_flag = False
        for mg, st in zip((2, 7), both):
            flags = set()
            for margin, M, m0, tiles in st[i]:
                for t in tiles:
                    flags |= {k for k, on in clamp_flags(sc.sizes, margin, M, t).items() if on}
            for k in flags:
                hit[(k, mg)].append(i)
            any_flag |= bool(flags - {"odd"})
        nvis, m0 = len(visible_list(pat["vis"][i])), both[0][i][0][2]
        if 2 <= m0 < min(nvis, 32):
            lost.append(i)
        elif not any_flag and m0 >= 3:
            plain.append(i)
    order, seen = [], set()

    def take(rows, n):
        for i in rows:
            if n <= 0:
                break
            if i not in seen:
                seen.add(i)
                order.append(i)
                n -= 1

    for mg in (2, 7):
        for k in keys[:4]:
            take(hit[(k, mg)], 10)
    take(lost, 24)
    take(plain, 32)
    out = np.ascontiguousarray(pat[order[:MAX_PATCHES]])
    _patches[(name, cell)] = out
    return out.copy()


# staged-view counts of the budget scene's refine: mostly few views, which keep
# the full margin in the 16 KiB arena, and a tail of many, which cannot
BUDGET_KS = (2, 3, 4, 5, 3, 4, 6, 2, 5, 3, 4, 8, 11, 14, 18)


def budget_patches(orc):
    """budget: seed patches that two or more zoomed views see, the most widely
    seen first; patch i's visible set is cut to BUDGET_KS[i % 15] views: its
    first ones, or (every fifth patch) two zoomed views after the first rig
    views, so that the large tiles are staged last"""
    if "budget" in _patches:
        return _patches["budget"].copy()
    sc, S = build("budget"), oracle_scene(orc, "budget")
    pat = S.seeds_to_patches(sc.seeds)
    nvis = np.array([len(visible_list(v)) for v in pat["vis"]])
    zoom = np.array([sum(v >= BUDGET_RIG for v in visible_list(m)) for m in pat["vis"]])
    rows = np.flatnonzero(zoom >= 2)
    rows = rows[np.argsort(-nvis[rows], kind="stable")][:MAX_PATCHES]
    out = np.ascontiguousarray(pat[rows])
    for i in range(len(out)):
        vl = visible_list(out["vis"][i])
        k = BUDGET_KS[i % len(BUDGET_KS)]
        rig, zoomed = [v for v in vl if v < BUDGET_RIG], [v for v in vl if v >= BUDGET_RIG]
        keep = vl[:k] if i % 5 else rig[:max(k - 2, 1)] + zoomed[:2]
        out["vis"][i] = mask_of(keep)
    _patches["budget"] = out
    return out.copy()
