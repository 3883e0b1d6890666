"""Deterministic BGR8 test images of the content that image kernels get wrong:
dense noise, saturated runs, 0/255 alternation, single border pixels.  The
synth scenes are smooth; these are not.  Every builder takes (W, H) and
returns an H x W x 3 uint8 array; cameras come from synth.cameras.

A GPU test that uses a case for a regime (more AKAZE candidates than the LDS
list holds, active retainBest cuts, keypoints below row 8191) has the regime
itself asserted on the oracle alone in tests/test_imgcases_cpu.py."""
import functools

import numpy as np

from densepoints_amd import synth

AKAZE_THRESHOLD = 0.0002
AKAZE_LIST_CAP = 9216  # kAkListCap (densepoints_amd/csrc/dp_akaze.h)


def _bgr(plane):
    return np.ascontiguousarray(np.repeat(plane[:, :, None], 3, axis=2).astype(np.uint8))


def noise(W, H, seed, independent=False):
    """uniform random bytes; the same in B, G and R unless independent"""
    rng = np.random.default_rng(seed)
    if independent:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return _bgr(rng.integers(0, 256, (H, W), dtype=np.uint8))


def noise01(W, H, seed, independent=False):
    """every byte 0 or 255; independent: each channel saturates on its own"""
    rng = np.random.default_rng(seed)
    if independent:
        return (rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return _bgr(rng.integers(0, 2, (H, W), dtype=np.uint8) * 255)


def constant(W, H, value):
    return np.full((H, W, 3), value, dtype=np.uint8)


def checker(W, H, cell, independent=False):
    """cell-px checkerboard of 0/255; independent: G is the inverse board and
    R the board one pixel to the right, so the channels saturate apart"""
    y, x = np.mgrid[0:H, 0:W]
    b = ((((x // cell) + (y // cell)) & 1) * 255).astype(np.uint8)
    if not independent:
        return _bgr(b)
    r = (((((x + 1) // cell) + (y // cell)) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([b, 255 - b, r], axis=2))


def ramp(W, H):
    """horizontal ramp 0 .. 255 over the width"""
    row = (np.arange(W, dtype=np.int64) * 255 // max(W - 1, 1)).astype(np.uint8)
    return _bgr(np.broadcast_to(row, (H, W)))


def border_impulses(W, H):
    """constant 128 with single 255 and 0 pixels on the four corners and
    along each border row and column (every 7th pixel, alternating)"""
    p = np.full((H, W), 128, dtype=np.uint8)
    xs, ys = np.arange(3, W - 1, 7), np.arange(3, H - 1, 7)
    p[0, xs] = np.where(np.arange(len(xs)) & 1, 0, 255)
    p[H - 1, xs] = np.where(np.arange(len(xs)) & 1, 255, 0)
    p[ys, 0] = np.where(np.arange(len(ys)) & 1, 0, 255)
    p[ys, W - 1] = np.where(np.arange(len(ys)) & 1, 255, 0)
    p[0, 0], p[0, W - 1], p[H - 1, 0], p[H - 1, W - 1] = 255, 0, 0, 255
    return _bgr(p)


def shifted(img, dx=5, dy=3):
    """img moved by (dx, dy) px; the uncovered strip keeps img's own pixels"""
    out = img.copy()
    out[dy:, dx:] = img[: img.shape[0] - dy, : img.shape[1] - dx]
    return out


def content_cases(W, H, seed=5):
    """name -> image: the saturated and dense content at one size"""
    return {
        "noise": noise(W, H, seed),
        "noise01": noise01(W, H, seed),
        "noise01_rgb": noise01(W, H, seed, independent=True),
        "const255": constant(W, H, 255),
        "const0": constant(W, H, 0),
        "checker1": checker(W, H, 1),
        "checker2": checker(W, H, 2),
        "checker1_rgb": checker(W, H, 1, independent=True),
        "ramp": ramp(W, H),
        "border": border_impulses(W, H),
    }


def cameras(n_views, W, H):
    return synth.cameras(synth.config(n_views=n_views, width=W, height=H, kind=0))


def match_set(kind, W, H, seed=5):
    """three views for the matching stages: view 1 is view 0 shifted by
    (5, 3) px, so descriptors match densely; view 2 is independent"""
    f = {"noise": noise, "noise01": noise01}[kind]
    v0 = f(W, H, seed)
    return cameras(3, W, H), [v0, shifted(v0), f(W, H, seed + 1)]


@functools.lru_cache(maxsize=None)
def synth_views(W, H, n=2):
    cfg = synth.config(n_views=n, width=W, height=H, kind=0)
    P = synth.cameras(cfg)
    return P, [synth.render_host(cfg, P, v) for v in range(n)]


def mixed_set(seed=5):
    """one 640 x 480 noise view (over the LDS cap) between two 320 x 240
    synth views (under it)"""
    P, im = synth_views(320, 240)
    return cameras(3, 640, 480), [im[0], noise(640, 480, seed), im[1]]


TALL_W, TALL_H, TALL_Y0 = 160, 8320, 8100


def tall_set(seed=5):
    """a 160 x 8320 view, constant 128 but for uniform noise in rows 8100 and
    below (keypoints at level-0 y > 8191), beside two small synth views"""
    t = constant(TALL_W, TALL_H, 128)
    t[TALL_Y0:] = noise(TALL_W, TALL_H - TALL_Y0, seed)
    P, im = synth_views(320, 240)
    return cameras(3, 320, 240), [im[0], t, im[1]]


# ORB retainBest: few features against thousands of FAST corners.  Seed 12:
# on the 0/255 noise two Harris responses tie at a level's cut (most seeds
# have no tie there), so the keep-ties rule decides the keypoint count.
ORB_KW = dict(n_features=500, n_levels=3, fast_threshold=20)
ORB_SEED = 12


def orb_set(kind):
    return match_set(kind, 320, 240, ORB_SEED)
