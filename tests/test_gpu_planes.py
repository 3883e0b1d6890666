"""Whole image planes against the oracle, every pixel, borders included:
the AKAZE scale space (Lt, Lx, Ly, Ldet per level) and ORB's gray pyramid as
seed generation builds them (the probes run its own launch sequence), the
BGR pyramid of dp_build_pyramid and the gray planes.  Keypoints lie well
inside a plane, so a wrong halo column or reflected tap shows only here.
Sizes sit on the kernels' tile edges (64-wide AKAZE tiles, 64 x 16 outputs of
128 x 32 inputs for pyr_down) and below one tile; content is tests/imgcases.py's
noise, saturated runs, 0/255 alternation and border impulses."""
import numpy as np
import pytest

import densepoints_amd as dp
from tests import imgcases as ic

pytestmark = pytest.mark.gpu

PLANE_SIZES = [(64, 48), (65, 49), (127, 95), (128, 96), (129, 97), (200, 41)]
PLANE_CASES = ("noise", "noise01", "checker1", "checker2", "const255", "border")
PLANE_NAMES = ("Lt", "Lx", "Ly", "Ldet")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _engine(imgs):
    W, H = imgs[0].shape[1], imgs[0].shape[0]
    P = ic.cameras(len(imgs), W, H)
    eng = dp.Engine()
    eng.set_views([dp.View(P[v], imgs[v]) for v in range(len(imgs))])
    return eng


def _compare_akaze_planes(orc, imgs):
    H, W = imgs[0].shape[:2]
    n_levels = len(orc.akaze_levels(W, H)[0])
    with _engine(imgs) as eng:
        for v, im in enumerate(imgs):
            for lvl in range(n_levels):
                for which in range(4):
                    want, _ = orc.akaze_plane(im, lvl, which)
                    got = eng.probe_akaze_plane(v, lvl, which)
                    assert got.shape == want.shape
                    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                    assert len(bad) == 0, (f"view {v} level {lvl} {PLANE_NAMES[which]}: {len(bad)} pixels differ, "
                                           f"first (y, x) {bad[:4].tolist()} of {want.shape}")
        with pytest.raises(dp.DensePointsError):
            eng.probe_akaze_plane(0, n_levels, 0)
    return n_levels


@pytest.mark.parametrize("size", PLANE_SIZES + [(161, 81)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_akaze_planes_equal_oracle(orc, size):
    W, H = size
    c = ic.content_cases(W, H)
    n = _compare_akaze_planes(orc, [c[k] for k in PLANE_CASES])
    assert n == (8 if size == (161, 81) else 4)  # 161 x 81 halves odd sides into a second octave (80 x 40)


@pytest.mark.parametrize("steps", [1, 4])
def test_akaze_planes_fed_steps_per_launch(orc, monkeypatch, steps):
    """DP_AKAZE_FED_STEPS 1 and 4 (the default): the multi-step FED tiles'
    halos reach the plane border at 129 x 97 in every tile."""
    monkeypatch.setenv("DP_AKAZE_FED_STEPS", str(steps))
    c = ic.content_cases(129, 97)
    _compare_akaze_planes(orc, [c["noise"], c["border"]])


def test_akaze_planes_of_views_in_later_chunks(orc, monkeypatch):
    """A chunk budget of one byte puts each of 3 views of 160 x 120 in a chunk
    of its own: the probe runs the chunks before its view's and stops after it."""
    monkeypatch.setenv("DP_AKAZE_CHUNK_BYTES", "1")
    c = ic.content_cases(160, 120)
    assert _compare_akaze_planes(orc, [c["noise"], c["border"], c["noise01"]]) == 8


@pytest.mark.parametrize("size", PLANE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_orb_gray_levels_equal_oracle(orc, size):
    W, H = size
    c = ic.content_cases(W, H)
    names = PLANE_CASES + ("noise01_rgb", "checker1_rgb")
    imgs = [c[k] for k in names]
    L = 4
    with _engine(imgs) as eng:
        for v, im in enumerate(imgs):
            for lvl in range(L):
                want = orc.orb_level(im, lvl, L)
                got = eng.probe_orb_level(v, lvl, L)
                assert got.shape == want.shape
                bad = np.argwhere(got != want)
                assert len(bad) == 0, f"{names[v]} level {lvl}: {len(bad)} pixels differ, first {bad[:4].tolist()}"


PYR_CASES = ("const255", "const0", "checker1", "checker2", "noise01", "noise01_rgb", "noise")


@pytest.mark.parametrize("W", [127, 128, 129, 131])
@pytest.mark.parametrize("H", [31, 32, 33])
def test_pyramid_tile_edges_equal_oracle(orc, W, H):
    """dp_build_pyramid against orc.pyr_down around one 128 x 32 input tile."""
    c = ic.content_cases(W, H)
    imgs = [c[k] for k in PYR_CASES]
    levels = 3
    with _engine(imgs) as eng:
        eng.build_pyramid(levels)
        for v, im in enumerate(imgs):
            ref = im
            for lvl in range(1, levels):
                ref = orc.pyr_down(ref)
                got = eng.read_level(lvl, v)
                assert got.shape == ref.shape
                assert np.array_equal(got, ref), f"{PYR_CASES[v]} level {lvl}"


@pytest.mark.parametrize("size", [(2, 2), (3, 5), (5, 3), (4, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_tiny_views_down_to_one_pixel(orc, size):
    """Views smaller than the 5-tap filter: BORDER_REFLECT_101 folds more than
    once, down to a 1 x 1 level (cv::pyrDown takes any size)."""
    W, H = size
    c = ic.content_cases(W, H)
    imgs = [c[k] for k in ("noise", "noise01_rgb", "checker1", "const255")]
    levels = 4
    with _engine(imgs) as eng:
        eng.build_pyramid(levels)
        for v, im in enumerate(imgs):
            ref = im
            for lvl in range(1, levels):
                ref = orc.pyr_down(ref)
                got = eng.read_level(lvl, v)
                assert got.shape == ref.shape
                assert np.array_equal(got, ref), f"view {v} level {lvl}"
            assert ref.shape[:2] == (1, 1)


def test_gray_planes_saturated_content(orc):
    """read_gray against Scene.gray at 129 x 33 on every content case, the
    independent-channel ones included (BGR -> gray with saturated channels)."""
    c = ic.content_cases(129, 33)
    names = sorted(c)
    imgs = [c[k] for k in names]
    S = orc.Scene(ic.cameras(len(imgs), 129, 33), imgs)
    with _engine(imgs) as eng:
        for v in range(len(imgs)):
            g = eng.read_gray(v)
            assert np.array_equal(g.astype(np.int32) - 1024, S.gray(v).astype(np.int32)), names[v]
