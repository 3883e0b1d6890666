"""The image cases of tests/imgcases.py are in the regime they are meant for,
checked on the oracle alone: a GPU test must never pass by missing its regime
(tests/test_gpu_dense.py and tests/test_gpu_planes.py use the same builders)."""
import numpy as np
import pytest

from tests import imgcases as ic


def _akaze_candidates(orc, img):
    return int(orc.akaze_candidates(img, ic.AKAZE_THRESHOLD).sum())


def test_candidate_accessor_equals_numpy_count(orc):
    """or_akaze_candidates counts what ak_extrema's rule says, restated here
    in numpy on the oracle's own Ldet planes (one small view, every level)."""
    img = ic.noise(200, 150, 5)
    info, _ = orc.akaze_levels(200, 150)
    got = orc.akaze_candidates(img, ic.AKAZE_THRESHOLD)
    assert len(got) == len(info) and got.sum() > 100
    sm = np.float32(10.0) * np.sqrt(np.float32(2.0))
    for lvl in range(len(info)):
        d, _ = orc.akaze_plane(img, lvl, 3)
        h, w = d.shape
        c = d[1:-1, 1:-1]
        m = (c > np.float32(ic.AKAZE_THRESHOLD)) & (c >= np.float32(0.00001))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    m &= c > d[1 + dy: h - 1 + dy, 1 + dx: w - 1 + dx]
        s = sm * np.float32(info[lvl, 3])
        y, x = np.mgrid[1: h - 1, 1: w - 1].astype(np.float32)
        m &= (np.rint(x - s) - 1 >= 0) & (np.rint(x + s) + 1 < w) & (np.rint(y - s) - 1 >= 0) & (np.rint(y + s) + 1 < h)
        assert int(m.sum()) == int(got[lvl]), lvl


def test_dense_akaze_views_exceed_the_lds_list(orc):
    """Every 640 x 480 noise view has more extrema candidates than the LDS
    suppression list holds, every 512 x 384 uniform-noise view fewer (the
    control), and the 512 x 384 0/255-noise view more again.  Measured:
    13090 / 13091 / 13079 (640 x 480 views 0-2), 7672 / 7680 / 7794
    (512 x 384), 9598 (512 x 384 0/255), 16397 (640 x 480 0/255)."""
    _, big = ic.match_set("noise", 640, 480)
    for v, im in enumerate(big):
        assert _akaze_candidates(orc, im) > ic.AKAZE_LIST_CAP, v
    _, small = ic.match_set("noise", 512, 384)
    for v, im in enumerate(small):
        assert 1000 < _akaze_candidates(orc, im) <= ic.AKAZE_LIST_CAP, v
    assert _akaze_candidates(orc, ic.noise01(512, 384, 5)) > ic.AKAZE_LIST_CAP
    assert _akaze_candidates(orc, ic.noise01(640, 480, 5)) > ic.AKAZE_LIST_CAP
    # the mixed set: the middle view over the cap, its neighbours under it
    _, mixed = ic.mixed_set()
    n = [_akaze_candidates(orc, im) for im in mixed]
    assert 0 < n[0] <= ic.AKAZE_LIST_CAP < n[1] and 0 < n[2] <= ic.AKAZE_LIST_CAP, n


def test_dense_akaze_list_is_shorter_than_the_candidates(orc):
    """The 0/255-noise 512 x 384 view: more candidates than the cap (9598) but
    fewer keypoints than it after suppression (6325), the case where the
    candidate count alone sends a view to the global list."""
    img = ic.noise01(512, 384, 5)
    r = orc.seeds_run(ic.cameras(1, 512, 384), [img],
                      orc.matcher_options(detector_type=orc.DETECTOR_AKAZE, akaze_threshold=ic.AKAZE_THRESHOLD))
    assert 0 < r["counts"]["detected"] < ic.AKAZE_LIST_CAP


@pytest.mark.parametrize("kind", ["noise", "noise01"])
def test_orb_retain_best_cuts_are_active(orc, kind):
    """With n_features = 500 the oracle detects strictly fewer keypoints than
    with 100000 on the same views (both retainBest cuts drop candidates); on
    the 0/255 noise it detects strictly more than the per-level quotas add up
    to, so a tie at a cut's threshold was kept."""
    P, imgs = ic.orb_set(kind)
    few = orc.seeds_run(P, imgs, orc.matcher_options(**ic.ORB_KW))["counts"]["detected"]
    many = orc.seeds_run(P, imgs, orc.matcher_options(**dict(ic.ORB_KW, n_features=100000)))["counts"]["detected"]
    quota = 3 * int(orc.features_per_level(ic.ORB_KW["n_features"], 1.2, ic.ORB_KW["n_levels"]).sum())
    assert quota <= few < many, (few, many, quota)
    # twice the quota still below what FAST finds: the first cut (2 n_l) is active too
    assert many > 2 * quota
    if kind == "noise01":
        assert few > quota, (few, quota)


def test_tall_view_has_keypoints_below_row_8191(orc):
    P, imgs = ic.tall_set()
    assert imgs[1].shape == (8320, 160, 3)
    r = orc.seeds_run(P, imgs, orc.matcher_options(detector_type=orc.DETECTOR_AKAZE,
                                                   akaze_threshold=ic.AKAZE_THRESHOLD))
    kp = r["keypoints"][1]
    assert int((kp["y"] >= 8192).sum()) >= 20
    assert len(r["keypoints"][0]) > 0 and len(r["keypoints"][2]) > 0


def test_content_cases_are_what_they_say():
    c = ic.content_cases(129, 33)
    for name, im in c.items():
        assert im.shape == (33, 129, 3) and im.dtype == np.uint8, name
    assert set(np.unique(c["noise01"])) == {0, 255} and set(np.unique(c["checker1"])) == {0, 255}
    assert np.array_equal(c["noise"][..., 0], c["noise"][..., 2])
    # independent channels: pixels where one channel is 0 and another 255
    for name in ("noise01_rgb", "checker1_rgb"):
        im = c[name].astype(int)
        assert np.any(im.max(axis=2) - im.min(axis=2) == 255), name
    assert c["checker2"][0, 0, 0] == c["checker2"][1, 1, 0] != c["checker2"][0, 2, 0]
    assert c["ramp"][0, 0, 0] == 0 and c["ramp"][0, -1, 0] == 255
    b = c["border"][..., 0]
    assert (b[0, 0], b[0, -1], b[-1, 0], b[-1, -1]) == (255, 0, 0, 255)
    for edge in (b[0, 1:-1], b[-1, 1:-1], b[1:-1, 0], b[1:-1, -1]):
        assert 0 in edge and 255 in edge
    assert np.all(b[1:-1, 1:-1] == 128)
    s = ic.shifted(c["noise"])
    assert np.array_equal(s[3:, 5:], c["noise"][:-3, :-5])
