"""Seed generation on dense and saturated views (tests/imgcases.py) against
the oracle, bit for bit at every stage (compare_run).  The synth scenes give
about 200 keypoints per view; these give thousands, so the AKAZE suppression
list leaves LDS, ORB's retainBest cuts drop candidates and keep ties, and a
tall view puts keypoints below row 8191.  tests/test_imgcases_cpu.py asserts
each of those regimes on the oracle alone."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import matcher as M
from tests import imgcases as ic
from tests.test_gpu_seeds import compare_run, engine_with

pytestmark = pytest.mark.gpu

AKAZE_KW = dict(detector_type=M.DETECTOR_AKAZE, akaze_threshold=ic.AKAZE_THRESHOLD)


def _both(orc, P, imgs, kw):
    r = orc.seeds_run(P, imgs, orc.matcher_options(**kw))
    with engine_with(P, imgs) as eng:
        m = compare_run(eng, r, kw, len(imgs))
    return r, m


def test_akaze_dense_views_global_list(orc):
    """Three 640 x 480 noise views, each with about 13,000 extrema candidates
    (more than the 9216 the LDS list holds): the suppression runs on the
    global list and equals the oracle; view 1 is view 0 shifted, so the
    match tables are dense."""
    P, imgs = ic.match_set("noise", 640, 480)
    r, m = _both(orc, P, imgs, AKAZE_KW)
    assert r["counts"]["detected"] > 3 * 3000 and r["counts"]["ratio_matches"] > 100


def test_akaze_dense_views_lds_control(orc):
    """Three 512 x 384 noise views, about 7,700 candidates each: the LDS list."""
    P, imgs = ic.match_set("noise", 512, 384)
    r, m = _both(orc, P, imgs, AKAZE_KW)
    assert r["counts"]["detected"] > 3 * 2000


def test_akaze_mixed_lists_in_one_launch(orc):
    """A 640 x 480 noise view (global list) between two 320 x 240 synth views
    (LDS list) in one launch: the global slice is the middle view's own."""
    P, imgs = ic.mixed_set()
    r, m = _both(orc, P, imgs, AKAZE_KW)
    assert all(len(k) > 0 for k in r["keypoints"])


def test_akaze_saturated_view_candidates_over_list_under(orc):
    """The 0/255-noise 512 x 384 view: 9598 candidates, fewer list entries."""
    imgs = [ic.noise01(512, 384, 5), ic.shifted(ic.noise01(512, 384, 5))]
    _both(orc, ic.cameras(2, 512, 384), imgs, AKAZE_KW)


def test_akaze_tall_view_key_packing(orc):
    """A 160 x 8320 view with its keypoints at y > 8191: the list key holds
    14 bits of y (13 bits carried y into the level field)."""
    P, imgs = ic.tall_set()
    r, m = _both(orc, P, imgs, AKAZE_KW)
    assert int((r["keypoints"][1]["y"] >= 8192).sum()) >= 20


def test_akaze_rejects_views_beyond_the_key(orc):
    """32 x 16384: one row more than the key's 14 bits address -- DP_E_ARG
    before any kernel runs."""
    img = ic.constant(32, 16384, 128)
    with engine_with(ic.cameras(1, 32, 16384), [img]) as eng:
        with pytest.raises(dp.DensePointsError) as e:
            M.Matcher(eng, M.MatcherOptions(**AKAZE_KW)).generate_seeds()
        assert "16383" in str(e.value)


@pytest.mark.parametrize("kind,extra", [("noise", {}), ("noise01", {}), ("noise01", dict(edge_threshold=19))])
def test_orb_retain_best_on_dense_views(orc, kind, extra):
    """n_features = 500 on 320 x 240 noise: the FAST-score histogram cut and
    the Harris cut both drop candidates, and on the 0/255 noise a Harris tie
    at a cut is kept (1501 detected against quotas of 1500)."""
    P, imgs = ic.orb_set(kind)
    kw = dict(ic.ORB_KW, **extra)
    r, m = _both(orc, P, imgs, kw)
    assert r["counts"]["ratio_matches"] > 50
