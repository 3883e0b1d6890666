"""The staging scenes of tests/fastcases.py on the CPU: that the oracle's staging
probe (or_fast_stage_probe, which runs fast_stage itself) equals the numpy
restatement with the margin loop and the budget prefix, that the oracle's work
counters follow from the probe, and -- on the oracle alone -- that every scene is
the case it is named for.  tests/test_gpu_fast_edges.py runs the kernel on the
same scenes; a premise that fails here names the scene and the case it lacks."""
import collections

import numpy as np
import pytest

import densepoints_amd as dp

import fastcases as FC
from test_fast_spec_cpu import _fast_stage_numpy

MIN_PATCHES = 32


def need(cond, scene, case, got):
    assert cond, "scene %s lacks the case: %s (found %s)" % (scene, case, got)


def flags_of(sc, st):
    """per clamp kind the number of stagings with a tile that takes it"""
    cnt = collections.Counter()
    for pair in st:
        for margin, M, m0, tiles in pair:
            kinds = set()
            for t in tiles:
                kinds |= {k for k, on in FC.clamp_flags(sc.sizes, margin, M, t).items() if on}
            cnt.update(kinds)
    return cnt


# ---------------------------------------------------------------------------
# the probe against the restatement, the counters against the probe
# ---------------------------------------------------------------------------
def probe_cases(orc):
    """(scene, patches, cell, options): a few patches of every scene, the clamped
    ones first, at the margins and budgets the GPU tests use"""
    e, b = dp.FastOptions(), FC.budget_patches(orc)
    return [("border", FC.edge_patches(orc, "border")[::6], 7, dp.FastOptions(margin=7)),
            ("mixed", FC.edge_patches(orc, "mixed")[::6], 7, e),
            ("mixed", FC.edge_patches(orc, "mixed")[1::9], 11, dp.FastOptions(margin=7)),
            ("budget", b[::10], 16, dp.FastOptions(margin=7, tile_budget=16384, max_views=32)),
            ("budget", b[3::10], 11, dp.FastOptions(margin=7, tile_budget=6656, max_views=32)),
            ("budget", b[5::12], 16, dp.FastOptions(margin=0, tile_budget=FC.TINY_BUDGET, max_views=32))]


def test_stage_probe_equals_numpy_restatement(orc):
    """M, the staged views before the prefix and every kept tile's rectangle,
    footprint and window box: or_fast_stage_probe against _fast_stage_numpy"""
    seen = collections.Counter()
    for name, pat, cell, fo in probe_cases(orc):
        sc, S = FC.build(name), FC.oracle_scene(orc, name)
        for p, pair in zip(pat, FC.stagings(orc, S, pat, cell, fo)):
            for (margin, M, m0, tiles), cap in zip(pair, (FC.filter_views(fo), fo.max_views)):
                want = _fast_stage_numpy(orc, sc.P, sc.sizes, p, cell, fo.tile_budget, margin, cap)
                assert want is not None
                assert (M, m0) == (want["M"], want["m0"]), (name, cell, margin)
                assert [tuple(int(x) for x in t) for t in tiles] == want["tiles"], (name, cell, margin)
                seen["clipped"] += M < margin or len(tiles) < m0
                seen["stagings"] += 1
    assert seen["stagings"] >= 150 and seen["clipped"] >= 20, dict(seen)


@pytest.mark.parametrize("threads", [1, 5])
def test_eval_counters_follow_from_the_probe(orc, threads):
    """FAST_EVAL is one scoring staging per patch: the oracle's counters,
    recomputed in Python from the probe; the same for any thread count"""
    for name, pat, cell, fo in probe_cases(orc):
        S = FC.oracle_scene(orc, name)
        pat = pat.copy()
        pat["evals"] = np.arange(len(pat)) % 3  # what a patch brings along is counted
        want = dict(patches=len(pat), evals=int(pat["evals"].sum()) + len(pat), view_evals=0, staged_bytes=0,
                    clipped_stagings=0)
        for pair in FC.stagings(orc, S, pat, cell, fo):
            margin, M, m0, tiles = pair[0]
            want["view_evals"] += len(tiles) if len(tiles) >= 2 else 0
            want["staged_bytes"] += int(sum(t["bytes"] - 64 for t in tiles))
            want["clipped_stagings"] += M < margin or len(tiles) < m0
        S.fast_refine(pat, cell, orc.MODE_FAST_EVAL, orc.fast_options(fo), nthreads=threads)
        assert orc.fast_last_stats() == want, (name, cell)


def test_refine_counters_sum_over_patches_and_generations(orc):
    """the counters of a batch are the sums of its patches' (one at a time), an
    expansion counts four patches per parent, and GenerationEngine(fast=...)
    records one entry per generation"""
    S, fo = FC.oracle_scene(orc, "budget"), dp.FastOptions(margin=7, tile_budget=8192, max_views=32)
    pat = FC.budget_patches(orc)[:24]
    one = collections.Counter()
    for i in range(len(pat)):
        q = pat[i:i + 1].copy()
        S.fast_refine(q, 11, orc.MODE_FAST_REFINE, orc.fast_options(fo))
        one.update(orc.fast_last_stats())
    q = pat.copy()
    S.fast_refine(q, 11, orc.MODE_FAST_REFINE, orc.fast_options(fo))
    st = orc.fast_last_stats()
    assert st == dict(one) and st["evals"] == int(q["evals"].sum()) and st["clipped_stagings"] > 0
    kids, _ = S.fast_expand(q, orc.fast_options(fo))
    st = orc.fast_last_stats()
    assert st["patches"] == 4 * len(q) and st["evals"] == int(kids["evals"].sum()) > 0
    sc = FC.build("mixed")
    eng = orc.GenerationEngine(FC.oracle_scene(orc, "mixed", max_pops=40), threads=3, fast=dp.FastOptions(densify=1))
    out = eng.densify_all(sc.seeds[::40])
    assert len(eng.fast_stats) >= 2 and eng.fast_stats[0]["patches"] == len(sc.seeds[::40])
    assert sum(s["patches"] for s in eng.fast_stats[1:]) >= 4 * min(len(out), 40)


# ---------------------------------------------------------------------------
# premises: each scene is the case it claims to be (the oracle alone)
# ---------------------------------------------------------------------------
def test_border_scene_premises(orc):
    sc, S, pat = FC.build("border"), FC.oracle_scene(orc, "border"), FC.edge_patches(orc, "border")
    need(MIN_PATCHES <= len(pat) <= FC.MAX_PATCHES, "border", "32 .. 160 patches", len(pat))
    assert set(sc.sizes) == {FC.BORDER_SIZE}
    for fo in (dp.FastOptions(), dp.FastOptions(margin=7)):
        cnt = flags_of(sc, FC.stagings(orc, S, pat, 7, fo))
        print("border, margin %d: stagings clamped %s" % (fo.margin, dict(cnt)))
        for side in ("left", "top", "right", "bottom"):
            need(cnt[side] >= 8, "border", "8 stagings clamped at the %s edge, margin %d" % (side, fo.margin), cnt[side])
        need(cnt["odd"] >= 8, "border", "8 stagings whose xa - M is odd, margin %d" % fo.margin, cnt["odd"])
        q = pat.copy()
        acc = S.fast_refine(q, 7, orc.MODE_FAST_REFINE, orc.fast_options(fo))
        need(acc.sum() >= MIN_PATCHES, "border", "32 accepted patches, margin %d" % fo.margin, int(acc.sum()))


def test_border_scene_drops_views_by_less_than_a_pixel(orc):
    """visible views whose window box fails View::IsPointInside by less than a
    pixel: dropped from the staging (the restatement names the miss)"""
    sc, S, pat = FC.build("border"), FC.oracle_scene(orc, "border"), FC.edge_patches(orc, "border")
    near = 0
    for p in pat:
        M, m0, tiles = S.fast_stage_probe(p, 7, None, 0, 32)
        if m0 == len(FC.visible_list(p["vis"])):
            continue
        want = _fast_stage_numpy(orc, sc.P, sc.sizes, p, 7, 6656, 0, 32)
        assert m0 == want["m0"] and [int(t["view"]) for t in tiles] == [t[0] for t in want["tiles"]]
        near += sum(1 for v, why, miss in want["dropped"] if why == "inside" and miss < 1.0)
    need(near >= 4, "border", "4 views dropped for a window box less than a pixel outside", near)


def test_mixed_scene_premises(orc):
    sc, S, pat = FC.build("mixed"), FC.oracle_scene(orc, "mixed"), FC.edge_patches(orc, "mixed")
    need(MIN_PATCHES <= len(pat) <= FC.MAX_PATCHES, "mixed", "32 .. 160 patches", len(pat))
    assert sc.sizes == FC.MIXED_SIZES and len(set(sc.sizes)) >= 4
    need(sum(w % 2 for w, _ in sc.sizes) >= 2, "mixed", "odd widths", sc.sizes)
    need(len({FC.gray_pitch(w) for w, _ in sc.sizes}) >= 2, "mixed", "two gray pitches", sc.sizes)
    assert np.array_equal(sc.P, FC.build("border").P)
    for fo in (dp.FastOptions(), dp.FastOptions(margin=7)):
        st = FC.stagings(orc, S, pat, 7, fo)
        three = sum(max(len({sc.sizes[int(t["view"])] for t in s[3]}) for s in pair) >= 3 for pair in st)
        odd_right = sum(1 for pair in st for margin, M, m0, tiles in pair
                        if any(sc.sizes[int(t["view"])][0] % 2 == 1 and FC.clamp_flags(sc.sizes, margin, M, t)["right"]
                               for t in tiles))
        print("mixed, margin %d: %d patches stage three sizes at once, %d stagings clamp at an odd width's right edge, "
              "clamped %s" % (fo.margin, three, odd_right, dict(flags_of(sc, st))))
        need(three >= MIN_PATCHES, "mixed", "32 patches staging views of three sizes at once, margin %d" % fo.margin,
             three)
        need(odd_right >= 8, "mixed", "8 stagings clamped at the right edge of an odd-width view, margin %d" % fo.margin,
             odd_right)
        q = pat.copy()
        acc = S.fast_refine(q, 7, orc.MODE_FAST_REFINE, orc.fast_options(fo))
        need(acc.sum() >= MIN_PATCHES, "mixed", "32 accepted patches, margin %d" % fo.margin, int(acc.sum()))


@pytest.mark.parametrize("cell", [16, 11])
def test_budget_scene_premises(orc, cell):
    sc, S, pat = FC.build("budget"), FC.oracle_scene(orc, "budget"), FC.budget_patches(orc)
    need(MIN_PATCHES <= len(pat) <= FC.MAX_PATCHES, "budget", "32 .. 160 patches", len(pat))
    assert sc.V == 24 and set(sc.sizes) == {FC.BUDGET_SIZE}
    words = 0
    for margin, budget in FC.BUDGETS:
        fo = dp.FastOptions(margin=margin, tile_budget=budget, max_views=32)
        ref = [pair[1] for pair in FC.stagings(orc, S, pat, cell, fo)]
        hist = collections.Counter(M for _, M, _, _ in ref)
        dropped0 = sum(1 for _, M, m0, tiles in ref if M == 0 and len(tiles) < m0)
        clipped = sum(1 for mg, M, m0, tiles in ref if M < mg or len(tiles) < m0)
        arena = max(sum(int(t["bytes"]) for t in tiles) for _, _, _, tiles in ref)
        big = max(((FC.tile_words(t), int(t["tw"]), int(t["th"])) for _, _, _, tiles in ref for t in tiles))
        words = max(words, big[0])
        print("budget, cell %d, margin %d, budget %d: M histogram %s, M = 0 with views dropped %d, clipped %d, "
              "largest tile %d words (%d x %d), fullest arena %d bytes"
              % (cell, margin, budget, sorted(hist.items()), dropped0, clipped, big[0], big[1], big[2], arena))
        case = "cell %d, margin %d, budget %d: " % (cell, margin, budget)
        assert arena <= budget and max(t["tw"] for _, _, _, tl in ref for t in tl) <= 63
        need(clipped > 0, "budget", case + "a clipped staging", clipped)
        if budget == 16384:
            need(2 * hist[7] > len(pat), "budget", case + "most patches keep M = 7", hist[7])
        else:
            need(sum(hist[M] for M in range(1, 7)) >= 8, "budget", case + "8 stagings with 0 < M < 7", dict(hist))
            need(dropped0 >= 4, "budget", case + "4 stagings at M = 0 that drop views", dropped0)
    if cell == 16:
        need(words >= 1500, "budget", "a tile of 1,500 words", words)
    # margin 0 and a budget of one small tile: the prefix leaves the anchor alone
    fo = dp.FastOptions(margin=0, tile_budget=FC.TINY_BUDGET, max_views=32)
    alone = sum(1 for pair in FC.stagings(orc, S, pat, cell, fo) if pair[0][2] >= 2 and len(pair[0][3]) < 2)
    q = pat.copy()
    S.fast_refine(q, cell, orc.MODE_FAST_EVAL, orc.fast_options(fo))
    print("budget, cell %d, budget %d: %d stagings keep fewer than two views" % (cell, FC.TINY_BUDGET, alone))
    need(alone >= 8 and (q["score"] == -1.0).sum() >= alone, "budget",
         "cell %d: 8 patches scored -1 because the prefix keeps fewer than two views" % cell, alone)
