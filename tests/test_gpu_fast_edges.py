"""The performance mode (dp_fast_kernel.hip) where its staging comes closest to its
limits, against the oracle (or_fast.c) bit for bit on every field, and its work
counters (dp_fast_last_stats) against the oracle's, exactly:

  arenas    every tile arena -- FastLds<6656>, <8192> and <16384>, the last both
            at its first budget (8193) and at its largest -- at one window shape of
            each pass width and the tail-round shape (cells 16, 11, 7, 5), in
            FAST_EVAL, the refine with forward differences and with the analytic
            gradient, and the expansion; margin 7, 32 staged views, on the budget
            scene (tests/fastcases.py): tiles of up to 1,798 words, every margin
            0 .. 7, the budget prefix; and the device-resident BFS instance of
            the largest arena (a densify);
  edges     tiles clamped at each image edge, left edges rounded to an even
            column, views of unequal size with odd widths and two gray pitches
            in one staging (the border and mixed scenes), at the default options
            and at margin 7; a densify over the mixed-size views.

tests/test_fastcases_cpu.py asserts, on the oracle alone, that the scenes are
these cases.  The references are computed once per launch description and
shared."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

import fastcases as FC
from test_gpu_parity import FIELDS, assert_same, scene

pytestmark = pytest.mark.gpu

CELLS = [16, 11, 7, 5]
BUDGETS = [6656, 8192, 8193, 16384]


class Case:
    """a scene, the oracle's scene per option set and one engine with its views"""

    def __init__(self, orc, name, eng):
        self.name, self.sc, self.orc, self.eng = name, FC.build(name), orc, eng
        eng.set_views(self.sc.views)

    def oracle(self, **options):
        return FC.oracle_scene(self.orc, self.name, **options)

    def refine(self, pat, cell, mode, fo):
        """one launch on both sides: accept flags, every field and the five
        counters equal; returns the oracle's patches"""
        gp, op = pat.copy(), pat.copy()
        self.eng.set_fast_options(fo)
        try:
            ga = self.eng.fast_refine(gp, cell, mode)
            gst = self.eng.fast_last_stats()
        finally:
            self.eng.set_fast_options(dp.FastOptions())
        oa = self.oracle().fast_refine(op, cell, mode, fo=self.orc.fast_options(fo))
        ost = self.orc.fast_last_stats()
        assert np.array_equal(ga, oa), "accept flags differ"
        assert_same(gp, op)
        assert gst == ost
        return op, ost

    def expand(self, parents, cell, fo):
        o = dp.Options(expand_cell_size=cell)
        self.eng.set_options(o)
        self.eng.set_fast_options(fo)
        try:
            gk, ga = self.eng.fast_expand(parents)
            gst = self.eng.fast_last_stats()
        finally:
            self.eng.set_fast_options(dp.FastOptions())
            self.eng.set_options(dp.Options())
        ok, oa = self.oracle(expand_cell_size=cell).fast_expand(parents, self.orc.fast_options(fo))
        ost = self.orc.fast_last_stats()
        assert np.array_equal(ga, oa), "accept flags differ"
        assert_same(gk, ok, FIELDS + ("parent",))
        assert gst == ost and ost["patches"] == 4 * len(parents)
        return ok, oa, ost

    def all_modes(self, pat, cell, fo_kw):
        """FAST_EVAL, the refine with either gradient, and the expansion of the
        refined patches (some of them dead parents: too few views left)"""
        fo = dp.FastOptions(**fo_kw)
        _, est = self.refine(pat, cell, N.MODE_FAST_EVAL, fo)
        par, rst = self.refine(pat, cell, N.MODE_FAST_REFINE, fo)
        q, _ = self.refine(pat, cell, N.MODE_FAST_REFINE, dp.FastOptions(gradient=1, **fo_kw))
        assert par["evals"].mean() > 10 and q["evals"].mean() > 5
        kids, acc, xst = self.expand(par, cell, fo)
        return est, rst, xst, acc


@pytest.fixture(scope="module")
def budget(orc):
    with dp.Engine(device=0) as eng:
        yield Case(orc, "budget", eng)


@pytest.fixture(scope="module")
def border(orc):
    with dp.Engine(device=0) as eng:
        yield Case(orc, "border", eng)


@pytest.fixture(scope="module")
def mixed(orc):
    with dp.Engine(device=0) as eng:
        yield Case(orc, "mixed", eng)


# ---------------------------------------------------------------------------
# arenas
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("tile_budget", BUDGETS)
def test_arena_bit_exact_with_counters(budget, orc, tile_budget, cell):
    pat = FC.budget_patches(orc)
    assert len(pat) <= FC.MAX_PATCHES
    est, rst, xst, acc = budget.all_modes(pat, cell, dict(margin=7, tile_budget=tile_budget, max_views=32))
    # the launch is the case: margins were cut (or, in the largest arena at the
    # small windows, at least the counters moved), children were accepted
    assert rst["clipped_stagings"] > 0 and rst["staged_bytes"] > est["staged_bytes"] > 0
    assert rst["view_evals"] > est["view_evals"] > 0 and acc.sum() > 0


@pytest.mark.parametrize("cell", [16, 11])
def test_budget_prefix_leaves_the_anchor_alone(budget, orc, cell):
    """margin 0 and a budget of one small tile: fewer than two views fit, the
    score is -1 and nothing is sampled"""
    pat = FC.budget_patches(orc)
    fo = dp.FastOptions(margin=0, tile_budget=FC.TINY_BUDGET, max_views=32)
    op, st = budget.refine(pat, cell, N.MODE_FAST_EVAL, fo)
    assert (op["score"] == -1.0).sum() >= 8 and st["clipped_stagings"] >= 8
    budget.refine(pat, cell, N.MODE_FAST_REFINE, fo)


def test_counters_include_what_a_patch_brings_along(budget, orc):
    """dp_fast_stats.evals is the sum of the patches' evals fields after the
    launch (include/densepoints.h): a patch refined again brings its count along"""
    pat = FC.budget_patches(orc)[:64]
    pat["evals"] = 3 + np.arange(len(pat)) % 5
    fo = dp.FastOptions(margin=7, tile_budget=8192, max_views=32)
    op, st = budget.refine(pat, 11, N.MODE_FAST_REFINE, fo)
    assert st["evals"] == int(op["evals"].sum()) and (op["evals"] > pat["evals"]).all()


def densify_both(orc, sc, S, opts, fo):
    """dp_densify against GenerationEngine.densify_all on every stored field, and
    the counters of the expansion generations.  dp_fast_last_stats reads the
    last batch of device-resident generations (up to eight, counted as one
    launch; the seed stage is a launch of its own before it), so max_pops is
    chosen small enough for the whole BFS to finish in one batch -- asserted
    here on the oracle.  A generation's parents at or past the pop cap do not
    expand: their four children count as patches and nothing else."""
    eng = orc.GenerationEngine(S, threads=8, fast=fo)
    g = eng.densify_begin(sc.seeds)
    want = dict.fromkeys(orc.FAST_STATS, 0)
    gens = 0
    while g.items:
        cand, acc = eng.densify_refine(g, 0, g.items)
        if g.index > 0:
            gens += 1
            assert 4 * g.items <= 1024, "the generation would outgrow the smallest candidate buffer"
            live = min(g.items, max(int(opts.max_pops) - g.head, 0))
            S.fast_expand(np.array(eng.store[g.head:g.head + live], dtype=orc.PATCH_DTYPE), orc.fast_options(fo), 8)
            st = orc.fast_last_stats()
            st["patches"] = 4 * g.items
            for k in want:
                want[k] += st[k]
        g = eng.densify_commit(g, cand, acc)
    assert 2 <= gens <= 8, "%d expansion generations: not one batch of the device-resident BFS" % gens
    op = np.array(eng.store, dtype=orc.PATCH_DTYPE)
    with dp.Engine(opts, device=0) as e:
        e.set_views(sc.views)
        e.set_fast_options(fo)
        gp, gst = e.densify(sc.seeds)
        fst = e.fast_last_stats()
    assert gst["patches"] == len(op) > 20
    assert_same(gp, op, FIELDS + ("seq", "parent", "rgb"))
    assert fst == want and want["view_evals"] > 0
    return want


def test_densify_in_the_large_arena(orc):
    """the device-resident BFS instance of FastLds<16384> (hf6, margin 7; every
    fourth seed and 120 pops: two generations)"""
    sc = scene("hf6")
    opts = dp.Options(max_pops=120)
    densify_both(orc, FC.Scene("hf6", sc.P, sc.imgs, sc.seeds[::4]), orc.Scene(sc.P, sc.imgs, opts), opts,
                 dp.FastOptions(densify=1, tile_budget=16384, margin=7))


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
@pytest.fixture
def case(request, border, mixed):
    return {"border": border, "mixed": mixed}[request.param]


@pytest.mark.parametrize("fo_kw", [dict(), dict(margin=7)], ids=["default", "margin7"])
@pytest.mark.parametrize("cell", [7, 11])
@pytest.mark.parametrize("case", ["border", "mixed"], indirect=True)
def test_edges_bit_exact_with_counters(case, orc, cell, fo_kw):
    pat = FC.edge_patches(orc, case.name)
    assert case.eng.view_sizes() == case.sc.sizes
    est, rst, xst, acc = case.all_modes(pat, cell, fo_kw)
    assert acc.sum() > 0 and rst["view_evals"] > est["view_evals"] > 0


def test_densify_over_views_of_unequal_size(orc):
    sc = FC.build("mixed")
    opts = dp.Options(max_pops=120)
    densify_both(orc, FC.Scene("mixed", sc.P, sc.imgs, sc.seeds[::20]), FC.oracle_scene(orc, "mixed", max_pops=120), opts,
                 dp.FastOptions(densify=1))
