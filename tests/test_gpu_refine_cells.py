"""The parity refine against the oracle, bit for bit, at every window size 2 .. 16
and in every view-pass width's kernel (G = 8, 4, 2, 1): every mode at every
cell, and per G the view-count edges of a pass and of a map chunk, 64-bit tap
addressing, an unsafe window in one slot, two row pitches in one pass, views
past 63, the edge patches, the whole densify on the device-resident generation
kernels and repeatability.  tests/refinecases.py builds the inputs and
tests/test_refinecases_cpu.py asserts, on the oracle alone, that each is the
case it is meant to be; the premises that cost nothing are asserted here too.
No comparison has a tolerance."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import dist as D

import refinecases as RC
from refinecases import assert_same

pytestmark = pytest.mark.gpu


class Device:
    """one engine for the module; views are uploaded when the scene changes"""

    def __init__(self, eng):
        self.eng, self.key = eng, None

    def use(self, key, P, imgs):
        if self.key != key:
            self.eng.set_views(RC.views_of(P, imgs))
            self.key = key
        return self.eng


@pytest.fixture(scope="module")
def device():
    with dp.Engine(device=0) as eng:
        yield Device(eng)


def compare(eng, pat, want, cell, mode):
    """engine.refine of a copy of `pat` equals the oracle's (patches, accept)"""
    op, oa = want
    gp = pat.copy()
    ga = eng.refine(gp, cell, mode)
    assert np.array_equal(ga, oa), f"cell {cell} mode {RC.MODE_NAME[mode]}: accept flags differ"
    assert_same(gp, op)
    return op


def use_hf6(device):
    sc = RC.scene("hf6")
    return device.use("hf6", sc.P, sc.imgs)


# ---------------------------------------------------------------------------
# 1. every cell, every mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RC.ALL_MODES, ids=RC.MODE_NAME.get)
@pytest.mark.parametrize("cell", RC.CELLS)
def test_every_cell_every_mode_bit_exact(device, orc, cell, mode):
    sc, S = RC.scene("hf6"), RC.oracle_scene(orc, "hf6")
    eng = use_hf6(device)
    gp = eng.seeds_to_patches(sc.seeds[:RC.N_HF6])
    pat = RC.hf6_patches(orc)
    assert gp.tobytes() == pat.tobytes()
    op, oa = RC.oracle_refine(orc, "hf6", S, pat, cell, mode)
    ga = eng.refine(gp, cell, mode)
    assert np.array_equal(ga, oa)
    assert_same(gp, op)
    if cell >= 4 and mode in RC.OPTIMISING:
        assert gp["evals"].mean() > 5  # the optimiser really ran
    if mode == N.MODE_EVAL:
        assert (op["score"] > -1.0).sum() >= (100 if cell >= 4 else 1)


# ---------------------------------------------------------------------------
# 2. every cell through dp_evaluate_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.CELLS)
def test_every_cell_eval_batch_scores_equal_oracle(device, orc, cell):
    """dp_eval_batch against the oracle's objective at the stored pose, -1
    where no view scores; the records are not mutated."""
    sc, S = RC.scene("hf6"), RC.oracle_scene(orc, "hf6")
    eng = use_hf6(device)
    gp = eng.seeds_to_patches(sc.seeds[:240])
    gp["vis"][:3] = 0  # no visible view: score -1
    before = gp.tobytes()
    got = eng.evaluate(gp, cell)
    assert gp.tobytes() == before
    op = gp.copy()
    S.refine(op, cell, orc.MODE_EVAL)
    assert np.array_equal(got.view(np.uint32), op["score"].view(np.uint32))
    assert (got[:3] == -1.0).all() and (got[3:] > -1.0).any()


# ---------------------------------------------------------------------------
# 3. view-count edges per pass width
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell,m", [(c, m) for c in sorted(RC.VISIBLE_M) for m in RC.VISIBLE_M[c]])
def test_visible_counts_bit_exact(device, orc, cell, m):
    """m visible views, all mapping, in the cell's kernel: m = k G is k full
    passes, k G + 1 leaves one view over, 24 fills a map chunk, 25 and 27 open a
    second one (without texture 0); at G = 2 also every remainder of the wide
    pass's four and, at 2 and 3, no wide pass.  Every listed m qualifies 96
    seeds at every cell (27 included), so none is replaced."""
    b, pat = RC.visible_case(orc, cell, m)
    # the intended case: all m views score at the stored pose (oracle, CPU)
    chk = pat.copy()
    b.S.refine(chk, cell, orc.MODE_EVAL)
    assert len(pat) == RC.VISIBLE_N and (chk["score"] > -1.0).all()
    eng = device.use("base", b.P, b.imgs)
    for mode in RC.VISIBLE_MODES:
        op = compare(eng, pat, RC.oracle_refine(orc, ("base", m), b.S, pat, cell, mode), cell, mode)
    assert op["evals"].mean() > 5


# ---------------------------------------------------------------------------
# 4. 64-bit tap addressing outside n = 11 / 16
# ---------------------------------------------------------------------------
@pytest.fixture
def wide_engine(monkeypatch):
    """a fresh engine whose views are set under DP_WIDE_ADDRESSING=1 (a.narrow
    false: 64-bit tap addresses; the G = 2 kernel then takes no wide and no
    split pass)"""
    monkeypatch.setenv("DP_WIDE_ADDRESSING", "1")
    with dp.Engine(device=0) as eng:
        yield eng


@pytest.mark.parametrize("cell", sorted({c for c, _ in RC.WIDE_ADDR_HF6}))
def test_wide_addressing_hf6_bit_exact(wide_engine, orc, cell):
    sc, S = RC.scene("hf6"), RC.oracle_scene(orc, "hf6")
    pat = S.seeds_to_patches(sc.seeds[:RC.WIDE_ADDR_N])
    wide_engine.set_views(sc.views)
    for mode in [m for c, m in RC.WIDE_ADDR_HF6 if c == cell]:
        op = compare(wide_engine, pat, RC.oracle_refine(orc, "hf6-120", S, pat, cell, mode), cell, mode)
        assert op["evals"].mean() > 5


@pytest.mark.parametrize("cell,m", RC.WIDE_ADDR_BASE)
def test_wide_addressing_full_passes_bit_exact(wide_engine, orc, cell, m):
    """the non-narrow kernels on full passes: nine mapping views"""
    b, pat = RC.visible_case(orc, cell, m)
    wide_engine.set_views(RC.views_of(b.P, b.imgs))
    for mode in (N.MODE_NM, N.MODE_EXPAND):
        op = compare(wide_engine, pat, RC.oracle_refine(orc, ("base", m), b.S, pat, cell, mode), cell, mode)
    assert op["evals"].mean() > 5


# ---------------------------------------------------------------------------
# 5. one unsafe window in a pass, per G
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.UNSAFE_CELLS)
def test_unsafe_window_in_one_slot(device, orc, cell):
    """eight extra cameras, each almost inside one candidate's window plane and
    seven ordinary views beside it: one slot of a pass is unsafe, the pass takes
    group_sample_clamped<G>"""
    c = RC.unsafe_case(orc, cell)
    assert c.found["cameras"] == 8, f"only {c.found['cameras']} unsafe cameras map"
    eng = device.use(("unsafe", cell), c.P, c.imgs)
    for mode in RC.UNSAFE_MODES:
        compare(eng, c.pat, RC.oracle_refine(orc, "unsafe", c.S, c.pat, cell, mode), cell, mode)


# ---------------------------------------------------------------------------
# 6. two row pitches in one pass, per G
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.PITCH_CELLS)
def test_two_row_pitches_in_one_pass(device, orc, cell):
    """every third view 40 pixels wider: group_sample_safe<..., kUniPitch=false>;
    for G = 1, consecutive passes of either pitch"""
    c = RC.pitch_case(orc, cell)
    assert c.found["mixed"] >= RC.MIN_PATCHES, f"only {c.found['mixed']} candidates mix two pitches in the first pass"
    eng = device.use("pitch", c.P, c.imgs)
    for mode in RC.PITCH_MODES:
        op = compare(eng, c.pat, RC.oracle_refine(orc, "pitch", c.S, c.pat, cell, mode), cell, mode)
    assert op["evals"].mean() > 5


# ---------------------------------------------------------------------------
# 7. views beyond 64 at every G
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.BEYOND64_CELLS)
def test_more_than_64_views_bit_exact(device, orc, cell):
    """V = 70: visible lists reaching past one wavefront's 64 views"""
    sc, S = RC.scene("wide70"), RC.oracle_scene(orc, "wide70")
    eng = device.use("wide70", sc.P, sc.imgs)
    pat = RC.beyond64_patches(orc)
    assert eng.seeds_to_patches(sc.seeds[::7][:48]).tobytes() == pat.tobytes()
    assert pat["vis"][:, 1].any(), "no patch sees a view >= 64"
    for mode in RC.BEYOND64_MODES:
        compare(eng, pat, RC.oracle_refine(orc, "wide70", S, pat, cell, mode), cell, mode)


# ---------------------------------------------------------------------------
# 8. edge patches at every G
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.EDGE_CELLS)
def test_edge_patches(device, orc, cell):
    """no visible view, one visible view, a position off every image, and a
    window that ends in the last column of its reference image"""
    S = RC.oracle_scene(orc, "hf6")
    eng = use_hf6(device)
    p = RC.edge_patches(orc, cell)
    _, u, Wr = RC.border_patch(orc, cell)
    assert Wr - 1 <= u < Wr
    for mode in RC.ALL_MODES:
        op = compare(eng, p, RC.oracle_refine(orc, "edge", S, p, cell, mode), cell, mode)
        if mode == N.MODE_EVAL:
            assert (op["score"][:3] == -1.0).all() and op["score"][3] > -1.0
    assert len(eng.refine(dp.empty_patches(0), cell, N.MODE_EXPAND)) == 0


# ---------------------------------------------------------------------------
# 9. whole densify on the device-resident generation kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", RC.DENSIFY_OPTIONS, ids=RC.options_id)
def test_densify_bit_exact(orc, kw):
    """dp_densify equals the oracle's Scene.densify.  No configuration yields
    20 patches or fewer on the oracle, so none of the issue's cells is
    replaced."""
    sc = RC.scene("hf6")
    op, ost = RC.oracle_densify(orc, kw)
    with dp.Engine(dp.Options(**kw), device=0) as eng:
        eng.set_views(sc.views)
        gp, gst = eng.densify(sc.seeds)
    assert gst["patches"] == ost["patches"] and gst["seed_patches"] == ost["seed_patches"]
    assert gst["pops"] == ost["pops"]
    assert len(gp) > 20
    if "max_pops" in kw:
        assert gst["pops"] == kw["max_pops"]
    assert_same(gp, op, RC.DENSIFY_FIELDS)


def test_generation_api_equals_oracle_densify(orc):
    """expand_cell_size = 13 (G = 1) through the host-array generation API
    (dist.densify_partitioned at one rank) and the device-resident
    dp_densify_run in batches of 1 and 3 generations: each equals the oracle's
    densify, and so dp_densify's."""
    kw = RC.GENERATION_API_OPTIONS
    sc = RC.scene("hf6")
    op, ost = RC.oracle_densify(orc, kw)
    with dp.Engine(dp.Options(**kw), device=0) as eng:
        eng.set_views(sc.views)
        ref, rst = eng.densify(sc.seeds)
        got, gst = D.densify_partitioned(eng, sc.seeds, None)
        runs = []
        for k in (1, 3):
            g = eng.densify_begin(sc.seeds)
            cand, acc = eng.densify_refine_items(g, np.arange(g.items))
            g = eng.densify_commit(g, cand, acc)
            calls = 0
            while g.items > 0:
                g = eng.densify_run(g, k)
                calls += 1
            runs.append((k, calls, eng.densify_result()))
    assert len(ref) > 20 and rst["pops"] == kw["max_pops"]
    assert_same(ref, op, RC.DENSIFY_FIELDS)
    assert got.tobytes() == ref.tobytes()
    keys = ("patches", "seed_patches", "pops", "candidates", "generations", "evals")
    for key in keys:
        assert gst[key] == rst[key], key
    for key in ("patches", "seed_patches", "pops"):
        assert rst[key] == ost[key], key
    for k, calls, (rp, rs) in runs:
        assert rp.tobytes() == ref.tobytes(), f"batch {k}"
        for key in keys:
            assert rs[key] == rst[key], (k, key)
        assert calls >= rst["generations"] // k


# ---------------------------------------------------------------------------
# 10. repeatability at the new cells
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.REPEAT_CELLS)
def test_deterministic_repeat(device, orc, cell):
    sc = RC.scene("hf6")
    eng = use_hf6(device)
    a = eng.seeds_to_patches(sc.seeds[:200])
    b = a.copy()
    fa = eng.refine(a, cell, N.MODE_NM)
    fb = eng.refine(b, cell, N.MODE_NM)
    assert a.tobytes() == b.tobytes() and np.array_equal(fa, fb)
    assert a["evals"].mean() > 5
