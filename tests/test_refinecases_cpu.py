"""The inputs of tests/refinecases.py on the CPU: on the oracle alone, that every
input of tests/test_gpu_refine_cells.py is the case it is meant to be, and that
the case tables cover every window size 2 .. 16 and, for every pass width G,
every kind of path.  A premise that fails here names the case it lacks, so a GPU
test cannot pass vacuously; and the cases can be read without a GPU."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

import refinecases as RC


def need(cond, case, what, got):
    assert cond, "%s lacks the case: %s (found %s)" % (case, what, got)


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
def test_pass_width_restates_the_kernel_table():
    want = {8: range(2, 6), 4: range(6, 9), 2: range(9, 12), 1: range(12, 17)}
    for g, cells in want.items():
        for cell in cells:
            assert RC.pass_width(cell) == g
            assert cell * cell <= (64 // g) * RC.TEX_PER_LANE and cell <= 64 // g
    with pytest.raises(ValueError):
        RC.pass_width(17)


def test_tables_cover_every_cell_and_every_path_per_pass_width():
    """items 1 and 2 run every cell; items 3-9 run, in every G's kernel, a full
    pass, a pass with one view left over (G > 1: with one view per pass none is
    ever part full), a full map chunk and the chunk boundary, 64-bit tap
    addressing -- also with full passes, for the two widths the issue names --
    an unsafe window, two row pitches, views past 63, the edge patches, the
    device-resident generation kernel and the repeat"""
    assert RC.CELLS == tuple(range(2, 17)) and len(RC.ALL_MODES) == 5
    assert set(RC.pass_width(c) for c in RC.CELLS) == {8, 4, 2, 1}
    cov = RC.coverage()
    kinds = ["full", "chunk-boundary", "wide-addressing", "unsafe", "mixed-pitch", "beyond-64", "edge", "generation"]
    for g in (8, 4, 2, 1):
        # G = 2 keeps test_gpu_wide_pass's counts, which cross the chunk at 27 and do not stop at 24
        for kind in kinds + (["remainder"] if g > 1 else []) + (["chunk-full"] if g != 2 else []):
            need(cov[g].get(kind), "G = %d" % g, kind, sorted(cov[g]))
        for cells in cov[g].values():
            assert all(RC.pass_width(c) == g for c in cells)
    for g in (4, 2):
        need(cov[g].get("wide-addressing-full"), "G = %d" % g, "64-bit addressing on full passes", sorted(cov[g]))
    # what the filling of the texel slots distinguishes, in item 3's cells
    item3 = set(RC.VISIBLE_M)
    assert {4, 8, 16} <= item3, "even cells and the two that fill their slots exactly"
    assert {9, 10} <= item3, "N = 81 and 100: pairs dead in both halves in the wide pass"
    assert {5, 13} <= item3, "odd cells: the last pair half dead"
    assert 2 in RC.EDGE_CELLS, "N = 4 < 8 lanes: lanes with no live texel"
    # G = 2: every remainder modulo the wide pass's four, and no wide pass at all
    for cell in (9, 10):
        assert {m % 4 for m in RC.VISIBLE_M[cell] if m >= 4} == {0, 1, 2, 3} and {2, 3} <= set(RC.VISIBLE_M[cell])
    # the seed stage's kernel off its default cell, in two further widths
    assert {RC.pass_width(kw["seed_cell_size"]) for kw in RC.DENSIFY_OPTIONS if "seed_cell_size" in kw} == {4, 1}
    assert RC.GENERATION_API_OPTIONS in RC.DENSIFY_OPTIONS and RC.pass_width(
        RC.GENERATION_API_OPTIONS["expand_cell_size"]) == 1
    assert {RC.pass_width(c) for c in RC.REPEAT_CELLS} == {8, 2, 1}


# ---------------------------------------------------------------------------
# items 1, 2, 4 (hf6), 7, 10: the optimiser runs, patches score
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.CELLS)
def test_hf6_premises(orc, cell):
    S, pat = RC.oracle_scene(orc, "hf6"), RC.hf6_patches(orc)
    assert len(pat) == RC.N_HF6
    for mode in RC.ALL_MODES:
        op, oa = RC.oracle_refine(orc, "hf6", S, pat, cell, mode)
        scored, evals = int((op["score"] > -1.0).sum()), float(op["evals"].mean())
        print("hf6 cell %d %s: %d score, evals mean %.1f, %d accepted" % (cell, RC.MODE_NAME[mode], scored, evals,
                                                                          int(oa.sum())))
        if cell >= 4 and mode in RC.OPTIMISING:
            need(evals > 5, "hf6 cell %d %s" % (cell, RC.MODE_NAME[mode]), "the optimiser really ran", evals)
        if cell >= 4 and mode == N.MODE_EVAL:
            need(scored >= 100, "hf6 cell %d" % cell, "100 of 160 patches scoring", scored)
        if cell < 4 and mode == N.MODE_EVAL:
            need(scored >= 1, "hf6 cell %d" % cell, "a patch that scores", scored)
    # item 2's input: 240 patches, the first three without a visible view
    q = S.seeds_to_patches(RC.scene("hf6").seeds[:240])
    q["vis"][:3] = 0
    S.refine(q, cell, orc.MODE_EVAL)
    need((q["score"][:3] == -1.0).all() and (q["score"][3:] > -1.0).any(), "hf6 cell %d" % cell,
         "evaluate: -1 without views, a score with", int((q["score"] > -1.0).sum()))


@pytest.mark.parametrize("cell", RC.BEYOND64_CELLS)
def test_beyond_64_views_premises(orc, cell):
    S, pat = RC.oracle_scene(orc, "wide70"), RC.beyond64_patches(orc)
    need(pat["vis"][:, 1].any(), "wide70", "a patch that sees a view >= 64", 0)
    long = sum(len(dp.visible_list(v)) > RC.MAP_CHUNK for v in pat["vis"])
    need(long >= 8, "wide70", "8 patches whose visible list spans two map chunks", long)
    op, _ = RC.oracle_refine(orc, "wide70", S, pat, cell, N.MODE_NM)
    need(op["evals"].mean() > 5, "wide70 cell %d" % cell, "the optimiser really ran", float(op["evals"].mean()))


# ---------------------------------------------------------------------------
# items 3 and 4 (Base): all m views score
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", sorted(RC.VISIBLE_M))
def test_visible_count_premises(orc, cell):
    """for every m of the cell: 96 patches whose m visible views all map at the
    stored pose -- by Base's pairwise search at this cell, and together (with
    every view mapping, EVAL's score is the mean of m - 1 scores, above -1)"""
    ms = set(RC.VISIBLE_M[cell]) | {m for c, m in RC.WIDE_ADDR_BASE if c == cell}
    for m in sorted(ms):
        b, pat = RC.visible_case(orc, cell, m)
        need(len(pat) == RC.VISIBLE_N, "Base cell %d" % cell, "96 seeds mapping in %d views" % m, len(pat))
        for p in pat:
            vl = dp.visible_list(p["vis"])
            assert len(vl) == m
        rows = b.qualifying(m)[:RC.VISIBLE_N]
        assert all(b.good[r, dp.visible_list(p["vis"])].all() for r, p in zip(rows, pat))
        chk = pat.copy()
        b.S.refine(chk, cell, orc.MODE_EVAL)
        need((chk["score"] > -1.0).all(), "Base cell %d m %d" % (cell, m), "every patch scores",
             int((chk["score"] > -1.0).sum()))
        op, _ = RC.oracle_refine(orc, ("base", m), b.S, pat, cell, N.MODE_NM)
        need(op["evals"].mean() > 5, "Base cell %d m %d" % (cell, m), "the optimiser really ran",
             float(op["evals"].mean()))


def test_base_at_cell_11_is_the_wide_pass_fixture(orc):
    """the default Base is the one test_gpu_wide_pass.py has always built"""
    b = RC.base(orc)
    assert b.cell == 11 and b.good.shape[1] == RC.V == 30
    assert len(b.with_visible(27)) == RC.NCAND and len(b.with_visible(9, n=48, spread=True)) == 48


# ---------------------------------------------------------------------------
# item 5: eight unsafe cameras map
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.UNSAFE_CELLS)
def test_unsafe_window_premises(orc, cell):
    c = RC.unsafe_case(orc, cell)
    need(c.found["cameras"] == 8 and len(c.pat) == 8, "unsafe cell %d" % cell, "eight unsafe cameras that map",
         c.found["cameras"])
    for i, p in enumerate(c.pat):
        vl = dp.visible_list(p["vis"])
        assert len(vl) == 8 and vl[-1] == RC.V + i and all(v < RC.V for v in vl[:-1])
        # the camera maps in the oracle, next to texture 0 alone
        q = c.pat[i:i + 1].copy()
        q["vis"][0] = dp.mask_from_list([vl[0], RC.V + i])
        c.S.refine(q, cell, orc.MODE_EVAL)
        need(q["score"][0] > -1.0, "unsafe cell %d" % cell, "camera %d maps" % i, float(q["score"][0]))
        # and its principal plane cuts the window: corners on both sides of it
        corners, _ = RC.window_corners(orc, c.P, p, cell)
        depth = np.array([c.P[RC.V + i][2] @ np.append(x, 1.0) for x in corners])
        need((depth > 0).any() and (depth < 0).any(), "unsafe cell %d" % cell,
             "camera %d's principal plane cuts the window" % i, depth)


# ---------------------------------------------------------------------------
# item 6: two row pitches in the first pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.PITCH_CELLS)
def test_mixed_pitch_premises(orc, cell):
    c = RC.pitch_case(orc, cell)
    widths = {im.shape[1] for im in c.imgs}
    assert widths == {RC.W, RC.W + RC.PITCH_PAD}
    need(c.found["mixed"] >= RC.MIN_PATCHES, "pitch cell %d" % cell,
         "32 candidates whose first pass mixes both pitches", c.found["mixed"])
    chk = c.pat.copy()
    c.S.refine(chk, cell, orc.MODE_EVAL)
    need((chk["score"] > -1.0).all(), "pitch cell %d" % cell, "every patch scores", int((chk["score"] > -1.0).sum()))


# ---------------------------------------------------------------------------
# item 8: the edge patches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", RC.EDGE_CELLS)
def test_edge_patch_premises(orc, cell):
    S = RC.oracle_scene(orc, "hf6")
    p = RC.edge_patches(orc, cell)
    assert len(p) == 4
    assert len(dp.visible_list(p["vis"][0])) == 0 and len(dp.visible_list(p["vis"][1])) == 1
    q, u, Wr = RC.border_patch(orc, cell)
    need(Wr - 1 <= u < Wr, "edge cell %d" % cell, "a window corner in the reference image's last column", u)
    assert int(q["ref"][0]) in dp.visible_list(q["vis"][0])
    chk = p.copy()
    S.refine(chk, cell, orc.MODE_EVAL)
    need((chk["score"][:3] == -1.0).all() and chk["score"][3] > -1.0, "edge cell %d" % cell,
         "three patches that cannot score and the border patch that does", chk["score"])
    # one more pixel and the reference view has no map for it
    _, _, _, _, xr = orc.view_geometry(RC.scene("hf6").P[int(q["ref"][0])])
    far = q.copy()
    corners, uv = RC.window_corners(orc, RC.scene("hf6").P, q[0], cell)
    step = np.linalg.norm(corners[1] - corners[0]) / (uv[1, 0] - uv[0, 0])  # world units per pixel of u
    far["pos"][0] = (q["pos"][0].astype(np.float64) + step * xr / np.linalg.norm(xr)).astype(np.float32)
    S.refine(far, cell, orc.MODE_EVAL)
    need(far["score"][0] == -1.0, "edge cell %d" % cell, "the window leaves the image one pixel further", far["score"])


# ---------------------------------------------------------------------------
# item 9: whole densify
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", RC.DENSIFY_OPTIONS, ids=RC.options_id)
def test_densify_premises(orc, kw):
    op, st = RC.oracle_densify(orc, kw)
    print("densify %s: %s" % (kw, st))
    need(len(op) > 20 and st["patches"] == len(op), "densify %s" % (kw,), "more than 20 patches", st)
    need(st["patches"] > st["seed_patches"], "densify %s" % (kw,), "patches made by the expansion", st)
    if "max_pops" in kw:
        need(st["pops"] == kw["max_pops"], "densify %s" % (kw,), "pops at the cap", st)
