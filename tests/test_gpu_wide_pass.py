"""The wide view pass of the n = 11 parity refine (four views of 16 lanes, two
gather batches) against the oracle, bit for bit, on inputs chosen for its
control flow: every remainder of the visible-view count modulo a full pass,
the pair map round, two map chunks, an invalid texture 0, an unsafe window in
one slot (the clamped fallback) and two row pitches in one pass.  Each input
is first checked on the CPU, with the oracle, to be the case it is meant to be."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

from refinecases import Base, _unsafe_camera  # built per cell there; here at the default, 11

pytestmark = pytest.mark.gpu

CELL = 11
FIELDS = ("pos", "normal", "ref", "vis", "cand", "score", "evals", "flags")
V, W, H = 30, 256, 192
NCAND = 160


def same(gp, op, fields=FIELDS):
    assert len(gp) == len(op)
    for f in fields:
        assert gp[f].tobytes() == op[f].tobytes(), f"field {f} differs"


@pytest.fixture(scope="module")
def base(orc):
    return Base(orc)


@pytest.fixture(scope="module")
def engine():
    with dp.Engine(device=0) as eng:
        yield eng


def views_of(P, imgs):
    return [dp.View(P[v], imgs[v]) for v in range(len(imgs))]


def run_both(engine, S, pat, modes):
    for mode in modes:
        gp, op = pat.copy(), pat.copy()
        ga = engine.refine(gp, CELL, mode)
        oa = S.refine(op, CELL, mode)
        assert np.array_equal(ga, oa), f"mode {mode}: accept flags differ"
        same(gp, op)
    return op


@pytest.mark.parametrize("m", [4, 5, 6, 7, 8, 9, 20, 27])
def test_visible_counts_bit_exact(engine, base, orc, m):
    """m = 4..9: one or two wide passes and every remainder (none, split,
    narrow, narrow + split); m = 20: the pair map round; m = 27: two map
    chunks (24 + 3), the second without texture 0."""
    pat = base.with_visible(m)
    # the intended case: all m views score at the stored pose (oracle, CPU)
    chk = pat.copy()
    base.S.refine(chk, CELL, orc.MODE_EVAL)
    assert (chk["score"] > -1.0).all()
    engine.set_views(views_of(base.P, base.imgs))
    op = run_both(engine, base.S, pat, (N.MODE_EVAL, N.MODE_NM, N.MODE_EXPAND))
    assert op["evals"].mean() > 5


def test_expand_children_bit_exact(engine, base, orc):
    """expand over refined parents (the bench step) on the same scene."""
    engine.set_views(views_of(base.P, base.imgs))
    parents = base.with_visible(9, n=48, spread=True)
    base.S.refine(parents, CELL, orc.MODE_NM)
    gk, ga = engine.expand(parents)
    ok, oa = base.S.expand(parents)
    assert np.array_equal(ga, oa)
    same(gk, ok, FIELDS + ("parent", "seq"))
    nvis = np.array([len(dp.visible_list(v)) for v in ok["vis"]])
    assert (nvis >= 4).any()


def test_texture0_invalid_no_view_scores(engine, base, orc):
    """An extra view 0 that sees nothing (its image coordinates are shifted
    off the image): texture 0's map fails, no view scores."""
    P0 = base.P[0].copy()
    P0[0] += 1.0e5 * P0[2]
    P = np.concatenate([P0[None], base.P])
    imgs = [base.imgs[0]] + list(base.imgs)
    S = orc.Scene(P, imgs)
    pat = base.with_visible(8, n=64)
    pat["vis"][:, 0] = (pat["vis"][:, 0] << np.uint64(1)) | np.uint64(1)
    pat["ref"] += 1
    chk = pat.copy()
    S.refine(chk, CELL, orc.MODE_EVAL)
    assert (chk["score"] == -1.0).all()
    engine.set_views(views_of(P, imgs))
    run_both(engine, S, pat, (N.MODE_EVAL, N.MODE_FILTER, N.MODE_NM, N.MODE_EXPAND))


def test_unsafe_window_in_one_slot(engine, base, orc):
    """Eight extra cameras, each almost inside one candidate's window plane:
    that candidate's visible set holds its camera next to seven ordinary
    views, so one slot of a wide pass is unsafe and the pass takes the
    clamped fallback."""
    pat = base.with_visible(7, n=64)
    extra, rows = [], []
    for k in range(len(pat)):
        if len(extra) == 8:
            break
        X = pat["pos"][k].astype(np.float64)
        n = pat["normal"][k].astype(np.float64)
        n /= np.linalg.norm(n)
        Pr = base.P[int(pat["ref"][k])]
        h = np.append(X, 1.0)
        depth = (Pr[2] @ h) / np.linalg.norm(Pr[2, :3])
        f = np.linalg.norm(np.cross(Pr[0, :3], Pr[2, :3])) / np.linalg.norm(Pr[2, :3]) ** 2
        s = CELL * depth / f  # world size of the window
        for angle in np.linspace(0.2, 6.0, 12):
            Pc = _unsafe_camera(X, n, s, angle)
            # the oracle finds a map for it (all corners inside its image)
            S1 = orc.Scene(np.concatenate([base.P, Pc[None]]), list(base.imgs) + [base.imgs[1]])
            q = pat[k:k + 1].copy()
            t0 = dp.visible_list(q["vis"][0])[0]
            q["vis"][0, 0] = np.uint64((1 << t0) | (1 << V))
            S1.refine(q, CELL, orc.MODE_EVAL)
            if q["score"][0] > -1.0:
                extra.append(Pc)
                rows.append(k)
                break
    assert len(extra) == 8, f"only {len(extra)} unsafe cameras map"
    P = np.concatenate([base.P, np.stack(extra)])
    imgs = list(base.imgs) + [base.imgs[1]] * 8
    S = orc.Scene(P, imgs)
    cases = pat[rows].copy()
    for i in range(8):
        cases["vis"][i, 0] |= np.uint64(1 << (V + i))
    engine.set_views(views_of(P, imgs))
    run_both(engine, S, cases, (N.MODE_EVAL, N.MODE_FILTER, N.MODE_NM, N.MODE_EXPAND))


def test_two_row_pitches_in_one_pass(engine, base, orc):
    """Every third view's image is 40 pixels wider (same camera, padded
    columns): passes mix two row pitches."""
    rng = np.random.default_rng(5)
    imgs = []
    for v, im in enumerate(base.imgs):
        if v % 3 == 1:
            pad = rng.integers(0, 256, (H, 40, 3), dtype=np.uint8)
            im = np.ascontiguousarray(np.concatenate([im, pad], axis=1))
        imgs.append(im)
    S = orc.Scene(base.P, imgs)
    pat = base.with_visible(9, spread=False)
    vl = [dp.visible_list(v) for v in pat["vis"]]
    mixed = sum(len({x % 3 == 1 for x in l[:4]}) == 2 for l in vl)
    assert mixed >= 32, f"only {mixed} candidates mix two pitches in the anchor pass"
    engine.set_views(views_of(base.P, imgs))
    run_both(engine, S, pat, (N.MODE_EVAL, N.MODE_NM, N.MODE_EXPAND))
