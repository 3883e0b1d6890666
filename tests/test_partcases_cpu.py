"""The planted partition cases (tests/partcases.py) hit what they are named
for: on the oracle's GenerationEngine (densify_begin + densify_owners) and on a
restatement of the header's key formula in plain Python (ints, math.floor) the
seed patches' reference views and keys are the intended ones, the owners are
the stable sort cut at floor(r n / world), the statistics equal a direct
count, and every edge class is present in its case."""
import math

import numpy as np
import pytest

import partcases as PC

oracle_run = PC.oracle_run


# ---- the header's formula (include/densepoints.h, partition spec) -----------
def _div(a, b):
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def tile_coord(q, tmax):
    t = 0
    if q > -2.0e9 and q < 2.0e9:  # a NaN fails both
        t = math.floor(q)
    return min(max(t, -1), tmax)


def quotients(case, pos, ref):
    """(v / tile_px, u / tile_px) per item, as Python floats"""
    out = []
    for X, r in zip(pos, ref):
        x, y, z = (float(c) for c in X)
        P = [[float(c) for c in row] for row in case.P[int(r)]]
        h = [((p[0] * x + p[1] * y) + p[2] * z) + p[3] for p in P]
        out.append((_div(h[1], h[2]) / float(case.tile_px), _div(h[0], h[2]) / float(case.tile_px), h[2]))
    return out


def restated_keys(case, pos, ref):
    Wmax = max(W for W, _ in case.sizes)
    Hmax = max(H for _, H in case.sizes)
    TX, TY = -(-Wmax // case.tile_px), -(-Hmax // case.tile_px)
    keys, tiles = [], []
    for (qv, qu, _), r in zip(quotients(case, pos, ref), ref):
        ty, tx = tile_coord(qv, TY), tile_coord(qu, TX)
        tiles.append((int(r), ty, tx))
        keys.append((int(r) * (TY + 2) + ty + 1) * (TX + 2) + tx + 1)
    return keys, tiles


def partition(keys, world):
    """(owners, tiles, split_items) of the spec, counted directly"""
    n = len(keys)
    order = sorted(range(n), key=lambda i: keys[i])  # stable: ties by ascending index
    lo = PC.cuts(n, world)
    own = [0] * n
    for r in range(world):
        for j in range(lo[r], lo[r + 1]):
            own[order[j]] = r
    sk = [keys[i] for i in order]
    split_tiles = {sk[c] for c in lo[1:world] if 0 < c < n and sk[c - 1] == sk[c]}
    return own, len(set(keys)), sum(1 for k in keys if k in split_tiles)


@pytest.mark.parametrize("name", PC.NAMES)
def test_case_lands_where_intended(orc, name):
    case, sp, runs = oracle_run(orc, name)
    assert case.n == len(sp) > 0
    assert np.array_equal(sp["ref"], case.ref)
    assert np.array_equal(sp["pos"].astype(np.float64), case.seeds)
    keys, tiles = restated_keys(case, sp["pos"], sp["ref"])
    assert tiles == [(int(r), int(y), int(x)) for r, y, x in zip(case.ref, case.ty, case.tx)]
    assert keys == case.key
    assert max(keys) < case.key_range
    for world in PC.WORLDS:
        own, stats, okeys = runs[world]
        assert [int(k) for k in okeys] == keys, world
        want_own, want_tiles, want_split = partition(keys, world)
        assert own.tolist() == want_own, world
        assert stats == {"items": case.n, "world": world, "tiles": want_tiles, "split_items": want_split}, world
        lo = PC.cuts(case.n, world)
        assert np.bincount(own, minlength=world).tolist() == [lo[r + 1] - lo[r] for r in range(world)]


@pytest.mark.parametrize("name", sorted(PC.REQUIRED))
def test_edge_classes_present(orc, name):
    """every class a case is named for holds an item, and the item has the
    property the class names"""
    case, sp, _ = oracle_run(orc, name)
    for label in PC.REQUIRED[name]:
        assert case.classes.get(label), (name, label)
    q = quotients(case, sp["pos"], sp["ref"])
    T = float(case.tile_px)
    W, H = (np.array(s) for s in zip(*case.sizes))
    for label, idx in case.classes.items():
        for i in idx:
            qv, qu, depth = q[i]
            r = int(case.ref[i])
            where = (name, label, i)
            if label == "interior":
                assert qu != math.floor(qu) and qv != math.floor(qv) and depth > 0, where
            elif label in ("integer_u", "integer_v"):
                x = qu if label == "integer_u" else qv
                assert x == math.floor(x) and depth > 0, where
            elif label == "zero":
                assert qu == 0.0 and qv == 0.0 and case.tx[i] == 0 and case.ty[i] == 0, where
            elif label == "negative_integer":
                assert qu == -1.0 and qv == -1.0, where
            elif label in ("ulp_below_u", "ulp_below_v"):
                x = qu if label == "ulp_below_u" else qv
                t = case.tx[i] if label == "ulp_below_u" else case.ty[i]
                assert math.nextafter(x, math.inf) == t + 1 and x < t + 1, where
            elif label in ("u_first_below", "v_first_below"):
                x = qu if label[0] == "u" else qv
                assert -1.0 <= x < 0.0, where
            elif label in ("u_far_below", "v_far_below"):
                x = qu if label[0] == "u" else qv
                assert x < -1.0, where
            elif label == "corner_low":
                assert qu < -1.0 and qv < -1.0, where
            elif label == "u_last_partial":
                assert W[r] % case.tile_px and (W[r] // case.tile_px) * T <= qu * T < W[r], where
            elif label == "v_last_partial":
                assert H[r] % case.tile_px and (H[r] // case.tile_px) * T <= qv * T < H[r], where
            elif label == "u_past_image":
                assert W[r] <= qu * T < case.TX * T and case.tx[i] == case.TX - 1, where
            elif label == "v_past_image":
                assert H[r] <= qv * T < case.TY * T and case.ty[i] == case.TY - 1, where
            elif label == "u_at_TX":
                assert qu == case.TX and case.tx[i] == case.TX, where
            elif label == "v_at_TY":
                assert qv == case.TY and case.ty[i] == case.TY, where
            elif label == "u_above":
                assert qu > case.TX + 1 and case.tx[i] == case.TX, where
            elif label == "v_above":
                assert qv > case.TY + 1 and case.ty[i] == case.TY, where
            elif label == "largest_key":
                assert case.key[i] == case.key_range - 1 and r == case.V - 1, where
            elif label == "centre":
                assert depth == 0.0 and qu != qu and qv != qv, where
            elif label == "principal_plane":
                assert depth == 0.0 and (math.isinf(qu) or math.isinf(qv)), where
                assert (case.ty[i], case.tx[i]) == (0, 0), where
            elif label == "behind":
                assert depth < 0.0 and math.isfinite(qu) and math.isfinite(qv), where
                # the sign flips: the seed lies on the other side of the axis than its image
                assert (case.seeds[i][0] - case.cams[r].C[0]) * (qu * T - case.cams[r].cx) < 0.0, where
            elif label in ("at_+2e9", "at_-2e9", "beyond_+2e9", "beyond_-2e9", "inside_+2e9", "inside_-2e9"):
                kind, sign = label.split("_")
                big, other, t, tmax = ((qu, qv, case.tx[i], case.TX) if not 0.0 <= qu < case.TX
                                       else (qv, qu, case.ty[i], case.TY))
                assert math.isfinite(big) and 0.0 <= other < tmax and (big > 0) == (sign == "+2e9"), where
                if kind == "at":
                    assert abs(big) == 2.0e9 and t == 0, where
                elif kind == "beyond":
                    assert abs(big) > 2.0e9 and t == 0, where
                else:  # one f32 step of the seed inside the guard: the clamp tile, not tile 0
                    assert 2.0e9 - 129.0 < abs(big) < 2.0e9 and t == (tmax if big > 0 else -1) and t != 0, where
            elif label == "smallest_view":
                assert W[r] == W.min() and H[r] == H.min() and (W.max() > W[r] and H.max() > H[r]), where
            elif label == "past_own_tiles":
                own_tx, own_ty = -(-W[r] // case.tile_px), -(-H[r] // case.tile_px)
                assert case.tx[i] > own_tx or case.ty[i] > own_ty, where
            elif label == "tie":
                assert case.key.count(case.key[i]) > 1, where
            else:
                raise AssertionError("unknown class %r" % (label,))


def test_key_width_premises():
    a, b = PC.build("pow2_keys"), PC.build("pow2_keys_plus_column")
    assert a.key_range == 64 and a.key_range & (a.key_range - 1) == 0
    assert max(a.key) == 63 and sorted(a.key) == list(range(64)) and a.key != sorted(a.key)
    assert (b.TX, b.TY) == (a.TX + 1, a.TY) and b.key_range == 80 and max(b.key) == 79
    assert b.key_range & (b.key_range - 1) != 0
    nine = PC.build("nine_keys")
    assert nine.key_range == 9 and sorted(nine.key) == list(range(9)) and nine.key[0] == 8
    one, huge = PC.build("tile1"), PC.build("tile_huge")
    assert one.tile_px == 1 and (one.TX, one.TY) == one.sizes[0]
    assert all(huge.tile_px > max(s) for s in huge.sizes) and (huge.TX, huge.TY) == (1, 1)
    un = PC.build("unequal")
    assert (un.TX, un.TY) == (-(-max(w for w, _ in un.sizes) // 64), -(-max(h for _, h in un.sizes) // 64))
    assert len(set(un.sizes)) == len(un.sizes)


def test_ties_and_cuts_premises(orc):
    """runs of equal keys given out of key order; for the tested worlds some
    cuts fall strictly inside a run and some exactly on a run's edge; a case
    with split_items > 0, one with split_items == 0 at world > 1 although its
    runs are longer than one item, and one with empty shares"""
    case, _, runs = oracle_run(orc, "ties")
    keys = case.key
    assert keys != sorted(keys) and case.n == sum(PC.TIE_RUNS)
    sk = sorted(keys)
    edges = {0}
    for run in PC.TIE_RUNS:
        edges.add(max(edges) + run)
    assert edges == {0, case.n} | {j for j in range(1, case.n) if sk[j - 1] != sk[j]}
    inside, on_edge = set(), set()
    for world in PC.WORLDS:
        for c in PC.cuts(case.n, world)[1:world]:
            (on_edge if c in edges else inside).add((world, c))
    assert {w for w, _ in inside} >= {2, 7, 8, 63, 64} and {w for w, _ in on_edge} >= {3, 7}
    assert runs[2][1]["split_items"] == 42 and runs[8][1]["split_items"] > 0
    assert runs[3][1]["split_items"] == 0 and runs[3][1]["tiles"] == len(PC.TIE_RUNS)
    assert runs[1][1]["split_items"] == 0
    few = PC.build("few")
    assert few.n < 7
    for name in ("few", "n1", "n2", "n63"):
        c, _, r = oracle_run(orc, name)
        for world in (w for w in PC.WORLDS if w > c.n):
            lo = PC.cuts(c.n, world)
            assert len(set(lo)) < len(lo)  # cuts coincide
            assert np.count_nonzero(np.bincount(r[world][0], minlength=world) == 0) == world - c.n
    # three of few's five items share a tile: at world 64 every cut between them splits it
    assert oracle_run(orc, "few")[2][64][1]["split_items"] == 3


def test_sizes_and_worlds_are_the_listed_ones():
    assert PC.WORLDS == (1, 2, 3, 7, 8, 63, 64)
    assert [PC.build("n%d" % n).n for n in PC.SIZES] == [1, 2, 63, 64, 65, 255, 256, 257, 1000]
    for n in PC.SIZES[2:]:
        c = PC.build("n%d" % n)
        assert len(set(c.key)) > 8 and set(c.ref.tolist()) == {0, 1, 2}
        assert c.ty.min() == -1 and c.tx.min() == -1 and c.ty.max() == c.TY and c.tx.max() == c.TX
