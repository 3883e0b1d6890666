"""The multi-rank partition and the slot exchange at their edges
(dp_partition.hip: tile_keys_kernel, the key-bit count and the pair sort of
partition_impl, partition_stats_kernel; dp_bfs.hip: compact_slot_kernel,
scatter_slots_kernel).  The planted items of tests/partcases.py -- tile
boundaries, clamp tiles, 0/0, x/0, negative depth, +-2e9, a power-of-two key
range, views of unequal size, runs of equal keys under cuts inside and on
their edges, fewer items than ranks -- against the oracle's statement of the
partition spec, in the host form and in the device form; then the one-wait
slot protocol driven by hand for 3 and 64 simulated ranks on one device.
Everything is integer-exact: no tolerance anywhere."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import synth
from densepoints_amd._native import PATCH_DTYPE

import partcases as PC

pytestmark = pytest.mark.gpu

REC = PATCH_DTYPE.itemsize


@pytest.fixture(scope="module")
def eng():
    with dp.Engine(device=0) as e:
        yield e


def _load(eng, case):
    eng.set_views([dp.View(case.P[v], case.imgs[v]) for v in range(case.V)])


class _DeviceArray:
    """n int64 at a device address, for torch.as_tensor"""

    def __init__(self, addr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (addr, False), "version": 2}


def _read_i64(addr, n):
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceArray(addr, n), device="cuda:0").cpu().numpy().copy()


@pytest.mark.parametrize("name", PC.NAMES)
def test_owners_equal_oracle_on_planted_items(orc, eng, name):
    """dp_densify_owners and its statistics equal the oracle's for every world,
    the seed patches' reference views are the intended ones, and a repeated
    call on the same generation returns the same bytes"""
    case, sp, runs = PC.oracle_run(orc, name)
    _load(eng, case)
    assert np.array_equal(eng.seeds_to_patches(case.seeds)["ref"], case.ref)
    g = eng.densify_begin(case.seeds)
    assert (g.items, g.per_item, g.index) == (case.n, 1, 0)
    for world in PC.WORLDS:
        own, fb = eng.densify_owners(g, world, case.tile_px)
        st = eng.densify_partition_stats()
        oown, ost, _ = runs[world]
        assert fb is False
        assert np.array_equal(own, oown), (name, world, np.nonzero(own != oown)[0][:8])
        assert st == ost, (name, world)
        again, _ = eng.densify_owners(g, world, case.tile_px)
        assert again.tobytes() == own.tobytes() and eng.densify_partition_stats() == st, (name, world)


@pytest.mark.parametrize("name", PC.NAMES)
def test_device_partition_equals_host_form(orc, eng, name):
    """dp_densify_partition_async on a non-default stream and on the legacy
    default stream: the shares are the floor cuts, the order read back is the
    stable sort of the oracle's keys, and order + shares imply the owners of
    dp_densify_owners on the same generation"""
    case, sp, runs = PC.oracle_run(orc, name)
    _load(eng, case)
    g = eng.densify_begin(case.seeds)
    n = case.n
    side = torch.cuda.Stream()
    for world in PC.WORLDS:
        own, _ = eng.densify_owners(g, world, case.tile_px)
        want_order = np.argsort(runs[world][2], kind="stable")
        lo = PC.cuts(n, world)
        for stream in (side.cuda_stream, None):
            assert stream is None or stream != 0
            d_order, counts = eng.densify_partition_async(g, world, case.tile_px, stream)
            assert counts.tolist() == [lo[r + 1] - lo[r] for r in range(world)], (name, world)
            order = _read_i64(d_order, n)
            assert np.array_equal(order, want_order), (name, world, stream)
            implied = np.full(n, -1, dtype=np.int32)
            implied[order] = np.repeat(np.arange(world, dtype=np.int32), counts)
            assert np.array_equal(implied, own), (name, world, stream)


def _code(fn):
    with pytest.raises(N.DensePointsError) as e:
        fn()
    return e.value.code


def test_refusals_leave_the_next_call_correct(orc, eng):
    """world 0 and 65 and tile_px 0 are DP_E_ARG, a generation out of sequence
    DP_E_STATE, in both forms; the valid call after each refusal is correct"""
    case, sp, runs = PC.oracle_run(orc, "clamps")
    _load(eng, case)
    g = eng.densify_begin(case.seeds)
    late = N.DpGeneration(g.items, g.head, g.per_item, g.cell, g.seq0, g.index + 1)
    side = torch.cuda.Stream().cuda_stream
    bad = [(0, case.tile_px, g, N.DP_E_ARG), (65, case.tile_px, g, N.DP_E_ARG), (8, 0, g, N.DP_E_ARG),
           (-1, case.tile_px, g, N.DP_E_ARG), (8, -64, g, N.DP_E_ARG), (8, case.tile_px, late, N.DP_E_STATE)]
    for world, tile, gen, code in bad:
        for form in ("owners", "async"):
            if form == "owners":
                own = np.zeros(gen.items, dtype=np.int32)
                rc = N.lib.dp_densify_owners(eng._ctx, ctypes.byref(gen), world, tile, N.ptr(own), None)
            else:
                d_order = ctypes.c_void_p()
                counts = np.zeros(64, dtype=np.int64)
                rc = N.lib.dp_densify_partition_async(eng._ctx, ctypes.byref(gen), world, tile,
                                                      ctypes.c_void_p(side), ctypes.byref(d_order), N.ptr(counts))
            assert rc == code, (world, tile, form)
            for w in (8, 3):
                own, _ = eng.densify_owners(g, w, case.tile_px)
                assert np.array_equal(own, runs[w][0]) and eng.densify_partition_stats() == runs[w][1], (world, form)
            d_order, counts = eng.densify_partition_async(g, 8, case.tile_px, side)
            assert np.array_equal(_read_i64(d_order, case.n), np.argsort(runs[8][2], kind="stable"))
    # the Python binding raises the same codes
    assert _code(lambda: eng.densify_owners(g, 65, case.tile_px)) == N.DP_E_ARG
    assert _code(lambda: eng.densify_partition_async(late, 8, case.tile_px, side)) == N.DP_E_STATE


# ---- the slot exchange -------------------------------------------------------
# hf6 (the scene of tests/test_gpu_dist.py) with 32 spread seeds: 30 that the
# seed stage's filter rejects and two that it keeps.  Generation 0 then has 32
# items of which two pass, generation 1 has two items -- fewer than three ranks
# -- and the expansion stays at a handful of items per generation; the pop cap
# ends it after nine generations.
REJECTED = (6, 23, 33, 50, 56, 60, 91, 103, 119, 131, 135, 138, 141, 144, 156, 165, 177, 189, 215, 229, 236, 253, 262,
            269, 277, 280, 288, 296, 303, 318)
KEPT = (0, 84)
MAX_POPS = 40
SENTINEL = 0xA5

_exchange = {}


def exchange_scene(orc):
    """P, imgs, seeds and the oracle's generations: per generation (items,
    per_item, accept flags per candidate in item order, {world: (owners,
    statistics)}): computed once"""
    if not _exchange:
        P, imgs, seeds = synth.scene_host(synth.config(6, 320, 240, 1))
        seeds = np.ascontiguousarray(seeds[sorted(REJECTED + KEPT)])
        G = orc.GenerationEngine(orc.Scene(P, imgs, dp.Options(max_pops=MAX_POPS)), threads=8)
        g = G.densify_begin(seeds)
        gens = []
        while g.items > 0:
            parts = {}
            for world in (3, 64):
                own, _ = G.densify_owners(g, world)
                parts[world] = (own, G.densify_partition_stats())
            cand, acc = G.densify_refine_items(g, np.arange(g.items))
            gens.append((g.items, g.per_item, acc.copy(), parts))
            g = G.densify_commit(g, cand, acc)
        _exchange.update(P=P, imgs=imgs, seeds=seeds, gens=gens)
    return _exchange


@pytest.mark.parametrize("world", [3, 64])
def test_slot_exchange_by_hand(orc, world):
    """The one-wait protocol with `world` simulated ranks, one context each, on
    one device and one stream: every rank partitions, refines its share into
    its slot of the gathered buffer (stride exactly max_r counts[r] *
    per_item, the buffer pre-filled with a sentinel), then every rank commits
    the gathered buffer.  Each slot's header equals the accepted candidates
    of the rank's items by the oracle, its records carry exactly their
    generation positions, nothing is written past record `count`, `exchanged`
    is the sum of the headers, the statistics read back with the commit equal
    the oracle's, and at the end every rank's store is dp_densify's."""
    ex = exchange_scene(orc)
    views = [dp.View(ex["P"][v], ex["imgs"][v]) for v in range(len(ex["P"]))]
    opts = dp.Options(max_pops=MAX_POPS)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    seen = dict(fewer_items_than_ranks=False, no_items=False, nothing_accepted=False, full_slot=False)
    with contextlib.ExitStack() as stack, torch.cuda.stream(stream):
        engs = [stack.enter_context(dp.Engine(opts, device=0)) for _ in range(world)]
        for e in engs:
            e.set_views(views)
        ref, rst = engs[0].densify(ex["seeds"])
        gens = [e.densify_begin(ex["seeds"]) for e in engs]
        index = 0
        while gens[0].items > 0:
            n, per = gens[0].items, gens[0].per_item
            o_items, o_per, o_acc, o_parts = ex["gens"][index]
            o_own, o_stats = o_parts[world]
            assert (n, per) == (o_items, o_per), index
            lo = PC.cuts(n, world)
            orders = []
            for r, e in enumerate(engs):
                d_order, counts = e.densify_partition_async(gens[r], world, 64, sp)
                assert counts.tolist() == [lo[q + 1] - lo[q] for q in range(world)]
                orders.append(d_order)
            stride = int(counts.max()) * per
            assert stride == max(lo[q + 1] - lo[q] for q in range(world)) * per >= 1
            recv = torch.full((world, (stride + 1) * REC), SENTINEL, dtype=torch.uint8, device="cuda:0")
            for r, e in enumerate(engs):
                mine = int(counts[r])
                e.densify_refine_share_async(gens[r], orders[r] + 8 * lo[r] if mine else 0, mine,
                                             recv[r].data_ptr(), stride, sp)
            stream.synchronize()
            host = recv.cpu().numpy()
            headers = []
            acc_item = o_acc.reshape(n, per)
            for r in range(world):
                mine = int(counts[r])
                cnt = int(host[r, :8].view(np.int64)[0])
                headers.append(cnt)
                items_r = np.nonzero(o_own == r)[0]
                assert len(items_r) == mine
                want = sorted(int(i) * per + d for i in items_r for d in range(per) if acc_item[i, d])
                assert cnt == len(want) <= mine * per <= stride, (index, r)
                recs = host[r, REC:(1 + cnt) * REC].view(PATCH_DTYPE)
                assert sorted(recs["seq"].tolist()) == want, (index, r)
                # the rest of the header record and everything past record `cnt` is untouched
                assert np.all(host[r, 8:REC] == SENTINEL), (index, r)
                assert np.all(host[r, (1 + cnt) * REC:] == SENTINEL), (index, r)
                seen["no_items"] |= mine == 0
                seen["nothing_accepted"] |= mine > 0 and cnt == 0
                seen["full_slot"] |= cnt == stride
            seen["fewer_items_than_ranks"] |= n < world
            for r, e in enumerate(engs):
                exchanged = e.densify_commit_gathered_device(gens[r], recv.data_ptr(), stride, world, sp)
                assert exchanged == sum(headers), (index, r)
                assert e.densify_partition_stats() == o_stats, (index, r)
                assert (gens[r].items, gens[r].head, gens[r].index) == (gens[0].items, gens[0].head, index + 1)
            index += 1
        assert index == len(ex["gens"]) > 3
        for r, e in enumerate(engs):
            got, st = e.densify_result()
            assert got.tobytes() == ref.tobytes(), r
            assert st["patches"] == rst["patches"] == len(ref) > 10
    assert all(seen.values()), seen
