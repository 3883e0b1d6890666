"""Every device form of tests/streamcases.py on a caller's stream behind pending
work.  The form's input buffers hold a valid poison; on the side stream a
bounded delay (torch.cuda._sleep, its cycle count from a measured rate) is
queued, then the copies of the real input into those buffers, then the form,
then the read-backs.  A step of the form that ran on any other stream ran
before the copies, read the poison and shows as a wrong answer (the poison is
valid input: never as a bad address).  The forms documented as queuing without
a host wait must return while the delay is still running.  The expected result
is the CPU reference's where the table has one, else the form's own run on the
default stream after a full synchronize; both are compared, so that a failure
separates "stream" from "kernel".

Measured on an MI355X: the delay t0 -> t1 is 118 to 127 ms in every case (the
cap is 500); the longest host time of one call of a no-wait form is 0.24 ms
(mesh_colour_device, back to back), most are below 0.12 ms, so a call returns
about 500 times sooner than the delay ends.  A form with its one wait returns
when the delay has run out (119 to 120 ms).  Each run prints both figures per
case on a line starting with STREAMCASE."""
import time

import numpy as np
import pytest
import torch

import densepoints_amd as dp

import cloudknn_ref as KR
import streamcases as SC

pytestmark = pytest.mark.gpu

SENT = 0xAA
PAD = 64
DELAY_MS = 120.0  # the cap per case is 500
NO_WAIT = [n for n, c in SC.CASES.items() if c.no_wait]
# mesh_decimate_device returns its counts, so it waits once, but its scratch is as shared as the others'
BACK_TO_BACK = NO_WAIT + ["mesh_decimate_device"]

_inputs, _rate = {}, {}


def sleep_cycles():
    """the cycle count of a DELAY_MS sleep, from the rate of one measured sleep"""
    if not _rate:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(2_000_000)
        b.record()
        torch.cuda.synchronize()
        _rate["per_ms"] = 2_000_000 / max(a.elapsed_time(b), 1e-3)
    return int(min(DELAY_MS * _rate["per_ms"], 2 ** 40))


def inputs(case, kind, eng):
    key = (case.name, kind)
    if key not in _inputs:
        _inputs[key] = case.make(kind, eng) if case.gpu_inputs else case.make(kind)
        for a in _inputs[key].values():  # the validity test_streamcases_cpu.py cannot check without the engine
            assert a.dtype.kind != "f" or np.isfinite(a).all(), key
    return _inputs[key]


def engine_for(case):
    eng = dp.Engine(device=0)
    if case.views:
        eng.set_views(SC.scene()["views"])
    if case.setup:
        case.setup(eng)
    return eng


def upload(I):
    return {k: torch.from_numpy(SC.as_bytes(v).copy()).cuda() for k, v in I.items()}


def fresh_outputs(case):
    return {k: torch.full((n + PAD,), SENT, dtype=torch.uint8, device="cuda") for k, n in case.outs.items()}


class _DeviceBytes:
    def __init__(self, addr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (addr, False), "version": 2}


def read_back(case, eng, din, dout):
    """copies of every output, queued on the current stream"""
    out = {k: t.clone() for k, t in dout.items()}
    out.update({k: din[k].clone() for k in case.inout})
    if case.store:
        addr, n = eng.densify_store_device()
        out["store"] = torch.as_tensor(_DeviceBytes(addr, n * SC.PATCH.itemsize), device="cuda:0").clone()
    return out


def call(case, eng, din, dout, stream, stats):
    p = {k: t.data_ptr() for k, t in list(din.items()) + list(dout.items())}
    return case.call(eng, p, stream, stats)


def to_host(out):
    return {k: t.cpu().numpy() for k, t in out.items()}


def default_run(case, eng, I):
    """the form on the default stream between two full synchronizes"""
    din, dout = upload(I), fresh_outputs(case)
    torch.cuda.synchronize()
    ret = call(case, eng, din, dout, None, True)
    torch.cuda.synchronize()
    out = read_back(case, eng, din, dout)
    torch.cuda.synchronize()
    return to_host(out), ret


def assert_equals_reference(case, out, ret, I, what):
    """against the CPU reference: the leading bytes, the sentinel behind them"""
    want, counters, host = case.ref(I)
    for k, a in want.items():
        exp = SC.as_bytes(a)
        assert out[k][:exp.size].tobytes() == exp.tobytes(), (what, case.name, k)
        assert (out[k][exp.size:] == SENT).all(), (what, case.name, k, "written past the results")
    if ret is not None:
        assert case.host(ret) == host, (what, case.name)
        if counters is not None:
            assert case.counters(ret) == counters, (what, case.name)


def assert_equals_run(case, out, want, what):
    assert sorted(out) == sorted(want)
    for k in want:
        assert out[k].tobytes() == want[k].tobytes(), (what, case.name, k)
    for k in case.outs:
        assert (out[k][case.outs[k]:] == SENT).all(), (what, case.name, k, "written past the buffer")


class Queued:
    """one delay on a side stream, then calls queued behind it"""

    def __init__(self):
        self.side = torch.cuda.Stream()
        assert self.side.cuda_stream != 0
        self.t0, self.t1, self.t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        self.host_s = 0.0
        cycles = sleep_cycles()
        with torch.cuda.stream(self.side):
            self.t0.record()
            torch.cuda._sleep(cycles)
            self.t1.record()

    def run(self, case, eng, real_dev, din, dout, stats):
        """real input over the poison, the form, the read-backs: all queued"""
        with torch.cuda.stream(self.side):
            for k, t in din.items():
                t.copy_(real_dev[k], non_blocking=True)
            h0 = time.perf_counter()
            ret = call(case, eng, din, dout, self.side.cuda_stream, stats)
            self.host_s = max(self.host_s, time.perf_counter() - h0)
            pending = not self.t1.query()
            out = read_back(case, eng, din, dout)
        return out, ret, pending

    def finish(self, name):
        with torch.cuda.stream(self.side):
            self.t2.record()
        self.side.synchronize()
        delay = self.t0.elapsed_time(self.t1)
        assert 0 < delay <= 500.0
        print("STREAMCASE %s delay_ms %.1f longest_host_call_ms %.3f" % (name, delay, 1e3 * self.host_s))


def side_run(case, eng, stats):
    real, poison = inputs(case, "real", eng), inputs(case, "poison", eng)
    real_dev, din, dout = upload(real), upload(poison), fresh_outputs(case)
    torch.cuda.synchronize()
    q = Queued()
    out, ret, pending = q.run(case, eng, real_dev, din, dout, stats)
    q.finish(case.name)
    return to_host(out), ret, pending


@pytest.mark.parametrize("name", list(SC.CASES))
def test_form_on_a_callers_stream_behind_pending_work(name):
    case = SC.CASES[name]
    with engine_for(case) as eng:
        real, poison = inputs(case, "real", eng), inputs(case, "poison", eng)
        # the warm-up on the real sizes (no scratch buffer grows later) is the default-stream run
        want, want_ret = default_run(case, eng, real)
        if case.ref is not None:
            assert_equals_reference(case, want, want_ret, real, "default stream")
        else:
            other, other_ret = default_run(case, eng, poison)
            assert any(other[k].tobytes() != want[k].tobytes() for k in want) or \
                case.host(other_ret) != case.host(want_ret), "the poison gives the same answer"
            want, want_ret = default_run(case, eng, real)
        out, ret, pending = side_run(case, eng, False)
        if case.no_wait:
            assert pending, "the call waited: it returned after the delay had run out"
        if case.ref is not None:
            assert_equals_reference(case, out, None, real, "caller's stream")
        assert_equals_run(case, out, want, "caller's stream")
        if ret is not None:  # what a form returns to the host, it returns with stats=False too
            assert case.host(ret) == case.host(want_ret)
            if not case.has_stats:
                assert case.counters(ret) == case.counters(want_ret)
        if case.has_stats:
            out, ret, _ = side_run(case, eng, True)
            if case.ref is not None:
                assert_equals_reference(case, out, ret, real, "caller's stream, stats")
            assert_equals_run(case, out, want, "caller's stream, stats")
            assert case.host(ret) == case.host(want_ret) and case.counters(ret) == case.counters(want_ret)
            st = ret[2] if isinstance(ret, tuple) else ret
            for k, v in st.items():
                if k.endswith("_ms"):
                    assert np.isfinite(v) and v >= 0, k


@pytest.mark.parametrize("name", BACK_TO_BACK)
def test_back_to_back_without_a_wait(name):
    """call A (real) and call B (other) of one form queued behind one delay: a
    host staging area or a scratch table that B overwrites before A has consumed
    it shows in A's outputs"""
    case = SC.CASES[name]
    with engine_for(case) as eng:
        X, Y, poison = (inputs(case, kind, eng) for kind in ("real", "other", "poison"))
        wants = [default_run(case, eng, I)[0] for I in (X, Y)]
        assert any(wants[0][k].tobytes() != wants[1][k].tobytes() for k in wants[0])
        devs = [upload(I) for I in (X, Y)]
        bufs = [(upload(poison), fresh_outputs(case)) for _ in range(2)]
        torch.cuda.synchronize()
        q = Queued()
        outs = [q.run(case, eng, dev, din, dout, False) for dev, (din, dout) in zip(devs, bufs)]
        assert outs[1][2] or not case.no_wait, "a call waited"
        q.finish(name + " x2")
        for (out, _, _), want, I, what in zip(outs, wants, (X, Y), ("call A", "call B")):
            out = to_host(out)
            if case.ref is not None:
                assert_equals_reference(case, out, None, I, what)
            assert_equals_run(case, out, want, what)


def run_family(eng, names, kinds, expect_pending):
    cases = [SC.CASES[n] for n in names]
    ins = [inputs(c, kind, eng) for c, kind in zip(cases, kinds)]
    for c, I in zip(cases, ins):  # warm-up
        default_run(c, eng, I)
    devs = [upload(I) for I in ins]
    bufs = [(upload(inputs(c, "poison", eng)), fresh_outputs(c)) for c in cases]
    torch.cuda.synchronize()
    q = Queued()
    outs = [q.run(c, eng, dev, din, dout, False) for c, dev, (din, dout) in zip(cases, devs, bufs)]
    if expect_pending:
        assert outs[-1][2], "a call waited"
    q.finish("+".join(names))
    for c, I, (out, _, _) in zip(cases, ins, outs):
        assert_equals_reference(c, to_host(out), None, I, "shared scratch")


def test_shared_scratch_across_families_without_a_wait():
    """the cloud forms share the nearest-point scratch and the scan's temporary
    storage, the mesh forms the adjacency's: four calls queued behind one delay"""
    with dp.Engine(device=0) as eng:
        run_family(eng, ["cloud_knn_device", "cloud_clean_device", "cloud_nearest_device", "cloud_normals_device"],
                   ["real", "other", "real", "other"], True)
        # mesh_adjacency_device waits once by its contract: no assertion on the delay here
        run_family(eng, ["mesh_adjacency_device", "mesh_smooth_device", "mesh_normals_device", "mesh_decimate_device"],
                   ["real", "other", "real", "other"], False)


def test_scratch_that_grows_between_queued_calls():
    """cloud_knn_device, then cloud_clean_device on a cloud four times larger,
    which the context has not seen: its scratch grows between the two queued
    calls (a growth may drain the device: no assertion on the delay)"""
    knn = SC.CASES["cloud_knn_device"]
    n = 4 * SC.NPTS
    big, big_poison = SC.cloud(77, n), SC.cloud(78, n)
    want = KR.clean(big, SC.K, 0.3)
    assert KR.clean(big_poison, SC.K, 0.3)["keep"].tobytes() != want["keep"].tobytes()
    with dp.Engine(device=0) as eng:
        A = inputs(knn, "real", eng)
        default_run(knn, eng, A)
        devA, dinA, doutA = upload(A), upload(inputs(knn, "poison", eng)), fresh_outputs(knn)
        d_big, d_in = upload(dict(p=big))["p"], upload(dict(p=big_poison))["p"]
        sizes = dict(keep=n, mean_dist=4 * n, map=4 * n, out=12 * n, n_out=8)
        o = {k: torch.full((b + PAD,), SENT, dtype=torch.uint8, device="cuda") for k, b in sizes.items()}
        torch.cuda.synchronize()
        q = Queued()
        outA, _, _ = q.run(knn, eng, devA, dinA, doutA, False)
        with torch.cuda.stream(q.side):
            d_in.copy_(d_big, non_blocking=True)
            eng.cloud_clean_device(d_in.data_ptr(), n, 12, SC.K, 0.3, o["keep"].data_ptr(), o["mean_dist"].data_ptr(),
                                   o["map"].data_ptr(), o["out"].data_ptr(), o["n_out"].data_ptr(),
                                   stream=q.side.cuda_stream, stats=False)
            got = {k: t.clone() for k, t in o.items()}
        q.finish("knn+clean x4")
        assert_equals_reference(knn, to_host(outA), None, A, "before the growth")
        got = to_host(got)
        exp = dict(keep=want["keep"], mean_dist=want["mean_dist"], map=want["map"], out=want["points"],
                   n_out=np.int64([len(want["points"])]))
        for k, a in exp.items():
            e = SC.as_bytes(a)
            assert got[k][:e.size].tobytes() == e.tobytes(), k
            assert (got[k][e.size:] == SENT).all(), k


# ---- the multi-rank generation protocol ------------------------------------------------

WORLD = 3


def protocol(orc, delayed):
    """Every generation of the slot-exchange scene with WORLD ranks, one context
    each: partition, the share's items copied into the caller's item buffer
    (which holds other valid items until then), refine into the rank's slot,
    commit.  delayed: everything on a side stream, each generation behind a
    delay, the two _async forms asserted to return while it runs; else on the
    default stream with a full synchronize around every call.  Returns per
    generation (orders, counts, slots, exchanged, generation fields), and the
    stores."""
    import contextlib

    import partcases as PC
    from test_gpu_partition_edges import MAX_POPS, REC, exchange_scene

    ex = exchange_scene(orc)
    views = [dp.View(ex["P"][v], ex["imgs"][v]) for v in range(len(ex["P"]))]
    record = []
    with contextlib.ExitStack() as stack:
        engs = [stack.enter_context(dp.Engine(dp.Options(max_pops=MAX_POPS), device=0)) for _ in range(WORLD)]
        for e in engs:
            e.set_views(views)
        gens = [e.densify_begin(ex["seeds"]) for e in engs]
        while gens[0].items > 0:
            n, per = gens[0].items, gens[0].per_item
            lo = PC.cuts(n, WORLD)
            share = [lo[r + 1] - lo[r] for r in range(WORLD)]
            stride = max(share) * per
            # poison: the items of the other end of the generation, all inside 0 .. n - 1
            items = [torch.from_numpy(((n - 1) - np.arange(max(m, 1), dtype=np.int64)) % n).cuda() for m in share]
            recv = torch.full((WORLD, (stride + 1) * REC), SENT, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            q = Queued() if delayed else None
            sp = q.side.cuda_stream if delayed else None

            def settle(what):
                if delayed:
                    assert not q.t1.query(), what + " waited: it returned after the delay had run out"
                else:
                    torch.cuda.synchronize()

            orders = []
            with torch.cuda.stream(q.side) if delayed else contextlib.nullcontext():
                for r, e in enumerate(engs):
                    h0 = time.perf_counter()
                    d_order, counts = e.densify_partition_async(gens[r], WORLD, 64, sp)
                    if delayed:
                        q.host_s = max(q.host_s, time.perf_counter() - h0)
                    settle("densify_partition_async")
                    assert counts.tolist() == share
                    order = torch.as_tensor(_DeviceBytes(d_order, 8 * n), device="cuda:0")
                    if not delayed:
                        torch.cuda.synchronize()
                    orders.append(order.clone())
                    if share[r]:
                        items[r].view(torch.uint8).copy_(order[8 * lo[r]:8 * lo[r + 1]], non_blocking=True)
                    settle("the copy of the share")
                for r, e in enumerate(engs):
                    h0 = time.perf_counter()
                    e.densify_refine_share_async(gens[r], items[r].data_ptr() if share[r] else 0, share[r],
                                                 recv[r].data_ptr(), stride, sp)
                    if delayed:
                        q.host_s = max(q.host_s, time.perf_counter() - h0)
                    settle("densify_refine_share_async")
                slots = recv.clone()
                exchanged = []
                for r, e in enumerate(engs):
                    exchanged.append(e.densify_commit_gathered_device(gens[r], recv.data_ptr(), stride, WORLD, sp))
            if delayed:
                q.finish("generation_protocol gen %d" % len(record))
            torch.cuda.synchronize()
            record.append(dict(orders=[o.cpu().numpy().view(np.int64) for o in orders], share=share,
                               slots=slots.cpu().numpy(), exchanged=exchanged, stride=stride,
                               gens=[(g.items, g.head, g.per_item, g.cell, g.index) for g in gens],
                               stats=[e.densify_partition_stats() for e in engs]))
        stores = [e.densify_result()[0].tobytes() for e in engs]
        single = engs[0].densify(ex["seeds"])[0].tobytes()
    return record, stores, single


def slot_records(rec, r):
    """(count, the records of rank r's slot in generation order, the bytes behind them)"""
    from test_gpu_partition_edges import REC

    row = rec["slots"][r]
    cnt = int(row[:8].view(np.int64)[0])
    assert 0 <= cnt <= rec["stride"]
    recs = row[REC:(1 + cnt) * REC].view(SC.PATCH)
    return cnt, recs[np.argsort(recs["seq"], kind="stable")].tobytes(), row[(1 + cnt) * REC:]


def test_generation_protocol_on_a_callers_stream(orc):
    """densify_partition_async, densify_refine_share_async and
    densify_commit_gathered_device chained behind a delay on a side stream equal
    the same chain on the default stream with a synchronize around every call,
    the oracle's owners and accepted candidates, and dp_densify's store"""
    from test_gpu_partition_edges import exchange_scene

    ex = exchange_scene(orc)
    want, want_stores, single = protocol(orc, False)
    got, got_stores, _ = protocol(orc, True)
    assert len(got) == len(want) == len(ex["gens"]) > 3
    for index, (g, w) in enumerate(zip(got, want)):
        o_items, o_per, o_acc, o_parts = ex["gens"][index]
        o_own, o_stats = o_parts[WORLD]
        assert g["share"] == w["share"] and g["gens"] == w["gens"] and g["exchanged"] == w["exchanged"], index
        assert g["stats"] == w["stats"] == [o_stats] * WORLD, index
        acc_item = o_acc.reshape(o_items, o_per)
        headers = 0
        for r in range(WORLD):
            assert np.array_equal(g["orders"][r], w["orders"][r]), (index, r)
            implied = np.full(o_items, -1, dtype=np.int32)
            implied[g["orders"][r]] = np.repeat(np.arange(WORLD, dtype=np.int32), g["share"])
            assert np.array_equal(implied, o_own), (index, r)
            cnt, recs, rest = slot_records(g, r)
            wcnt, wrecs, _ = slot_records(w, r)
            assert cnt == wcnt and recs == wrecs, (index, r)
            assert (rest == SENT).all(), (index, r)
            seqs = sorted(int(i) * o_per + d for i in np.nonzero(o_own == r)[0] for d in range(o_per) if acc_item[i, d])
            assert np.frombuffer(recs, SC.PATCH)["seq"].tolist() == seqs, (index, r)
            headers += cnt
        assert g["exchanged"] == [headers] * WORLD, index
    assert got_stores == want_stores == [single] * WORLD
