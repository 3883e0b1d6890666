"""dp_densify_resume / dp_densify_iterate without a GPU: the header and the
bindings, the argument errors, PMVS.run's argument check, and the CPU reference
(tests/iterate_ref.py, a composition of the oracle) on the hf6 scene."""
import ctypes
import os
import re

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import synth

import iterate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dp_densify_resume", "dp_densify_resume_device", "dp_densify_iterate")


def test_header_declares_and_native_binds_the_new_calls():
    txt = open(os.path.join(ROOT, "include", "densepoints.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, txt), f"{sym} not declared"
        assert sym in bound and hasattr(N.lib, sym)
    assert len(bound["dp_densify_resume"]) == 5 and len(bound["dp_densify_resume_device"]) == 6
    assert len(bound["dp_densify_iterate"]) == 9
    # struct dp_iterate_stats: 6 x int64, 2 x int32, 3 x double
    m = re.search(r"typedef struct dp_iterate_stats \{(.*?)\} dp_iterate_stats;", txt, flags=re.S)
    assert m
    names = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert names == [name for name, _ in N.DpIterateStats._fields_]
    assert ctypes.sizeof(N.DpIterateStats) == 6 * 8 + 2 * 4 + 3 * 8 == 80
    # dp_filter_options is untouched
    assert ctypes.sizeof(N.DpFilterOptions) == 16


def test_argument_errors_without_device_are_loud():
    """No context can exist without a device: a null context and bad counts
    return DP_E_ARG, never a crash or a silent success.  On a GPU box the
    checks that need a context run too (no views: DP_E_STATE)."""
    g = N.DpGeneration()
    pat = np.zeros(2, dtype=N.PATCH_DTYPE)
    keep = np.ones(2, dtype=np.uint8)
    out, n = ctypes.c_void_p(), ctypes.c_int64()
    seeds = np.zeros((1, 3))
    lib = N.lib
    assert lib.dp_densify_resume(None, N.ptr(pat), 2, N.ptr(keep), ctypes.byref(g)) == N.DP_E_ARG
    assert lib.dp_densify_resume_device(None, None, 0, None, ctypes.byref(g), None) == N.DP_E_ARG
    for it in (0, 17, -1, 1):
        assert lib.dp_densify_iterate(None, N.ptr(seeds), 1, it, None, ctypes.byref(out), ctypes.byref(n), None,
                                      None) == N.DP_E_ARG
    h = ctypes.c_void_p()
    rc = lib.dp_ctx_create(None, 0, ctypes.byref(h))
    if rc != N.DP_OK:
        assert rc in (N.DP_E_NODEVICE, N.DP_E_HIP)
        return
    try:
        for it in (0, 17):
            assert lib.dp_densify_iterate(h, N.ptr(seeds), 1, it, None, ctypes.byref(out), ctypes.byref(n), None,
                                          None) == N.DP_E_ARG
        assert lib.dp_densify_iterate(h, N.ptr(seeds), 1, 2, None, ctypes.byref(out), ctypes.byref(n), None,
                                      None) == N.DP_E_STATE
        assert lib.dp_densify_resume(h, N.ptr(pat), -1, N.ptr(keep), ctypes.byref(g)) == N.DP_E_ARG
        assert lib.dp_densify_resume(h, None, 2, N.ptr(keep), ctypes.byref(g)) == N.DP_E_ARG
        assert lib.dp_densify_resume(h, N.ptr(pat), 2, N.ptr(keep), None) == N.DP_E_ARG
        assert lib.dp_densify_resume(h, N.ptr(pat), 2, N.ptr(keep), ctypes.byref(g)) == N.DP_E_STATE
        assert lib.dp_densify_resume_device(h, None, 2, None, ctypes.byref(g), None) == N.DP_E_ARG
        # keep flags without patches: still the patches' error, never a read of keep
        assert lib.dp_densify_resume(h, None, 2, None, ctypes.byref(g)) == N.DP_E_ARG
        k = ctypes.c_int64()
        assert lib.dp_probe_keep_gather(h, N.ptr(pat), 2, None, N.ptr(pat), ctypes.byref(k)) == N.DP_E_ARG
    finally:
        lib.dp_ctx_destroy(h)


def test_pmvs_run_iterations_need_the_filter():
    pm = dp.PMVS()
    with pytest.raises(ValueError):
        pm.run(np.zeros((1, 3)), filter_passes=0, iterations=2)
    with pytest.raises(ValueError):
        pm.run(np.zeros((1, 3)), filter_passes=3, iterations=0)
    with pytest.raises(ValueError):
        pm.run(np.zeros((1, 3)), filter_passes=3, iterations=17)


def test_partitioned_drivers_check_iterations():
    from densepoints_amd import dist

    with pytest.raises(ValueError):
        dist.densify_partitioned(None, np.zeros((1, 3)), None, iterations=2, filter_passes=0)
    with pytest.raises(ValueError):
        dist.densify_partitioned_device(None, np.zeros((1, 3)), None, None, iterations=2, filter_passes=0)


@pytest.fixture(scope="module")
def hf6():
    cfg = synth.config(6, 320, 240, 1)
    return synth.scene_host(cfg)


def test_reference_rounds_on_hf6(orc, hf6):
    P, imgs, seeds = hf6
    S = orc.Scene(P, imgs)
    surv, rounds, states = R.iterate(orc, S, seeds, 3)
    assert rounds[0]["offered"] == len(seeds)
    for k in (1, 2):
        # a round is offered the previous round's survivors
        assert rounds[k]["offered"] == rounds[k - 1]["patches"] - rounds[k - 1]["filtered_out"]
    for r, (store, keep) in zip(rounds, states):
        assert r["reinserted"] <= r["offered"] and len(store) >= r["reinserted"]
        assert np.array_equal(store["seq"], np.arange(len(store)))
        assert (store["flags"] & N.PATCH_ACCEPTED).all()
    assert rounds[0]["filtered_out"] > 0
    # the filter made room: round 2 expanded from the survivors
    assert (states[1][0]["parent"] != R.NO_PARENT).any()
    assert len(surv) == rounds[2]["patches"] - rounds[2]["filtered_out"]
    # iterations = 1 is densify then filter
    op, _ = S.densify(seeds)
    one, r1, _ = R.iterate(orc, S, seeds, 1)
    assert one.tobytes() == op[S.filter_patches(op, 3) != 0].tobytes()


def test_reference_resume_keeps_records(orc, hf6):
    """a stored record is the input record with seq, parent, flags and rgb rewritten"""
    P, imgs, seeds = hf6
    S = orc.Scene(P, imgs)
    op, _ = S.densify(seeds)
    eng = R.make_engine(orc, S)
    g = R.resume(orc, eng, op, None)
    st = eng.densify_result()[0]
    assert (g.index, g.head, g.per_item, g.cell, g.seq0, g.items) == (1, 0, 4, 11, len(op), len(st))
    assert 0 < len(st) <= len(op)
    assert (st["parent"] == R.NO_PARENT).all() and np.array_equal(st["seq"], np.arange(len(st)))
    # the store is a subsequence of the input in input order
    j = 0
    for p in st:
        while not (op[j]["pos"] == p["pos"]).all():
            j += 1
        for f in ("normal", "ref", "vis", "cand", "score", "evals"):
            assert np.array_equal(op[j][f], p[f])
        j += 1


def test_host_partitioned_driver_iterates_with_the_oracle_engine(orc, hf6):
    """dist.densify_partitioned(iterations=2) on the oracle's generation engine
    (one rank, no process group) equals the reference composition"""
    from densepoints_amd import dist

    P, imgs, seeds = hf6
    S = orc.Scene(P, imgs)
    want, rounds, _ = R.iterate(orc, S, seeds, 2)
    got, stats = dist.densify_partitioned(R.make_engine(orc, S), seeds, None, iterations=2, filter_passes=3)
    assert got.tobytes() == want.tobytes()
    assert stats["iterations"] == rounds
