"""Return codes of the batch entry points (dp_refine_batch, dp_expand_batch,
dp_fast_expand_batch, their _device forms, dp_seeds_to_patches) for invalid
input, on a context without views and on one with the hf6 views.

The expected codes are the documented order of each entry point's checks.  The
two expand families differ on purpose: dp_expand_batch looks at the views
first (n = 0 without views is DP_E_STATE), dp_fast_expand_batch only once it
has work (DP_OK).  A record naming a view outside the scene is a host-side
DP_E_ARG in dp_refine_batch only; every other form launches, and the kernel
rejects the record.  dp_refine_batch_device has no null check, so null arrays
are offered to it only where it returns before looking at them."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

from test_gpu_parity import scene

pytestmark = pytest.mark.gpu

OK, ARG, STATE = N.DP_OK, N.DP_E_ARG, N.DP_E_STATE
NP = 4  # parents / patches / seed points per call


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def test_batch_entry_points_return_codes():
    import torch

    L, ptr = N.lib, N.ptr
    sc = scene("hf6")
    V = len(sc.views)
    xyz = np.ascontiguousarray(sc.seeds[:NP], dtype=np.float64)
    with dp.Engine(device=0) as bare, dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        good = eng.seeds_to_patches(xyz)
        eng.refine(good, 16, N.MODE_SEED)
        bad = good.copy()
        bad["ref"][1] = V
        kids = dp.empty_patches(4 * NP)
        acc = np.zeros(4 * NP, dtype=np.uint8)
        out = dp.empty_patches(NP)
        d_good, d_bad = _dev(good), _dev(bad)
        d_kids = torch.zeros(4 * NP * N.PATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_acc = torch.zeros(4 * NP, dtype=torch.uint8, device="cuda")
        dg, db, dk, da = (t.data_ptr() for t in (d_good, d_bad, d_kids, d_acc))
        torch.cuda.synchronize()
        ev, cell = N.MODE_EVAL, 11

        # (label, call(ctx), code without views, code with views; None: not offered)
        cases = [
            ("refine n=0", lambda c: L.dp_refine_batch(c, ptr(good), 0, cell, ev, ptr(acc)), STATE, OK),
            ("refine n<0", lambda c: L.dp_refine_batch(c, ptr(good), -1, cell, ev, ptr(acc)), STATE, ARG),
            ("refine null", lambda c: L.dp_refine_batch(c, None, NP, cell, ev, ptr(acc)), STATE, ARG),
            ("refine cell=1", lambda c: L.dp_refine_batch(c, ptr(good), NP, 1, ev, ptr(acc)), STATE, ARG),
            ("refine ref>=V", lambda c: L.dp_refine_batch(c, ptr(bad), NP, cell, ev, ptr(acc)), STATE, ARG),
            ("refine_device n=0", lambda c: L.dp_refine_batch_device(c, dg, 0, cell, ev, da, None), STATE, OK),
            ("refine_device n<0", lambda c: L.dp_refine_batch_device(c, dg, -1, cell, ev, da, None), STATE, ARG),
            ("refine_device null", lambda c: L.dp_refine_batch_device(c, None, NP, cell, ev, None, None), STATE, None),
            ("refine_device cell=1", lambda c: L.dp_refine_batch_device(c, dg, NP, 1, ev, da, None), STATE, ARG),
            ("refine_device ref>=V", lambda c: L.dp_refine_batch_device(c, db, NP, cell, ev, da, None), STATE, OK),
            ("expand n=0", lambda c: L.dp_expand_batch(c, ptr(good), 0, ptr(kids), ptr(acc)), STATE, OK),
            ("expand n<0", lambda c: L.dp_expand_batch(c, ptr(good), -1, ptr(kids), ptr(acc)), STATE, ARG),
            ("expand null parents", lambda c: L.dp_expand_batch(c, None, NP, ptr(kids), ptr(acc)), STATE, ARG),
            ("expand null children", lambda c: L.dp_expand_batch(c, ptr(good), NP, None, ptr(acc)), STATE, ARG),
            ("expand ref>=V", lambda c: L.dp_expand_batch(c, ptr(bad), NP, ptr(kids), ptr(acc)), STATE, OK),
            ("expand_device n=0", lambda c: L.dp_expand_batch_device(c, dg, 0, dk, da, None), STATE, OK),
            ("expand_device n<0", lambda c: L.dp_expand_batch_device(c, dg, -1, dk, da, None), STATE, ARG),
            ("expand_device null parents", lambda c: L.dp_expand_batch_device(c, None, NP, dk, da, None), STATE, ARG),
            ("expand_device null children", lambda c: L.dp_expand_batch_device(c, dg, NP, None, da, None), STATE, ARG),
            ("expand_device ref>=V", lambda c: L.dp_expand_batch_device(c, db, NP, dk, da, None), STATE, OK),
            ("fast_expand n=0", lambda c: L.dp_fast_expand_batch(c, ptr(good), 0, ptr(kids), ptr(acc)), OK, OK),
            ("fast_expand n<0", lambda c: L.dp_fast_expand_batch(c, ptr(good), -1, ptr(kids), ptr(acc)), ARG, ARG),
            ("fast_expand null parents", lambda c: L.dp_fast_expand_batch(c, None, NP, ptr(kids), ptr(acc)), ARG, ARG),
            ("fast_expand null children", lambda c: L.dp_fast_expand_batch(c, ptr(good), NP, None, ptr(acc)), ARG, ARG),
            ("fast_expand valid", lambda c: L.dp_fast_expand_batch(c, ptr(good), NP, ptr(kids), ptr(acc)), STATE, OK),
            ("fast_expand ref>=V", lambda c: L.dp_fast_expand_batch(c, ptr(bad), NP, ptr(kids), ptr(acc)), STATE, OK),
            ("fast_expand_device n=0", lambda c: L.dp_fast_expand_batch_device(c, dg, 0, dk, da, None), STATE, OK),
            ("fast_expand_device n<0", lambda c: L.dp_fast_expand_batch_device(c, dg, -1, dk, da, None), STATE, ARG),
            ("fast_expand_device null parents",
             lambda c: L.dp_fast_expand_batch_device(c, None, NP, dk, da, None), STATE, ARG),
            ("fast_expand_device null children",
             lambda c: L.dp_fast_expand_batch_device(c, dg, NP, None, da, None), STATE, ARG),
            ("fast_expand_device ref>=V", lambda c: L.dp_fast_expand_batch_device(c, db, NP, dk, da, None), STATE, OK),
            ("seeds n=0", lambda c: L.dp_seeds_to_patches(c, ptr(xyz), 0, ptr(out)), STATE, OK),
            ("seeds n<0", lambda c: L.dp_seeds_to_patches(c, ptr(xyz), -1, ptr(out)), ARG, ARG),
            ("seeds null points", lambda c: L.dp_seeds_to_patches(c, None, NP, ptr(out)), ARG, ARG),
            ("seeds null out", lambda c: L.dp_seeds_to_patches(c, ptr(xyz), NP, None), ARG, ARG),
            ("seeds valid", lambda c: L.dp_seeds_to_patches(c, ptr(xyz), NP, ptr(out)), STATE, OK),
        ]
        got, want = {}, {}
        for label, call, no_views, with_views in cases:
            for tag, e, code in (("no views", bare, no_views), ("hf6", eng, with_views)):
                if code is not None:
                    got[label, tag] = call(e._ctx)
                    want[label, tag] = code
            torch.cuda.synchronize()
        assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}

        # the record naming view V: every child rejected, on both engines and
        # through the device forms (the last calls above wrote d_kids / d_acc)
        for expand in (eng.expand, eng.fast_expand):
            _, a = expand(bad)
            assert not a[4:8].any()
        torch.cuda.synchronize()
        assert not d_acc.cpu().numpy()[4:8].any()
