"""The C-level refusals of a bad view list by dp_render_maps, dp_fuse_maps,
dp_refine_maps and dp_tsdf_integrate, in the host and the device form, called
through ctypes: the Python wrappers raise ValueError before the C checks run,
so nothing else reaches them.  The expected codes (DP_E_ARG = -1, DP_E_STATE =
-5) and texts are those of include/densepoints.h and of the messages the entry
points have always set; every refusal comes before any device work.  The planes
handed in are real (host memory for the host forms, device memory for the
device forms) and large enough for any view here."""
import ctypes

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
ENTRIES = ["dp_render_maps", "dp_fuse_maps", "dp_refine_maps", "dp_tsdf_integrate"]
FORMS = ["host", "device"]
MAX_N = 66                 # entries of every table handed in
PLANE = 16 * 12 * 3 * 4    # bytes of the largest plane (a normal map of 16 x 12)


def make_views(V, W, H):
    K = np.array([[float(W), 0.0, W / 2.0], [0.0, float(W), H / 2.0], [0.0, 0.0, 1.0]])
    views = []
    for v in range(V):
        Rt = np.hstack([np.eye(3), np.array([[0.01 * v], [0.0], [2.0]])])
        views.append(dp.View(K @ Rt, np.zeros((H, W, 3), np.uint8)))
    return views


class Planes:
    """MAX_N depth and MAX_N normal planes in one buffer, as two pointer tables"""

    def __init__(self, form):
        if form == "device":
            import torch

            self.buf = torch.zeros(2 * MAX_N * PLANE, dtype=torch.uint8, device="cuda")
            base = self.buf.data_ptr()
        else:
            self.buf = np.zeros(2 * MAX_N * PLANE, np.uint8)
            base = self.buf.ctypes.data
        self.depth = (ctypes.c_void_p * MAX_N)(*[base + k * PLANE for k in range(MAX_N)])
        self.normal = (ctypes.c_void_p * MAX_N)(*[base + (MAX_N + k) * PLANE for k in range(MAX_N)])


@pytest.fixture(scope="module")
def planes():
    return {form: Planes(form) for form in FORMS}


@pytest.fixture(scope="module")
def ordinary():
    with dp.Engine(device=0) as eng:
        eng.set_views(make_views(4, 16, 12))
        yield eng


@pytest.fixture(scope="module")
def capped():
    with dp.Engine(device=0) as eng:
        eng.set_views(make_views(65, 8, 8))
        yield eng


@pytest.fixture(scope="module")
def empty():
    with dp.Engine(device=0) as eng:
        yield eng


def call(eng, entry, form, views, n_views, depth, normal):
    """the entry point with nothing wanted but the view list and the input
    planes: no patches, default options, no outputs, a 2 x 2 x 2 volume"""
    c, dev = eng.handle, form == "device"
    f = getattr(N.lib, entry + ("_device" if dev else ""))
    vp = None if views is None else (ctypes.c_int32 * MAX_N)(*(list(views) + [0] * (MAX_N - len(views))))
    tail = (None,) if dev else ()  # the stream
    if entry == "dp_render_maps":
        return f(c, None, 0, None, vp, n_views, None, None, None, None, None, None, *tail)
    if entry == "dp_fuse_maps":
        n_out, out = ctypes.c_int64(0), ctypes.c_void_p()
        if dev:
            return f(c, vp, n_views, None, depth, normal, None, 0, ctypes.byref(n_out), None, None)
        return f(c, vp, n_views, None, depth, normal, ctypes.byref(out), ctypes.byref(n_out), None)
    if entry == "dp_refine_maps":
        return f(c, vp, n_views, None, None, depth, normal, None, None, None, None, None, *tail)
    to = N.DpTsdfOptions((ctypes.c_float * 3)(0.0, 0.0, 0.0), 1.0, (ctypes.c_int32 * 3)(2, 2, 2), 1.0, 1, 0)
    return f(c, vp, n_views, ctypes.byref(to), depth, None, None, None, None, *tail)


def refused(eng, entry, form, planes, views, n_views, code, text, depth=None):
    p = planes[form]
    rc = call(eng, entry, form, views, n_views, p.depth if depth is None else depth, p.normal)
    msg = N.lib.dp_last_error(eng.handle).decode()
    assert (rc, msg) == (code, entry + ": " + text), (entry, form, views, n_views)


def range_text(entry):
    return "n_views must be in 1..V" if entry == "dp_render_maps" else "n_views must be in 1..min(V, 64)"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_view_list_refusals(ordinary, capped, empty, planes, entry, form):
    V = 4
    refused(empty, entry, form, planes, [0], 1, E_STATE, "no views set")
    refused(ordinary, entry, form, planes, None, 1, E_ARG, range_text(entry))
    refused(ordinary, entry, form, planes, [0, 1], 0, E_ARG, range_text(entry))
    refused(ordinary, entry, form, planes, list(range(V)) + [0], V + 1, E_ARG, range_text(entry))
    unique = "view ids must be unique and < V"
    refused(ordinary, entry, form, planes, [0, 1, 1], 3, E_ARG, unique)
    refused(ordinary, entry, form, planes, [0, 1, V], 3, E_ARG, unique)
    refused(ordinary, entry, form, planes, [0, -1], 2, E_ARG, unique)
    # 65 of 65 views: beyond the cap of 64 for all but render, whose only cap is
    # V -- it gets as far as the ids, of which the last repeats the one before
    ids = list(range(64)) + [63]
    refused(capped, entry, form, planes, ids, 65, E_ARG, unique if entry == "dp_render_maps" else range_text(entry))
    refused(capped, entry, form, planes, list(range(66)), 66, E_ARG, range_text(entry))
    if entry != "dp_render_maps":  # render has no input planes
        p = planes[form]
        holed = (ctypes.c_void_p * MAX_N)(*[None if k == 1 else p.depth[k] for k in range(MAX_N)])
        refused(ordinary, entry, form, planes, [0, 1, 2], 3, E_ARG, "a plane pointer is NULL", depth=holed)


def test_render_accepts_more_than_64_views(capped):
    """n_views = 65 is in render's range: with no patches and no output planes the
    host form clears its z-buffer, resolves nothing and returns DP_OK"""
    assert call(capped, "dp_render_maps", "host", list(range(65)), 65, None, None) == 0
