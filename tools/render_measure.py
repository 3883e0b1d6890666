"""dp_render_maps on config 3 ("Depth, index and normal maps"): the
performance-mode store of the 32 x 3840 x 2160 scene rendered into depth and
index planes of all 32 views, device-resident -- render_ms (median of 7 warm
runs), pairs, pixel tests, z-buffer traffic, and the filter's visibility pass on
the same store for scale.

    python tools/render_measure.py [OUT_DIR]      (default bench_out/)
"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import densepoints_amd as dp
from densepoints_amd import _native as N, synth

torch.cuda.init()
cfg = synth.named("cfg3_32view_4k", seed_stride_px=32.0)
V, W, H = cfg.n_views, cfg.width, cfg.height
P = synth.cameras(cfg)
eng = dp.Engine(dp.Options(), device=0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
planes = torch.empty((V, H, W), dtype=torch.int32, device="cuda")
for v in range(V):
    N.check(N.lib.dp_synth_render_device(eng.handle, ctypes.byref(cfg), N.ptr(P), v, planes[v].data_ptr(),
                                         stream.cuda_stream), eng.handle)
torch.cuda.synchronize()
eng.set_views_device(P, [W] * V, [H] * V, [W] * V, [p.data_ptr() for p in planes])
seeds = synth.seeds(cfg, P)
eng.set_fast_options(dp.FastOptions(densify=1))
t0 = time.perf_counter()
pat, st = eng.densify(seeds, copy=False)
print("densify(fast): %d patches in %.3f s" % (len(pat), time.perf_counter() - t0), flush=True)
d_store, n = eng.densify_store_device()
depth = torch.empty((V, H, W), dtype=torch.float32, device="cuda")
index = torch.empty((V, H, W), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
runs = []
for k in range(9):
    s = eng.render_maps_device(d_store, n, None, range(V), [depth[v].data_ptr() for v in range(V)],
                               [index[v].data_ptr() for v in range(V)], stream=stream.cuda_stream)
    runs.append(s)
    print("run %d: %.3f ms" % (k, s["render_ms"]), flush=True)
warm = sorted(r["render_ms"] for r in runs[2:])
ms = statistics.median(warm)
s = runs[-1]
# the filter's visibility pass on the same store (rho + front + visibility), for scale
keep = torch.empty(n, dtype=torch.uint8, device="cuda")
ft = []
for k in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    eng.filter_patches_device(d_store, n, keep.data_ptr(), 1, stream=stream.cuda_stream)
    e1.record(stream)
    torch.cuda.synchronize()
    ft.append(e0.elapsed_time(e1))
zbytes = 8 * V * W * H
out = {"patches": s["patches"], "pairs": s["pairs"], "pixel_tests": s["pixel_tests"],
       "covered_pixels": s["covered_pixels"], "coverage": s["covered_pixels"] / (V * W * H),
       "render_ms_median": ms, "render_ms_min": warm[0], "render_ms_max": warm[-1],
       "pixel_tests_per_s": s["pixel_tests"] / (ms * 1e-3),
       "zbuffer_bytes": zbytes, "zbuffer_clear_plus_resolve_read_ms_at_8TBs": 2 * zbytes / 8e12 * 1e3,
       "filter_visibility_pass_ms_median": statistics.median(ft)}
print(json.dumps(out), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "render_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
