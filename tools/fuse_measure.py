"""dp_fuse_maps on config 3 ("Depth-map fusion"): the performance-mode
store of the 32 x 3840 x 2160 scene rendered into depth and normal planes of all
32 views and fused, device-resident -- fuse_ms (nine calls, the median of the
last seven), the point counts, matched pairs per second, and the two lower
bounds the code implies: the mask buffer's write and read, and the depth planes'
read, at 8 TB/s.

    python tools/fuse_measure.py [OUT_DIR]      (default bench_out/)
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
normal = torch.empty((V, H, W, 3), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
rs = eng.render_maps_device(d_store, n, None, range(V), [depth[v].data_ptr() for v in range(V)], None,
                            [normal[v].data_ptr() for v in range(V)], stream=stream.cuda_stream)
print("render: %d covered pixels in %.3f ms" % (rs["covered_pixels"], rs["render_ms"]), flush=True)
# an empty pixel is never emitted: the first call only counts, the rest write
cap, points = 0, None
runs = []
for k in range(9):
    n_out, s = eng.fuse_maps_device(range(V), [depth[v].data_ptr() for v in range(V)],
                                    [normal[v].data_ptr() for v in range(V)],
                                    points.data_ptr() if points is not None else None, cap,
                                    stream=stream.cuda_stream)
    runs.append(s)
    print("run %d: %.3f ms, %d points (cap %d)" % (k, s["fuse_ms"], n_out, cap), flush=True)
    if points is None:
        cap = n_out
        points = torch.empty((max(cap, 1), N.FUSED_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
warm = sorted(r["fuse_ms"] for r in runs[2:])
ms = statistics.median(warm)
s = runs[-1]
pixels = V * W * H
mask_bytes = 8 * s["depth_pixels"]
out = {"patches": int(n), "covered_pixels": rs["covered_pixels"], "render_ms": rs["render_ms"],
       "depth_pixels": s["depth_pixels"], "matched_pairs": s["matched_pairs"],
       "consistent_pairs": s["consistent_pairs"], "fusable": s["fusable"], "emitted": s["emitted"],
       "fuse_ms_median": ms, "fuse_ms_min": warm[0], "fuse_ms_max": warm[-1],
       "matched_pairs_per_s": s["matched_pairs"] / (ms * 1e-3),
       "observations_per_s": s["depth_pixels"] * (V - 1) / (ms * 1e-3),
       "mask_write_plus_read_ms_at_8TBs": 2 * mask_bytes / 8e12 * 1e3,
       "depth_planes_read_ms_at_8TBs": 4 * pixels / 8e12 * 1e3}
print(json.dumps(out), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "fuse_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
