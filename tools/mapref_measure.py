"""dp_refine_maps on config 3 ("Depth-map refinement"): the
performance-mode store of the 32 x 3840 x 2160 scene rendered into depth and
normal planes of all 32 views, then one and three refine passes, device-resident
-- refine_ms, the counters and window samples per second of each pass, and, from
dp_synth_surface, the median and p90 |depth - true depth| and the coverage of
the maps before and after (on a pixel subsample of a few views).  Nothing is
asserted on those figures.

    python tools/mapref_measure.py [OUT_DIR] [CONFIG]   (default bench_out/ cfg3_32view_4k)
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import densepoints_amd as dp
from densepoints_amd import _native as N, synth

name = sys.argv[2] if len(sys.argv) > 2 else "cfg3_32view_4k"
torch.cuda.init()
cfg = synth.named(name, seed_stride_px=32.0)
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
bufs = [(torch.empty((V, H, W), dtype=torch.float32, device="cuda"),
         torch.empty((V, H, W, 3), dtype=torch.float32, device="cuda")) for _ in range(2)]
torch.cuda.synchronize()
rs = eng.render_maps_device(d_store, n, None, range(V), [bufs[0][0][v].data_ptr() for v in range(V)], None,
                            [bufs[0][1][v].data_ptr() for v in range(V)], stream=stream.cuda_stream)
print("render: %d covered pixels in %.3f ms" % (rs["covered_pixels"], rs["render_ms"]), flush=True)
eng.build_gray()

SAMPLE_VIEWS, STRIDE = sorted({0, V // 3, (2 * V) // 3, V - 1}), 8


def quality(depth):
    """median and p90 |depth - true depth| and the coverage, on every STRIDE-th
    pixel of SAMPLE_VIEWS: the true depth is that of the ray's intersection with
    dp_synth_surface (secant iterations from the map's depth)"""
    err, covered, total = [], 0, 0
    for v in SAMPLE_VIEWS:
        z = depth[v, ::STRIDE, ::STRIDE].cpu().numpy().astype(np.float64)
        y, x = np.mgrid[0:H:STRIDE, 0:W:STRIDE].astype(np.float64)
        ok = z > 0
        total, covered = total + z.size, covered + int(ok.sum())
        z, x, y = z[ok], x[ok], y[ok]
        Mi, p4 = np.linalg.inv(P[v][:, :3]), P[v][:, 3]
        C = -Mi @ p4
        d = (Mi @ np.stack([x, y, np.ones_like(x)])).T  # X(t) = C + t d has depth t

        def f(t):
            X = C + t[:, None] * d
            return X[:, 2] - synth.surface(cfg, X[:, :2])[0]

        t0_, t1 = z * 0.999, z.copy()
        f0, f1 = f(t0_), f(t1)
        for _ in range(8):
            den = np.where(f1 != f0, f1 - f0, 1.0)
            t2 = np.where(f1 != f0, t1 - f1 * (t1 - t0_) / den, t1)
            t0_, f0, t1 = t1, f1, t2
            f1 = f(t1)
        err.append(np.abs(z - t1))
    err = np.concatenate(err) if err else np.zeros(1)
    return dict(median=float(np.median(err)), p90=float(np.percentile(err, 90)), coverage=covered / max(total, 1))


out = {"config": name, "patches": int(n), "covered_pixels": rs["covered_pixels"], "render_ms": rs["render_ms"],
       "before": quality(bufs[0][0]), "passes": []}
print("before:", json.dumps(out["before"]), flush=True)
window = dp.pmvs.MAPREF_DEFAULTS["window"]
cur = 0
for k in range(3):
    src, dst = bufs[cur], bufs[cur ^ 1]
    s = eng.refine_maps_device(range(V), [src[0][v].data_ptr() for v in range(V)],
                               [src[1][v].data_ptr() for v in range(V)], [dst[0][v].data_ptr() for v in range(V)],
                               [dst[1][v].data_ptr() for v in range(V)], stream=stream.cuda_stream)
    cur ^= 1
    s["samples_per_s"] = s["source_scores"] * window * window / (s["refine_ms"] * 1e-3)
    s["quality"] = quality(bufs[cur][0])
    out["passes"].append(s)
    print("pass %d:" % (k + 1), json.dumps(s), flush=True)
print(json.dumps(out), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mapref_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
