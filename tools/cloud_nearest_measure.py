"""dp_cloud_nearest on a named synthetic config ("Cloud evaluation"):
the scene densified, its ground-truth height field (synth.surface) sampled on a
regular grid over the patches' extent as the truth cloud, and one JSON line:
build_ms and query_ms of both directions (five calls each, the median of the
last three, device events), the point counts, grid_cells, max_cell_targets, the
accuracy / completeness / F-score of the patch cloud with the filtered cloud
beside it, and for scale the time of a brute-force pass (torch.cdist in fp32,
chunked) at a size where that is affordable.  No time is asserted anywhere.

    python tools/cloud_nearest_measure.py [CONFIG] [GRID] [OUT_DIR]
        (defaults: cfg1_4view_vga, 1024 samples along x, bench_out/)
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import densepoints_amd as dp
from densepoints_amd import synth

name = sys.argv[1] if len(sys.argv) > 1 else "cfg1_4view_vga"
grid = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
out_dir = sys.argv[3] if len(sys.argv) > 3 else "bench_out"
BRUTE = 20000  # queries and targets of the brute-force pass

torch.cuda.init()
cfg = synth.named(name)
P, imgs, seeds = synth.scene_host(cfg)
pm = dp.PMVS(fast=dp.FastOptions(densify=1))
for v in range(cfg.n_views):
    pm.add_camera(dp.View(P[v], imgs[v]))
t0 = time.perf_counter()
pm.run(seeds)
raw = pm.patches
print("densify(fast): %d patches in %.3f s" % (len(raw), time.perf_counter() - t0), flush=True)
with dp.Engine(pm.options, device=0) as eng:
    eng.set_views(pm.views)
    keep = eng.filter_patches(raw, 1)
filtered = raw[keep == 1]

lo, hi = raw["pos"][:, :2].min(axis=0).astype(np.float64), raw["pos"][:, :2].max(axis=0).astype(np.float64)
pitch = float(hi[0] - lo[0]) / (grid - 1)
gx, gy = np.meshgrid(np.arange(lo[0], hi[0] + pitch / 2, pitch), np.arange(lo[1], hi[1] + pitch / 2, pitch), indexing="ij")
xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
z, _ = synth.surface(cfg, xy)
truth = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
tau = 2 * pitch
out = {"config": name, "patches": len(raw), "filtered": len(filtered), "truth": len(truth), "pitch": pitch, "tau": tau,
       "max_dist": 10 * tau}


def timed(eng, q, t):
    runs = [eng.cloud_nearest(q, t, 10 * tau)["stats"] for _ in range(5)]
    s = runs[-1]
    row = {k: s[k] for k in ("queries", "targets", "matched", "grid_cells", "max_cell_targets")}
    for key in ("build_ms", "query_ms"):
        row[key] = statistics.median(r[key] for r in runs[2:])
    return row


with dp.Engine(device=0) as eng:
    out["patches_to_truth"] = timed(eng, raw, truth)
    out["truth_to_patches"] = timed(eng, truth, raw)
    for label, cloud in (("patches", raw), ("filtered", filtered)):
        c = dp.cloud_compare(eng, cloud, truth, tau)
        out[label + "_quality"] = {"accuracy": c["accuracy"], "completeness": c["completeness"], "fscore": c["fscore"]}
    # for scale: all pairs of up to BRUTE x BRUTE points, evenly thinned, in fp32 (no radius, no ties rule), and the grid on the same
    bq = np.ascontiguousarray(raw["pos"][::max(1, len(raw) // BRUTE)][:BRUTE])
    bt = np.ascontiguousarray(truth[::max(1, len(truth) // BRUTE)][:BRUTE])
    q, t = torch.from_numpy(bq).cuda(), torch.from_numpy(bt).cuda()
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best = torch.cat([torch.cdist(q[i:i + 4096], t).min(dim=1).values for i in range(0, len(q), 4096)])
        torch.cuda.synchronize()
        brute_ms = (time.perf_counter() - t0) * 1e3
    out["brute_force"] = {"queries": len(q), "targets": len(t), "ms": brute_ms,
                          "grid": timed(eng, bq, bt)}
print(json.dumps(out), flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "cloud_nearest_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
