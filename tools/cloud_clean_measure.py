"""dp_cloud_knn and dp_cloud_clean on the fused cloud of a named synthetic config
("Cloud neighbours and outlier removal"): the scene densified and
fused (PMVS.fused_cloud), the radius four times the cloud's mean spacing in the
image plane of the height field, and one JSON line: build_ms and query_ms of
dp_cloud_nearest (the yardstick, the cloud against itself) and of dp_cloud_knn at
k = 1, 8, 16 and 32 with their full / partial / empty counts, knn_ms and clean_ms
of dp_cloud_clean at k = 8 with what it removed, and the two ratios knn(k = 1) /
cloud_nearest and knn(k = 8) / knn(k = 1) of the query times (five calls each,
the median of the last three, device events).  No time is asserted anywhere.

    python tools/cloud_clean_measure.py [CONFIG] [OUT_DIR]
        (defaults: cfg1_4view_vga, bench_out/)
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
out_dir = sys.argv[2] if len(sys.argv) > 2 else "bench_out"

torch.cuda.init()
cfg = synth.named(name)
P, imgs, seeds = synth.scene_host(cfg)
pm = dp.PMVS(fast=dp.FastOptions(densify=1))
for v in range(cfg.n_views):
    pm.add_camera(dp.View(P[v], imgs[v]))
t0 = time.perf_counter()
pm.run(seeds)
cloud = pm.fused_cloud()
print("densify(fast) + fuse: %d patches, %d fused points in %.3f s" % (len(pm.patches), len(cloud),
                                                                     time.perf_counter() - t0), flush=True)
pos = cloud["pos"].astype(np.float64)
ext = pos[:, :2].max(axis=0) - pos[:, :2].min(axis=0)
spacing = float(np.sqrt(ext[0] * ext[1] / max(len(cloud), 1)))
R = float(np.float32(4 * spacing))
out = {"config": name, "patches": len(pm.patches), "fused": len(cloud), "spacing": spacing, "max_dist": R}


def median_ms(runs, keys):
    return {key: statistics.median(r[key] for r in runs[2:]) for key in keys}


with dp.Engine(device=0) as eng:
    runs = [eng.cloud_nearest(cloud, cloud, R)["stats"] for _ in range(5)]
    out["cloud_nearest"] = dict(median_ms(runs, ("build_ms", "query_ms")), grid_cells=runs[-1]["grid_cells"],
                                max_cell_targets=runs[-1]["max_cell_targets"])
    for k in (1, 8, 16, 32):
        runs = [eng.cloud_knn(cloud, cloud, k, R)["stats"] for _ in range(5)]
        s = runs[-1]
        out["knn_k%d" % k] = dict(median_ms(runs, ("build_ms", "query_ms")),
                                  **{c: s[c] for c in ("full", "partial", "empty", "neighbours")})
    runs = [eng.cloud_clean(cloud, 8, R)["stats"] for _ in range(5)]
    s = runs[-1]
    out["clean_k8"] = dict(median_ms(runs, ("knn_ms", "clean_ms")),
                           **{c: s[c] for c in ("points", "eligible", "kept", "removed_sparse", "removed_far", "mu",
                                                "sigma", "threshold")})
out["knn1_over_cloud_nearest"] = out["knn_k1"]["query_ms"] / out["cloud_nearest"]["query_ms"]
out["knn8_over_knn1"] = out["knn_k8"]["query_ms"] / out["knn_k1"]["query_ms"]
print(json.dumps(out), flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "cloud_clean_measure_%s.json" % name), "w") as f:
    json.dump(out, f, indent=1)
