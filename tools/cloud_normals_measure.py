"""dp_cloud_normals on the fused cloud of a named synthetic config (DESIGN.md,
"Cloud normals"): the scene densified and fused (PMVS.fused_cloud), the cloud
against itself with max_dist four times its mean spacing in the image plane of
the height field, at k = 8, 16 and 32, and one JSON line: knn_ms and normals_ms
of dp_cloud_normals with its classes, beside build_ms + query_ms of dp_cloud_knn
at the same k on the same cloud (the yardstick), and the ratios normals_ms /
knn_ms and normals_ms / dp_cloud_knn's total (five calls each, the median of the
last three, device events).  BENCH_JSON, when given, is a file with the JSON
line bench.py printed on the same tree; it is copied into the result under
"bench" (nothing of this runs in the flagship workload).  No time is asserted
anywhere.

    python tools/cloud_normals_measure.py [CONFIG] [OUT_DIR] [BENCH_JSON]
        (defaults: cfg1_4view_vga, bench_out/, none)
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
bench_json = sys.argv[3] if len(sys.argv) > 3 else None

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
    for k in (8, 16, 32):
        runs = [eng.cloud_knn(cloud, cloud, k, R)["stats"] for _ in range(5)]
        knn = dict(median_ms(runs, ("build_ms", "query_ms")), neighbours=runs[-1]["neighbours"], full=runs[-1]["full"])
        runs = [eng.cloud_normals(cloud, k, max_dist=R, directions=True)["stats"] for _ in range(5)]
        s = runs[-1]
        nrm = dict(median_ms(runs, ("knn_ms", "normals_ms")),
                   **{c: s[c] for c in ("points", "estimated", "sparse", "degenerate", "flipped", "unoriented")})
        out["k%d" % k] = {"cloud_knn": knn, "cloud_normals": nrm,
                          "normals_over_own_knn": nrm["normals_ms"] / nrm["knn_ms"],
                          "normals_over_cloud_knn": nrm["normals_ms"] / (knn["build_ms"] + knn["query_ms"])}
if bench_json:
    with open(bench_json) as f:
        lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
    out["bench"] = json.loads(lines[-1])
print(json.dumps(out), flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "cloud_normals_measure_%s.json" % name), "w") as f:
    json.dump(out, f, indent=1)
