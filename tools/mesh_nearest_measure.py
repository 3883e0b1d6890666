"""dp_mesh_nearest on a named synthetic config ("Mesh surface
evaluation"): the scene densified and meshed (PMVS.mesh, the TSDF mesh and the
same decimated by two voxels with the mean and with the quadric placement), its
ground-truth height field (synth.surface) sampled on a regular grid over the
patches' extent as the truth cloud, and one JSON line: build_ms and query_ms of
truth -> mesh surface for the TSDF mesh and the decimated one (five calls each,
the median of the last three, device events) with the grid's facts, for scale
dp_cloud_nearest of the same truth against the same meshes' vertices,
mesh_compare ("mesh_surface") beside cloud_compare on the vertices
("mesh_vertices") before and after decimation, and mesh_deviation between the
TSDF mesh and either decimated one.  No time is asserted anywhere.

    python tools/mesh_nearest_measure.py [CONFIG] [GRID] [DIM] [OUT_DIR]
        (defaults: cfg1_4view_vga, 1024 samples along x, a volume of 256 voxels, bench_out/)
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
dim = int(sys.argv[3]) if len(sys.argv) > 3 else 256
out_dir = sys.argv[4] if len(sys.argv) > 4 else "bench_out"

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
meshes = {"tsdf": pm.mesh(dim=dim)}
voxel = float(pm.stats["mesh"]["voxel"])
meshes["decimated_mean"] = pm.mesh(dim=dim, decimate=dict(factor=2))
meshes["decimated_quadric"] = pm.mesh(dim=dim, decimate=dict(factor=2, quadric=True))

lo, hi = raw["pos"][:, :2].min(axis=0).astype(np.float64), raw["pos"][:, :2].max(axis=0).astype(np.float64)
pitch = float(hi[0] - lo[0]) / (grid - 1)
gx, gy = np.meshgrid(np.arange(lo[0], hi[0] + pitch / 2, pitch), np.arange(lo[1], hi[1] + pitch / 2, pitch), indexing="ij")
xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
z, _ = synth.surface(cfg, xy)
truth = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
tau = 2 * pitch
max_dist = 10 * tau
out = {"config": name, "patches": len(raw), "truth": len(truth), "pitch": pitch, "tau": tau, "max_dist": max_dist,
       "voxel": voxel, "dim": dim}


def timed(call, keys):
    runs = [call()["stats"] for _ in range(5)]
    row = {k: runs[-1][k] for k in keys}
    for key in ("build_ms", "query_ms"):
        row[key] = statistics.median(r[key] for r in runs[2:])
    return row


with dp.Engine(device=0) as eng:
    for label, (v, t) in meshes.items():
        row = {"vertices": len(v), "triangles": len(t)}
        row["truth_to_surface"] = timed(lambda: eng.mesh_nearest(truth, v, t, max_dist),
                                        ("queries", "matched", "triangles", "grid_cells", "grid_entries", "max_cell_entries"))
        row["truth_to_vertices"] = timed(lambda: eng.cloud_nearest(truth, v, max_dist),
                                         ("queries", "targets", "matched", "grid_cells", "max_cell_targets"))
        row["mesh_surface"] = dp.mesh_compare(eng, v, t, truth, tau)
        row["mesh_vertices"] = dp.cloud_compare(eng, v, truth, tau)
        if label != "tsdf":
            row["decimate_deviation"] = dp.mesh_deviation(eng, meshes["tsdf"], (v, t), max_dist)
        out[label] = row
print(json.dumps(out), flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_nearest_measure_%s.json" % name), "w") as f:
    json.dump(out, f, indent=1)
