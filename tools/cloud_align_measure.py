"""dp_cloud_align on a synthetic surface cloud of N points and a rigidly moved,
jittered copy of it ("Cloud registration"): one JSON line per N with
grid_ms, iterate_ms and ms per pass of dp_cloud_align (ITER iterations, so ITER +
1 passes; the device form, the clouds already on the device), and in the same
run build_ms and query_ms of one dp_cloud_nearest_device call on the same clouds
(five calls each, the median of the last three, device events), and the ratio of
one pass to one whole dp_cloud_nearest call.  No time is asserted anywhere.

    python tools/cloud_align_measure.py [N ...] [--iterations ITER] [--out OUT_DIR]
        (defaults: 100000 1000000 4000000, 20, bench_out/)
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import densepoints_amd as dp

argv = sys.argv[1:]
iterations, out_dir = 20, "bench_out"
for flag in ("--iterations", "--out"):
    if flag in argv:
        k = argv.index(flag)
        value = argv[k + 1]
        del argv[k:k + 2]
        if flag == "--iterations":
            iterations = int(value)
        else:
            out_dir = value
sizes = [int(a) for a in argv] or [100000, 1000000, 4000000]

torch.cuda.init()


def surface(n, rng):
    """n points on a height field over the unit square"""
    xy = rng.random((n, 2))
    z = 0.1 * np.sin(6.0 * xy[:, 0]) * np.cos(5.0 * xy[:, 1]) + 0.05 * np.sin(17.0 * xy[:, 0] + 11.0 * xy[:, 1])
    return np.column_stack([xy, z]).astype(np.float32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


results = []
with dp.Engine(device=0) as eng:
    for n in sizes:
        rng = np.random.default_rng(n)
        target = surface(n, rng)
        spacing = float(1.0 / np.sqrt(n))
        # the copy: moved by a few spacings, jittered by a tenth of one
        M = np.hstack([rotation([1, 2, 3], 2.0 * spacing), np.array([[2.0], [-1.5], [1.0]]) * spacing])
        source = (target.astype(np.float64) @ M[:, :3].T + M[:, 3] +
                  rng.standard_normal((n, 3)) * 0.1 * spacing).astype(np.float32)
        R = float(np.float32(8.0 * spacing))
        ds, dt = device(source), device(target)
        d_index = torch.empty(n, dtype=torch.int32, device="cuda")
        d_dist = torch.empty(n, dtype=torch.float32, device="cuda")
        near = [eng.cloud_nearest_device(ds.data_ptr(), n, 12, dt.data_ptr(), n, 12, R, d_index.data_ptr(),
                                         d_dist.data_ptr()) for _ in range(5)]
        runs = [eng.cloud_align_device(ds.data_ptr(), n, 12, dt.data_ptr(), n, 12, R, iterations=iterations)
                for _ in range(5)]
        last = runs[-1]
        passes = last["stats"]["iterations_run"] + 1
        med = {k: statistics.median(r["stats"][k] for r in runs[2:]) for k in ("grid_ms", "iterate_ms")}
        nmed = {k: statistics.median(r[k] for r in near[2:]) for k in ("build_ms", "query_ms")}
        back = np.linalg.inv(np.vstack([M, [0, 0, 0, 1]]))[:3]
        out = {"n": n, "max_dist": R, "iterations": iterations, "passes": passes,
               "stop_reason": last["stats"]["stop_reason"], "matched": int(last["trace"]["matched"][passes - 1]),
               "rms_before": float(last["trace"]["rms"][0]), "rms": float(last["trace"]["rms"][passes - 1]),
               "matrix_error": float(np.abs(last["matrix"] - back).max()),
               "grid_ms": med["grid_ms"], "iterate_ms": med["iterate_ms"], "pass_ms": med["iterate_ms"] / passes,
               "nearest_build_ms": nmed["build_ms"], "nearest_query_ms": nmed["query_ms"],
               "nearest_ms": nmed["build_ms"] + nmed["query_ms"],
               "grid_cells": last["stats"]["grid_cells"], "max_cell_targets": last["stats"]["max_cell_targets"]}
        out["pass_over_nearest"] = out["pass_ms"] / out["nearest_ms"]
        print(json.dumps(out), flush=True)
        results.append(out)
        del ds, dt, d_index, d_dist
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "cloud_align_measure.json"), "w") as f:
    json.dump(results, f, indent=1)
