"""dp_mesh_decimate on the config-3 meshes ("Mesh simplification"): the
scene tools/mesh_smooth_measure.py measures (the performance-mode store of the
32 x 3840 x 2160 scene, rendered, integrated into a dim^3 cube and meshed with
min_weight 2) at dim = 128, 256 and 512, device-resident, at cells of 2 and 4
voxels anchored at the volume's origin, in both modes -- decimate_ms (nine calls,
the median of the last seven, device events), vertices and triangles in and out,
the counts, and the compulsory bytes beside them as a time at 8 TB/s: the
triangles read (12 B each), the used records read (16 B each; QUADRIC: the
three records of every proper triangle once more), the records and triangles
written.  The sorts' own passes and the scratch arrays are not compulsory and
not counted.

    python tools/mesh_decimate_measure.py [OUT_DIR]      (default bench_out/)
"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import densepoints_amd as dp
from densepoints_amd import _native as N, synth

HBM_BYTES_PER_S = 8e12
DIMS = (128, 256, 512)
FACTORS = (2.0, 4.0)

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
pos = pat["pos"].astype("float64")
lo, hi = pos.min(axis=0), pos.max(axis=0)
d_store, n = eng.densify_store_device()
depth = torch.empty((V, H, W), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
eng.render_maps_device(d_store, n, None, range(V), [depth[v].data_ptr() for v in range(V)], stream=stream.cuda_stream)


def median_of(runs, key):
    warm = sorted(r[key] for r in runs[2:])
    return dict(median=statistics.median(warm), min=warm[0], max=warm[-1], first=runs[0][key])


out = {"patches": int(n), "meshes": []}
for dim in DIMS:
    # tsdf_measure's volume: a dim^3 cube centred on the patches' box, four voxels (= trunc) of padding
    voxel = float((hi - lo).max()) / (dim - 8)
    vol = dict(origin=tuple(float(c) for c in (lo + hi) / 2 - voxel * dim / 2), voxel=voxel, dim=(dim, dim, dim),
               trunc=4 * voxel)
    points = dim ** 3
    tsdf = torch.empty(points, dtype=torch.float32, device="cuda")
    weight = torch.empty(points, dtype=torch.int32, device="cuda")
    rgb = torch.empty(points, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.tsdf_integrate_device(range(V), [depth[v].data_ptr() for v in range(V)], tsdf.data_ptr(), weight.data_ptr(),
                              rgb.data_ptr(), stream=stream.cuda_stream, **vol)
    nv, nt, _ = eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), None, 0, None, 0, min_weight=2,
                                     stream=stream.cuda_stream, **vol)
    verts = torch.empty((max(nv, 1), 16), dtype=torch.uint8, device="cuda")
    tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    overts, otris = torch.empty_like(verts), torch.empty_like(tris)
    torch.cuda.synchronize()
    eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), verts.data_ptr(), nv, tris.data_ptr(), nt,
                         min_weight=2, stream=stream.cuda_stream, **vol)
    del tsdf, weight, rgb
    print("dim %d: %d vertices, %d triangles" % (dim, nv, nt), flush=True)
    for factor in FACTORS:
        for quadric in (False, True):
            cell = float(np.float32(factor * float(np.float32(voxel))))
            runs = []
            for k in range(9):
                vo, to, s = eng.mesh_decimate_device(verts.data_ptr(), nv, tris.data_ptr(), nt, overts.data_ptr(), nv,
                                                     otris.data_ptr(), nt, cell, vol["origin"], quadric,
                                                     stream=stream.cuda_stream)
                runs.append(s)
            s = runs[-1]
            used = nv - s["unused_vertices"]
            proper = nt - s["invalid_triangles"] - s["degenerate_triangles"]
            nbytes = 12 * nt + 16 * used + (3 * 16 * proper if quadric else 0) + 16 * vo + 12 * to
            ms = median_of(runs, "decimate_ms")
            row = {"dim": dim, "volume": vol, "factor": factor, "cell": cell, "mode": "quadric" if quadric else "mean",
                   "vertices_in": nv, "triangles_in": nt, "vertices_out": vo, "triangles_out": to,
                   "counts": {k: s[k] for k in s if not k.endswith("_ms")}, "decimate_ms": ms,
                   "compulsory_bytes": nbytes, "ms_at_8TBs": nbytes / HBM_BYTES_PER_S * 1e3,
                   "fraction_of_hbm_peak": nbytes / HBM_BYTES_PER_S * 1e3 / ms["median"]}
            out["meshes"].append(row)
            print(json.dumps(row), flush=True)
    del verts, tris, overts, otris
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_decimate_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
