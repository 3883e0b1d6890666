"""dp_mesh_render on the config-3 mesh ("Mesh rendering"): the scene
tools/mesh_decimate_measure.py measures (the performance-mode store of the
32 x 3840 x 2160 scene, rendered, integrated into a 256^3 cube and meshed with
min_weight 2), device-resident, rendered back into all 32 views at 3840 x 2160,
depth planes only, with and without back-face culling -- render_ms (nine calls,
the median of the last seven, device events), pairs, pixel tests and covered
pixels.  No time is asserted anywhere.

    python tools/mesh_render_measure.py [OUT_DIR]      (default bench_out/)
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

DIM = 256

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
disc = eng.render_maps_device(d_store, n, None, range(V), [depth[v].data_ptr() for v in range(V)],
                              stream=stream.cuda_stream)

# tsdf_measure's volume: a DIM^3 cube centred on the patches' box, four voxels (= trunc) of padding
voxel = float((hi - lo).max()) / (DIM - 8)
vol = dict(origin=tuple(float(c) for c in (lo + hi) / 2 - voxel * DIM / 2), voxel=voxel, dim=(DIM, DIM, DIM),
           trunc=4 * voxel)
tsdf = torch.empty(DIM ** 3, dtype=torch.float32, device="cuda")
weight = torch.empty(DIM ** 3, dtype=torch.int32, device="cuda")
rgb = torch.empty(DIM ** 3, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
eng.tsdf_integrate_device(range(V), [depth[v].data_ptr() for v in range(V)], tsdf.data_ptr(), weight.data_ptr(),
                          rgb.data_ptr(), stream=stream.cuda_stream, **vol)
nv, nt, _ = eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), None, 0, None, 0, min_weight=2,
                                 stream=stream.cuda_stream, **vol)
verts = torch.empty((max(nv, 1), 16), dtype=torch.uint8, device="cuda")
tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), verts.data_ptr(), nv, tris.data_ptr(), nt,
                     min_weight=2, stream=stream.cuda_stream, **vol)
del tsdf, weight, rgb
print("dim %d: %d vertices, %d triangles" % (DIM, nv, nt), flush=True)


def median_of(runs, key):
    warm = sorted(r[key] for r in runs[2:])
    return dict(median=statistics.median(warm), min=warm[0], max=warm[-1], first=runs[0][key])


out = {"patches": int(n), "views": V, "width": W, "height": H, "dim": DIM, "volume": vol, "vertices": nv,
       "triangles": nt, "disc_render": {k: disc[k] for k in disc}, "renders": []}
for cull in (False, True):
    runs = []
    for k in range(9):
        runs.append(eng.mesh_render_device(verts.data_ptr(), nv, tris.data_ptr(), nt, range(V),
                                           [depth[v].data_ptr() for v in range(V)], cull_back=cull,
                                           stream=stream.cuda_stream))
    s = runs[-1]
    row = {"cull_back": cull, "counts": {k: s[k] for k in s if not k.endswith("_ms")},
           "render_ms": median_of(runs, "render_ms")}
    out["renders"].append(row)
    print(json.dumps(row), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_render_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
