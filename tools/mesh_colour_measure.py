"""dp_mesh_colour on the config-3 mesh ("Mesh colouring"): the scene
tools/mesh_render_measure.py measures (the performance-mode store of the
32 x 3840 x 2160 scene, rendered, integrated into a 256^3 cube and meshed with
min_weight 2), device-resident: its vertices coloured from all 32 views at
3840 x 2160 against the depth planes dp_mesh_render leaves, weighted by
dp_mesh_normals' normals -- colour_ms and this run's own render_ms (nine calls
each, the median of the last seven with min and max, device events), the
counters, and the mean absolute difference per channel between the new colours
and the TSDF colours of the coloured vertices.  No time is asserted anywhere.

    python tools/mesh_colour_measure.py [OUT_DIR]      (default bench_out/)
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
       "triangles": nt, "colours": []}
normals = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
coloured = torch.empty_like(verts)
seen = torch.empty(max(nv, 1), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
eng.mesh_normals_device(verts.data_ptr(), nv, tris.data_ptr(), nt, normals.data_ptr(), stream=stream.cuda_stream)
d_depth = [depth[v].data_ptr() for v in range(V)]
runs = [eng.mesh_render_device(verts.data_ptr(), nv, tris.data_ptr(), nt, range(V), d_depth, stream=stream.cuda_stream)
        for _ in range(9)]
out["render_ms"] = median_of(runs, "render_ms")
print(json.dumps({"render_ms": out["render_ms"]}), flush=True)
before = verts[:nv, 12:15].cpu().numpy().astype("float64")
for use_normals, bilinear in ((True, False), (True, True), (False, False)):
    runs = [eng.mesh_colour_device(verts.data_ptr(), nv, range(V), d_depth, coloured.data_ptr(),
                                   d_normals=normals.data_ptr() if use_normals else None, bilinear=bilinear,
                                   d_seen=seen.data_ptr(), stream=stream.cuda_stream) for _ in range(9)]
    s = runs[-1]
    after = coloured[:nv, 12:15].cpu().numpy().astype("float64")
    was_seen = seen[:nv].cpu().numpy() != 0
    row = {"normals": use_normals, "bilinear": bilinear, "counts": {k: s[k] for k in s if not k.endswith("_ms")},
           "colour_ms": median_of(runs, "colour_ms"),
           "mean_abs_diff_rgb": [float(x) for x in abs(after - before)[was_seen].mean(axis=0)] if was_seen.any() else None}
    out["colours"].append(row)
    print(json.dumps(row), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_colour_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
