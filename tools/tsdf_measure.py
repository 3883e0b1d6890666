"""dp_tsdf_integrate and dp_tsdf_mesh on config 3 ("TSDF volume and
mesh"): the performance-mode store of the 32 x 3840 x 2160 scene rendered into
depth planes of all 32 views, integrated into a 256^3 volume around the patches
and meshed, device-resident -- integrate_ms and mesh_ms (nine calls each, the
median of the last seven), the counts, and the compulsory bytes beside them: the
three volumes' writes plus one depth read and one texel read per counted
observation for the integration, the tsdf and weight reads plus the vertex and
triangle writes for the mesh, as times at 8 TB/s.

    python tools/tsdf_measure.py [OUT_DIR]      (default bench_out/)
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

HBM_BYTES_PER_S = 8e12
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
# a DIM^3 cube centred on the patches' box: its longest side plus four voxels (= trunc) at either end
pos = pat["pos"].astype("float64")
lo, hi = pos.min(axis=0), pos.max(axis=0)
voxel = float((hi - lo).max()) / (DIM - 8)
vol = dict(origin=tuple(float(c) for c in (lo + hi) / 2 - voxel * DIM / 2), voxel=voxel, dim=(DIM, DIM, DIM),
           trunc=4 * voxel)
d_store, n = eng.densify_store_device()
depth = torch.empty((V, H, W), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
rs = eng.render_maps_device(d_store, n, None, range(V), [depth[v].data_ptr() for v in range(V)],
                            stream=stream.cuda_stream)
print("render: %d covered pixels in %.3f ms; volume %s" % (rs["covered_pixels"], rs["render_ms"], vol), flush=True)
points = vol["dim"][0] * vol["dim"][1] * vol["dim"][2]
tsdf = torch.empty(points, dtype=torch.float32, device="cuda")
weight = torch.empty(points, dtype=torch.int32, device="cuda")
rgb = torch.empty(points, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
iruns = []
for k in range(9):
    s = eng.tsdf_integrate_device(range(V), [depth[v].data_ptr() for v in range(V)], tsdf.data_ptr(),
                                  weight.data_ptr(), rgb.data_ptr(), stream=stream.cuda_stream, **vol)
    iruns.append(s)
    print("integrate %d: %.3f ms, %d observations" % (k, s["integrate_ms"], s["observations"]), flush=True)
# the first mesh call only counts, the rest write
vcap = tcap = 0
verts = tris = None
mruns = []
for k in range(9):
    nv, nt, s = eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(),
                                     verts.data_ptr() if verts is not None else None, vcap,
                                     tris.data_ptr() if tris is not None else None, tcap, min_weight=2,
                                     stream=stream.cuda_stream, **vol)
    mruns.append(s)
    print("mesh %d: %.3f ms, %d vertices, %d triangles (caps %d, %d)" % (k, s["mesh_ms"], nv, nt, vcap, tcap),
          flush=True)
    if verts is None:
        vcap, tcap = nv, nt
        verts = torch.empty((max(vcap, 1), 16), dtype=torch.uint8, device="cuda")
        tris = torch.empty((max(tcap, 1), 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
iwarm = sorted(r["integrate_ms"] for r in iruns[2:])
mwarm = sorted(r["mesh_ms"] for r in mruns[2:])
ims, mms = statistics.median(iwarm), statistics.median(mwarm)
si, sm = iruns[-1], mruns[-1]
ibytes = 12 * points + 8 * si["observations"]
mbytes = 8 * points + 16 * sm["vertices"] + 12 * sm["triangles"]
out = {"patches": int(n), "volume": vol, "voxels": si["voxels"], "observations": si["observations"],
       "observed_voxels": si["observed_voxels"], "near_voxels": si["near_voxels"],
       "integrate_ms_median": ims, "integrate_ms_min": iwarm[0], "integrate_ms_max": iwarm[-1],
       "integrate_compulsory_bytes": ibytes, "integrate_ms_at_8TBs": ibytes / HBM_BYTES_PER_S * 1e3,
       "integrate_fraction_of_hbm_peak": ibytes / HBM_BYTES_PER_S * 1e3 / ims,
       "voxel_views_per_s": si["voxels"] * V / (ims * 1e-3),
       "active_cells": sm["active_cells"], "vertices": sm["vertices"], "triangles": sm["triangles"],
       "mesh_ms_median": mms, "mesh_ms_min": mwarm[0], "mesh_ms_max": mwarm[-1],
       "mesh_compulsory_bytes": mbytes, "mesh_ms_at_8TBs": mbytes / HBM_BYTES_PER_S * 1e3,
       "mesh_fraction_of_hbm_peak": mbytes / HBM_BYTES_PER_S * 1e3 / mms}
print(json.dumps(out), flush=True)
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "tsdf_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
