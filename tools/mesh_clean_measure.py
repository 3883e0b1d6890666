"""dp_mesh_components and dp_mesh_clean on the config-3 mesh ("Mesh
clean-up"): the mesh tools/tsdf_measure.py measures (the performance-mode store
of the 32 x 3840 x 2160 scene, rendered, integrated into a 256^3 cube and
meshed with min_weight 2) and the same scene at dim = 512, device-resident --
clean_ms of both calls (nine calls each, the median of the last seven, device
events), the components, the sizes of the largest five, and the compulsory
bytes beside them: the triangles read twice (the union and the emit) plus the
vertices read and the kept vertices and triangles written, as times at 8 TB/s.

    python tools/mesh_clean_measure.py [OUT_DIR]      (default bench_out/)
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
DIMS = (256, 512)
KEEP = dict(max_components=1)

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
    cverts, ctris = torch.empty_like(verts), torch.empty_like(tris)
    torch.cuda.synchronize()
    eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), verts.data_ptr(), nv, tris.data_ptr(), nt,
                         min_weight=2, stream=stream.cuda_stream, **vol)
    del tsdf, weight, rgb
    print("dim %d: %d vertices, %d triangles" % (dim, nv, nt), flush=True)
    table = torch.empty((max(nv, 1), 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kruns, cruns = [], []
    for k in range(9):
        nc, s = eng.mesh_components_device(tris.data_ptr(), nt, nv, None, None, table.data_ptr(), nv,
                                           stream=stream.cuda_stream)
        kruns.append(s)
        print("components %d: %.3f ms, %d components" % (k, s["clean_ms"], nc), flush=True)
    for k in range(9):
        no, nto, s = eng.mesh_clean_device(verts.data_ptr(), nv, tris.data_ptr(), nt, cverts.data_ptr(), nv,
                                           ctris.data_ptr(), nt, stream=stream.cuda_stream, **KEEP)
        cruns.append(s)
        print("clean %d: %.3f ms, %d vertices, %d triangles kept" % (k, s["clean_ms"], no, nto), flush=True)
    rows = table[:nc].cpu().numpy().view(N.MESH_COMPONENT_DTYPE).reshape(-1)
    largest = sorted(rows["triangles"].tolist(), reverse=True)[:5]
    # per-root adds of the triangle count: one per distinct root of a wave's 64 triangles
    tc = torch.empty(max(nt, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.mesh_components_device(tris.data_ptr(), nt, nv, None, tc.data_ptr(), None, 0, stream=stream.cuda_stream)
    lab = tc[:nt].cpu().numpy()
    waves = [lab[i:i + 64] for i in range(0, nt, 64)]
    adds = [len(np.unique(w[w >= 0])) for w in waves]
    kwarm = sorted(r["clean_ms"] for r in kruns[2:])
    cwarm = sorted(r["clean_ms"] for r in cruns[2:])
    kms, cms = statistics.median(kwarm), statistics.median(cwarm)
    sc = cruns[-1]
    kbytes = 2 * 12 * nt + 16 * nc
    cbytes = 2 * 12 * nt + 16 * nv + 16 * sc["vertices_out"] + 12 * sc["triangles_out"]
    out["meshes"].append({
        "dim": dim, "volume": vol, "vertices": nv, "triangles": nt, "components": int(nc), "largest_five": largest,
        "invalid_triangles": sc["invalid_triangles"], "unused_vertices": sc["unused_vertices"],
        "triangle_count_adds_per_wave_mean": float(np.mean(adds)) if adds else 0.0,
        "triangle_count_adds_per_wave_max": int(max(adds)) if adds else 0,
        "components_ms_median": kms, "components_ms_min": kwarm[0], "components_ms_max": kwarm[-1],
        "components_ms_first": kruns[0]["clean_ms"],
        "components_compulsory_bytes": kbytes, "components_ms_at_8TBs": kbytes / HBM_BYTES_PER_S * 1e3,
        "components_fraction_of_hbm_peak": kbytes / HBM_BYTES_PER_S * 1e3 / kms,
        "clean_options": KEEP, "vertices_out": sc["vertices_out"], "triangles_out": sc["triangles_out"],
        "clean_ms_median": cms, "clean_ms_min": cwarm[0], "clean_ms_max": cwarm[-1], "clean_ms_first": cruns[0]["clean_ms"],
        "clean_compulsory_bytes": cbytes, "clean_ms_at_8TBs": cbytes / HBM_BYTES_PER_S * 1e3,
        "clean_fraction_of_hbm_peak": cbytes / HBM_BYTES_PER_S * 1e3 / cms})
    print(json.dumps(out["meshes"][-1]), flush=True)
    del verts, tris, cverts, ctris, table, tc
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_clean_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
