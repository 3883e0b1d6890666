"""dp_mesh_adjacency, dp_mesh_smooth and dp_mesh_normals on the config-3 mesh
("Mesh smoothing and normals"): the mesh tools/mesh_clean_measure.py
measures (the performance-mode store of the 32 x 3840 x 2160 scene, rendered,
integrated into a 256^3 cube and meshed with min_weight 2) and the same scene at
dim = 512, device-resident -- adjacency_ms, smooth_ms (10 iterations = 20
steps) and normals_ms (nine calls each, the median of the last seven, device
events), the counts, and the compulsory bytes beside them as times at 8 TB/s:
the adjacency reads the triangles and writes the rows (8 B per entry), the
offsets and the flags; a smoothing step reads the offsets, the flags, the rows'
neighbours and every position once and writes every position; the normals read
the triangles and the records and write 12 B per vertex.  None of the three
counts the sort's own passes: they are not compulsory.

    python tools/mesh_smooth_measure.py [OUT_DIR]      (default bench_out/)
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
DIMS = (256, 512)
ITERATIONS = 10

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


out = {"patches": int(n), "iterations": ITERATIONS, "meshes": []}
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
    sverts = torch.empty_like(verts)
    normals = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.tsdf_mesh_device(tsdf.data_ptr(), weight.data_ptr(), rgb.data_ptr(), verts.data_ptr(), nv, tris.data_ptr(), nt,
                         min_weight=2, stream=stream.cuda_stream, **vol)
    del tsdf, weight, rgb
    print("dim %d: %d vertices, %d triangles" % (dim, nv, nt), flush=True)
    offsets = torch.empty(nv + 1, dtype=torch.int32, device="cuda")
    flags = torch.empty(max(nv, 1), dtype=torch.uint8, device="cuda")
    nbr = torch.empty(max(6 * nt, 1), dtype=torch.int32, device="cuda")
    cnt = torch.empty_like(nbr)
    torch.cuda.synchronize()
    aruns, sruns, nruns = [], [], []
    for k in range(9):
        E, s = eng.mesh_adjacency_device(tris.data_ptr(), nt, nv, offsets.data_ptr(), nbr.data_ptr(), cnt.data_ptr(),
                                         6 * nt, flags.data_ptr(), stream=stream.cuda_stream)
        aruns.append(s)
        print("adjacency %d: %.3f ms, %d entries" % (k, s["adjacency_ms"], E), flush=True)
    for k in range(9):
        s = eng.mesh_smooth_device(verts.data_ptr(), nv, tris.data_ptr(), nt, sverts.data_ptr(), iterations=ITERATIONS,
                                   stream=stream.cuda_stream)
        sruns.append(s)
        print("smooth %d: adjacency %.3f ms, %d steps %.3f ms" % (k, s["adjacency_ms"], s["steps"], s["smooth_ms"]),
              flush=True)
    for k in range(9):
        s = eng.mesh_normals_device(sverts.data_ptr(), nv, tris.data_ptr(), nt, normals.data_ptr(),
                                    stream=stream.cuda_stream)
        nruns.append(s)
        print("normals %d: %.3f ms, %d zero" % (k, s["normals_ms"], s["zero_normals"]), flush=True)
    a, sm, nr = aruns[-1], sruns[-1], nruns[-1]
    steps = sm["steps"]
    abytes = 12 * nt + 8 * E + 4 * (nv + 1) + nv
    # per step: offsets, flags, the neighbours, every position read and written; plus the unpack and the pack
    sbytes = steps * (4 * (nv + 1) + nv + 4 * E + 24 * nv) + (16 + 12) * nv + (12 + 4 + 16) * nv
    nbytes = 12 * nt + 16 * nv + 12 * nv
    ams, sms, nms = median_of(aruns, "adjacency_ms"), median_of(sruns, "smooth_ms"), median_of(nruns, "normals_ms")
    row = {"dim": dim, "volume": vol, "vertices": nv, "triangles": nt, "entries": int(E),
           "counts": {k: a[k] for k in a if not k.endswith("_ms")},
           "movable_vertices": sm["movable_vertices"], "pinned_vertices": sm["pinned_vertices"], "steps": steps,
           "zero_normals": nr["zero_normals"],
           "adjacency_ms": ams, "adjacency_ms_inside_smooth": median_of(sruns, "adjacency_ms"), "smooth_ms": sms,
           "smooth_ms_per_step": sms["median"] / max(steps, 1), "normals_ms": nms,
           "adjacency_compulsory_bytes": abytes, "adjacency_ms_at_8TBs": abytes / HBM_BYTES_PER_S * 1e3,
           "adjacency_fraction_of_hbm_peak": abytes / HBM_BYTES_PER_S * 1e3 / ams["median"],
           "smooth_compulsory_bytes": sbytes, "smooth_ms_at_8TBs": sbytes / HBM_BYTES_PER_S * 1e3,
           "smooth_fraction_of_hbm_peak": sbytes / HBM_BYTES_PER_S * 1e3 / sms["median"],
           "normals_compulsory_bytes": nbytes, "normals_ms_at_8TBs": nbytes / HBM_BYTES_PER_S * 1e3,
           "normals_fraction_of_hbm_peak": nbytes / HBM_BYTES_PER_S * 1e3 / nms["median"]}
    out["meshes"].append(row)
    print(json.dumps(row), flush=True)
    del verts, tris, sverts, normals, offsets, flags, nbr, cnt
out_dir = sys.argv[1] if len(sys.argv) > 1 else "bench_out"
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "mesh_smooth_measure.json"), "w") as f:
    json.dump(out, f, indent=1)
eng.close()
