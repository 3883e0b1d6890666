#!/usr/bin/env python3
"""dp_densify_iterate against the same result obtained with the store on the
host between rounds, on a BASELINE config, warm, in parity and performance
mode; the per-round counts and the geometry of the survivors against the
synthetic ground truth (dp_synth_surface) for 1 and N rounds.  One JSON line
per mode (DESIGN.md "Iterated expand-filter").

The host route uses only the calls that predate dp_densify_resume: dp_densify,
host dp_filter_patches, then a seed-less re-entry -- dp_densify_begin over the
patches' centres (its seed patches are never refined) and dp_densify_commit of
generation 0 with the patches themselves as the candidates and the keep flags
as the accept flags -- then dp_densify_run and dp_densify_result.

    python tools/iterate_timing.py [--config cfg3_32view_4k] [--iterations 3] [--repeat 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def geometry(cfg, p):
    from densepoints_amd import synth

    if not len(p):
        return {"n": 0}
    z, _ = synth.surface(cfg, p["pos"][:, :2].astype(np.float64))
    dz = np.abs(p["pos"][:, 2] - z)
    return {"n": int(len(p)), "median_abs_dz": float(np.median(dz)), "p90_abs_dz": float(np.percentile(dz, 90))}


def host_route(eng, seeds, rounds, passes):
    pat, _ = eng.densify(seeds)
    keep = eng.filter_patches(pat, passes)
    for _ in range(rounds - 1):
        g = eng.densify_begin(pat["pos"].astype(np.float64))
        g = eng.densify_commit(g, pat, keep)
        if g.items:
            eng.densify_run(g)
        pat, _ = eng.densify_result()
        keep = eng.filter_patches(pat, passes)
    return pat[keep != 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3_32view_4k")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--modes", default="parity,fast")
    a = ap.parse_args()
    import densepoints_amd as dp
    from densepoints_amd import _native as N
    from densepoints_amd import synth

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    cfg = synth.named(a.config)
    P = synth.cameras(cfg)
    V, W, H = cfg.n_views, cfg.width, cfg.height
    with dp.Engine(dp.Options(), device=0) as eng:
        planes = torch.empty((V, H, W), dtype=torch.int32, device="cuda")
        for v in range(V):
            N.check(N.lib.dp_synth_render_device(eng.handle, ctypes.byref(cfg), N.ptr(P), v, planes[v].data_ptr(),
                                                 stream.cuda_stream), eng.handle)
        torch.cuda.synchronize()
        eng.set_views_device(P, [W] * V, [H] * V, [W] * V, [p.data_ptr() for p in planes])
        seeds = synth.seeds(cfg, P)
        for mode in a.modes.split(","):
            eng.set_fast_options(dp.FastOptions(densify=1 if mode == "fast" else 0))
            routes = {"iterate": lambda: eng.densify_iterate(seeds, a.iterations, a.passes)[0],
                      "host": lambda: host_route(eng, seeds, a.iterations, a.passes)}
            rec = {"config": a.config, "mode": mode, "seeds": int(len(seeds)), "iterations": a.iterations}
            res = {}
            for name, fn in routes.items():
                fn()  # warm-up (gray planes, buffers, clocks)
                ts = []
                for _ in range(a.repeat):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res[name] = fn()
                    ts.append(round((time.perf_counter() - t0) * 1e3, 2))
                rec[name + "_ms"] = ts
            rec["identical"] = bool(res["iterate"].tobytes() == res["host"].tobytes())
            pn, stn = eng.densify_iterate(seeds, a.iterations, a.passes)
            p1, _ = eng.densify_iterate(seeds, 1, a.passes)
            rec["rounds"] = [{k: r[k] for k in ("offered", "reinserted", "patches", "filtered_out")}
                             for r in stn["iterations"]]
            rec["geometry_1"] = geometry(cfg, p1)
            rec["geometry_n"] = geometry(cfg, pn)
            print(json.dumps(rec), flush=True)
        eng.set_fast_options(dp.FastOptions())
        del planes


if __name__ == "__main__":
    main()
