"""Host-side mirror of the reference's methods/pmvs + modules/core + modules/io
plugin surface, driving the HIP C ABI.

Reference interface -> here:
  View (modules/core/types.h:37-74)                  -> View
  PMVS::Options (methods/pmvs/options.h:8-21) and the
  scattered constructor defaults          -> Options
  Patch (methods/pmvs/patch.h:21-101)                -> rows of a PATCH_DTYPE array
  Optimization / OptimizationOpenCV::Optimize,
  FilterByErrorMeasurement (optimization*.h)         -> Engine.refine / Engine.filter
  NCCScore (modules/core/error_measurements.h:11)    -> ncc_score
  PMVS::AddCamera / Run / GetPointCloud (pmvs.h)     -> PMVS
  IO::JSONReader (modules/io/json_reader.h:30-37)    -> read_scene_json
  PMVS::PrintCloud (methods/pmvs/utils.cpp:9-50)     -> write_ply
"""
from __future__ import annotations

import ctypes
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from ._native import FUSED_DTYPE, PATCH_DTYPE, check, lib, ptr

__all__ = [
    "Options",
    "FastOptions",
    "View",
    "Engine",
    "PMVS",
    "ncc_score",
    "read_scene_json",
    "write_ply",
    "write_pfm",
    "check_fuse_args",
    "check_mapref_args",
    "check_tsdf_args",
    "check_mesh_clean_args",
    "check_mesh_colour_args",
    "check_cloud_align_args",
    "check_cloud_nearest_args",
    "check_cloud_transform_args",
    "cloud_compare",
    "check_mesh_nearest_args",
    "mesh_compare",
    "mesh_deviation",
    "check_mesh_decimate_args",
    "check_mesh_render_args",
    "check_mesh_smooth_args",
    "mesh_volume",
    "write_mesh_ply",
    "read_pfm",
    "empty_patches",
    "visible_list",
    "mask_from_list",
]


@dataclass
class FastOptions:
    """Performance-mode knobs (dp_fast_options; no reference counterpart: the
    mode replaces OptimizationOpenCV::Optimize, optimization_opencv.cpp:44-78,
    with a conjugate-gradient refine on LDS-staged gray tiles)."""

    iters: int = 4            # CG iterations: E <= 1 + 3 iters (gradient 1) / 1 + 5 iters (0), +1 filter evaluation
    margin: int = 2           # tile margin around the initial window, pixels (<= 7)
    tile_budget: int = 6656   # LDS bytes per patch: tiles + 64 per view (<= 16384; <= 6656: 4 waves/SIMD)
    max_views: int = 8        # staged views of the refine (<= 32; spec v5, was 32)
    fd_step: float = 0.5      # forward-difference step, scaled units (gradient 0)
    ls_step: float = 1.0      # initial line-search step, scaled units
    densify: int = 0          # 1: dp_densify expands with the fast refine
    gradient: int = 0         # 0: forward differences (spec v3); 1: analytic gradient (spec v4)
    filter_max_views: int = 32  # staged views of the filter / FAST_EVAL scoring (0 = max_views; spec v5)

    def to_c(self) -> N.DpFastOptions:
        o = N.DpFastOptions()
        for name, _ in N.DpFastOptions._fields_:
            setattr(o, name, getattr(self, name))
        return o


@dataclass
class Options:
    """Every hot-path knob with the reference's default (see include/densepoints.h)."""

    seed_cell_size: int = 16        # matcher.h:25
    expand_cell_size: int = 11      # expand.h:12
    grid_scale: int = 8             # patch_organizer.h:43
    max_patches_per_cell: int = 1   # patch_organizer.h:42
    min_visible: int = 3            # optimization.h:17
    min_expand_visible: int = 2     # expand.cpp:67
    nm_max_evals: int = 500         # optimization_opencv.cpp:60
    ncc_threshold: float = 0.6      # optimization.h:16
    visible_angle: float = 0.78     # patch.h:56
    candidate_angle: float = 1.04   # patch.h:57
    nm_step: tuple = (0.02, 0.2, 0.2)  # optimization_opencv.cpp:56
    nm_eps: float = 1e-4            # optimization_opencv.cpp:60
    ncc_denom_min: float = 0.1      # error_measurements.cpp:57
    max_pops: int = 10_000_000      # expand.cpp:95
    # reference PMVS::Options (options.h:10-15): stored, never read by the path
    scale: int = 1
    cell_size: int = 4
    expansions: int = 3

    def to_c(self) -> N.DpOptions:
        o = N.DpOptions()
        for name, _ in N.DpOptions._fields_:
            if name == "reserved0":
                continue
            v = getattr(self, name)
            if name == "nm_step":
                o.nm_step[:] = [float(x) for x in v]
            else:
                setattr(o, name, v)
        return o

    def to_numpy(self) -> np.ndarray:
        """The same POD as bytes (for handing to the oracle's identical layout)."""
        c = self.to_c()
        return np.frombuffer(bytes(c), dtype=np.uint8).copy()


class View:
    """A camera: 3x4 projection (fp64) + BGR8 image (H x W x 3)."""

    def __init__(self, P, image: np.ndarray | None = None, filename: str | None = None):
        self.P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(3, 4))
        self.image = None if image is None else np.ascontiguousarray(image, dtype=np.uint8)
        self.filename = filename
        C = np.zeros(3)
        K = np.zeros(9)
        E = np.zeros(12)
        x = np.zeros(3)
        rc = lib.dp_view_geometry(ptr(self.P), ptr(C), ptr(K), ptr(E), ptr(x))
        if rc != N.DP_OK:
            raise N.DensePointsError(rc, "singular projection matrix")
        self.camera_center = C
        self.intrinsics = K.reshape(3, 3)
        self.extrinsics = E.reshape(3, 4)
        self.x_axis = x

    @property
    def width(self) -> int:
        return int(self.image.shape[1])

    @property
    def height(self) -> int:
        return int(self.image.shape[0])

    def project_point(self, X) -> np.ndarray:
        h = self.P @ np.append(np.asarray(X, dtype=np.float64), 1.0)
        return h[:2] / h[2]

    def is_point_inside(self, X) -> bool:
        u, v = self.project_point(X)
        return bool(0 < u < self.width and 0 < v < self.height)


def empty_patches(n: int) -> np.ndarray:
    return np.zeros(n, dtype=PATCH_DTYPE)


def result_array(addr, n: int, copy: bool = True) -> np.ndarray:
    """n dp_patch records at a library-owned address (a densify's pinned result
    buffer) as a numpy array: a copy, or (copy=False) a view that stays valid
    until the library reuses the buffer"""
    if not n:
        return empty_patches(0)
    buf = (ctypes.c_char * (n * PATCH_DTYPE.itemsize)).from_address(addr)
    view = np.frombuffer(buf, dtype=PATCH_DTYPE, count=n)
    return view.copy() if copy else view


def visible_list(mask) -> list[int]:
    """Bitmask (u64[2]) -> ascending view list (Patch::GetTrullyVisibleImages)."""
    out = []
    for w in range(2):
        m = int(mask[w])
        for b in range(64):
            if (m >> b) & 1:
                out.append(64 * w + b)
    return out


def mask_from_list(views) -> np.ndarray:
    m = np.zeros(2, dtype=np.uint64)
    for v in views:
        m[v >> 6] |= np.uint64(1) << np.uint64(v & 63)
    return m


class Engine:
    """One GPU context: views resident in HBM, batched patch operators."""

    def __init__(self, options: Options | None = None, device: int = 0):
        self.options = options or Options()
        self._ctx = ctypes.c_void_p()
        copt = self.options.to_c()
        rc = lib.dp_ctx_create(ctypes.byref(copt), device, ctypes.byref(self._ctx))
        check(rc)
        self.views: list[View] = []
        self._keep = []
        self._V = 0      # views set (either form)
        self._level = 0  # current pyramid level

    @property
    def handle(self):
        return self._ctx

    def close(self):
        if self._ctx:
            lib.dp_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        check(rc, self._ctx)

    def set_options(self, options: Options):
        self.options = options
        copt = options.to_c()
        self._check(lib.dp_set_options(self._ctx, ctypes.byref(copt)))

    def set_views(self, views: list[View]):
        V = len(views)
        P = np.ascontiguousarray(np.stack([v.P for v in views]).reshape(V, 12))
        imgs = (N.DpImage * V)()
        for i, v in enumerate(views):
            im = v.image
            imgs[i].width = im.shape[1]
            imgs[i].height = im.shape[0]
            imgs[i].stride = im.strides[0]
            imgs[i].bgr = im.ctypes.data
        self._check(lib.dp_set_views(self._ctx, V, ptr(P), imgs))
        self.views = list(views)
        self._V, self._level = V, 0

    def set_views_device(self, P: np.ndarray, widths, heights, pitches, dev_ptrs):
        V = len(dev_ptrs)
        P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(V, 12))
        w = np.asarray(widths, dtype=np.int32)
        h = np.asarray(heights, dtype=np.int32)
        pt = np.asarray(pitches, dtype=np.int32)
        arr = (ctypes.c_void_p * V)(*[int(p) for p in dev_ptrs])
        self._check(lib.dp_set_views_device(self._ctx, V, ptr(P), ptr(w), ptr(h), ptr(pt), arr))
        self._keep = [P, w, h, pt, arr]
        self._V, self._level = V, 0

    # ---- image pyramid (include/densepoints.h dp_build_pyramid / dp_set_level) ----
    def build_pyramid(self, levels: int):
        """Levels 1..levels-1 by cv::pyrDown on the device (level 0 = the views)."""
        self._check(lib.dp_build_pyramid(self._ctx, int(levels)))
        self._level = 0

    def set_level(self, level: int):
        """Run the patch loop on pyramid level `level` (P rows 0-1 scaled by 2^-level)."""
        self._check(lib.dp_set_level(self._ctx, int(level)))
        self._level = int(level)

    def level_info(self, level: int, view: int):
        w, h, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_void_p()
        self._check(lib.dp_level_info(self._ctx, level, view, ctypes.byref(w), ctypes.byref(h), ctypes.byref(d)))
        return w.value, h.value, d.value

    def read_level(self, level: int, view: int) -> np.ndarray:
        w, h, _ = self.level_info(level, view)
        out = np.zeros((h, w, 3), dtype=np.uint8)
        self._check(lib.dp_read_level(self._ctx, level, view, ptr(out)))
        return out

    # ---- PMVS-style filter (include/densepoints.h dp_filter_patches) ----
    def filter_patches(self, patches: np.ndarray, passes: int = 3, min_neighbor_frac: float = 0.25) -> np.ndarray:
        """Visibility-consistency + neighbourhood filter (PMVS::FilterPatches,
        pmvs.h:27, which the reference leaves undefined); returns keep flags."""
        patches = np.ascontiguousarray(patches)
        assert patches.dtype == PATCH_DTYPE
        fo = N.DpFilterOptions(passes, 0, min_neighbor_frac)
        keep = np.zeros(len(patches), dtype=np.uint8)
        self._check(lib.dp_filter_patches(self._ctx, ptr(patches), len(patches), ctypes.byref(fo), ptr(keep)))
        return keep

    def seeds_to_patches(self, xyz: np.ndarray) -> np.ndarray:
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = empty_patches(len(xyz))
        self._check(lib.dp_seeds_to_patches(self._ctx, ptr(xyz), len(xyz), ptr(out)))
        return out

    def refine(self, patches: np.ndarray, cell: int, mode: int) -> np.ndarray:
        """Fused evaluate+refine+filter over a batch, in place; returns accept flags."""
        assert patches.dtype == PATCH_DTYPE and patches.flags.c_contiguous
        acc = np.zeros(len(patches), dtype=np.uint8)
        self._check(lib.dp_refine_batch(self._ctx, ptr(patches), len(patches), cell, mode, ptr(acc)))
        return acc

    def refine_device(self, d_patches: int, n: int, cell: int, mode: int, d_accept: int | None,
                      stream: int | None = None):
        self._check(lib.dp_refine_batch_device(self._ctx, ctypes.c_void_p(d_patches), n, cell, mode,
                                               ctypes.c_void_p(d_accept) if d_accept else None,
                                               ctypes.c_void_p(stream) if stream else None))

    def expand(self, parents: np.ndarray):
        """Expand::ExpandPatch over a batch: returns (children[4n], accept[4n])."""
        parents = np.ascontiguousarray(parents)
        assert parents.dtype == PATCH_DTYPE
        kids = empty_patches(4 * len(parents))
        acc = np.zeros(4 * len(parents), dtype=np.uint8)
        self._check(lib.dp_expand_batch(self._ctx, ptr(parents), len(parents), ptr(kids), ptr(acc)))
        return kids, acc

    def expand_device(self, d_parents: int, n: int, d_children: int, d_accept: int | None,
                      stream: int | None = None):
        self._check(lib.dp_expand_batch_device(self._ctx, ctypes.c_void_p(d_parents), n,
                                               ctypes.c_void_p(d_children),
                                               ctypes.c_void_p(d_accept) if d_accept else None,
                                               ctypes.c_void_p(stream) if stream else None))

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_double()
        self._check(lib.dp_last_kernel_ms(self._ctx, ctypes.byref(ms)))
        return ms.value

    # ---- performance mode (include/densepoints.h dp_fast_options) ----
    def set_fast_options(self, fo: FastOptions):
        c = fo.to_c()
        self._check(lib.dp_set_fast_options(self._ctx, ctypes.byref(c)))

    def build_gray(self):
        """fp16 gray planes of the current level (built on demand otherwise)."""
        self._check(lib.dp_build_gray(self._ctx))

    def read_gray(self, view: int) -> np.ndarray:
        vw = self.views[view] if self.views else None
        w, h, _ = self.level_info(0, view) if vw is None else (vw.width, vw.height, 0)
        out = np.zeros((h, w), dtype=np.float16)
        self._check(lib.dp_read_gray(self._ctx, view, ptr(out)))
        return out

    def probe_akaze_plane(self, view: int, level: int, which: int) -> np.ndarray:
        """One fp32 plane (0 Lt, 1 Lx, 2 Ly, 3 Ldet) of the AKAZE scale space
        seed generation builds of the views set (dp_probe_akaze_plane)."""
        wh = np.zeros(2, dtype=np.int32)
        self._check(lib.dp_probe_akaze_plane(self._ctx, view, level, which, None, 0, ptr(wh)))
        out = np.zeros((int(wh[1]), int(wh[0])), dtype=np.float32)
        self._check(lib.dp_probe_akaze_plane(self._ctx, view, level, which, ptr(out), out.size, ptr(wh)))
        return out

    def probe_orb_level(self, view: int, level: int, n_levels: int, scale_factor: float = 1.2) -> np.ndarray:
        """One u8 level of the gray pyramid ORB detection builds (dp_probe_orb_level)."""
        wh = np.zeros(2, dtype=np.int32)
        self._check(lib.dp_probe_orb_level(self._ctx, view, level, n_levels, scale_factor, None, 0, ptr(wh)))
        out = np.zeros((int(wh[1]), int(wh[0])), dtype=np.uint8)
        self._check(lib.dp_probe_orb_level(self._ctx, view, level, n_levels, scale_factor, ptr(out), out.size,
                                           ptr(wh)))
        return out

    def fast_refine(self, patches: np.ndarray, cell: int, mode: int = N.MODE_FAST_REFINE) -> np.ndarray:
        """Performance-mode refine (or one fast evaluation) in place; accept flags."""
        return self.refine(patches, cell, mode)

    def fast_expand(self, parents: np.ndarray):
        """Expand::ExpandPatch children refined in performance mode."""
        parents = np.ascontiguousarray(parents)
        assert parents.dtype == PATCH_DTYPE
        kids = empty_patches(4 * len(parents))
        acc = np.zeros(4 * len(parents), dtype=np.uint8)
        self._check(lib.dp_fast_expand_batch(self._ctx, ptr(parents), len(parents), ptr(kids), ptr(acc)))
        return kids, acc

    def fast_expand_device(self, d_parents: int, n: int, d_children: int, d_accept: int | None,
                           stream: int | None = None):
        self._check(lib.dp_fast_expand_batch_device(self._ctx, ctypes.c_void_p(d_parents), n,
                                                    ctypes.c_void_p(d_children),
                                                    ctypes.c_void_p(d_accept) if d_accept else None,
                                                    ctypes.c_void_p(stream) if stream else None))

    def fast_last_stats(self) -> dict:
        st = N.DpFastStats()
        self._check(lib.dp_fast_last_stats(self._ctx, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in N.DpFastStats._fields_}

    def evaluate(self, patches: np.ndarray, cell: int) -> np.ndarray:
        out = np.zeros(len(patches), dtype=np.float32)
        self._check(lib.dp_eval_batch(self._ctx, ptr(patches), len(patches), cell, ptr(out)))
        return out

    def optimize(self, patches: np.ndarray, cell: int) -> np.ndarray:
        """OptimizationOpenCV::Optimize over a batch (always accepts)."""
        return self.refine(patches, cell, N.MODE_NM)

    def filter(self, patches: np.ndarray, cell: int) -> np.ndarray:
        """Optimization::FilterByErrorMeasurement over a batch."""
        return self.refine(patches, cell, N.MODE_FILTER)

    def densify(self, seeds_xyz: np.ndarray, copy: bool = True):
        """dp_densify: (patches, stats).  copy=False returns a view of the
        library's pinned result buffer instead of a copy -- valid until the next
        densify on this engine, the C ABI's own contract for *out
        (include/densepoints.h dp_densify)."""
        seeds = np.ascontiguousarray(seeds_xyz, dtype=np.float64).reshape(-1, 3)
        out = ctypes.c_void_p()
        n = ctypes.c_int64()
        st = N.DpDensifyStats()
        self._check(lib.dp_densify(self._ctx, ptr(seeds), len(seeds), ctypes.byref(out), ctypes.byref(n),
                                   ctypes.byref(st)))
        stats = {name: getattr(st, name) for name, _ in N.DpDensifyStats._fields_}
        return result_array(out.value, n.value, copy), stats

    # ---- one generation at a time (multi-GPU partitioning; dist.py) ----
    def densify_begin(self, seeds_xyz: np.ndarray) -> N.DpGeneration:
        seeds = np.ascontiguousarray(seeds_xyz, dtype=np.float64).reshape(-1, 3)
        g = N.DpGeneration()
        self._check(lib.dp_densify_begin(self._ctx, ptr(seeds), len(seeds), ctypes.byref(g)))
        return g

    def densify_commit(self, gen: N.DpGeneration, cand: np.ndarray, acc: np.ndarray) -> N.DpGeneration:
        cand = np.ascontiguousarray(cand, dtype=PATCH_DTYPE)
        acc = np.ascontiguousarray(acc, dtype=np.uint8)
        self._check(lib.dp_densify_commit(self._ctx, ctypes.byref(gen), ptr(cand), ptr(acc), len(cand)))
        return gen

    def densify_run(self, gen: N.DpGeneration, max_generations: int = 1 << 30) -> N.DpGeneration:
        """Up to max_generations expansion generations device-resident on this
        context (dp_densify_run: 8 per host wait)."""
        self._check(lib.dp_densify_run(self._ctx, ctypes.byref(gen), int(min(max_generations, 2**31 - 1))))
        return gen

    def densify_run_until(self, gen: N.DpGeneration, yield_items: int, max_generations: int = 1 << 30):
        """dp_densify_run_until: device-resident generations until the densify
        ends or the next generation has >= yield_items items (returned unrun);
        (gen, objective evaluations this call spent)."""
        ev = ctypes.c_int64()
        self._check(lib.dp_densify_run_until(self._ctx, ctypes.byref(gen), int(min(max_generations, 2**31 - 1)),
                                             int(yield_items), ctypes.byref(ev)))
        return gen, int(ev.value)

    # ---- partitioned generations (reference-view super-tiles) ----
    def densify_owners(self, gen: N.DpGeneration, world: int, tile_px: int = 64):
        """(owner rank per item, fallback flag -- always False since the round-4
        partition spec) of the generation: dp_densify_owners."""
        own = np.zeros(gen.items, dtype=np.int32)
        fb = ctypes.c_int32()
        self._check(lib.dp_densify_owners(self._ctx, ctypes.byref(gen), world, tile_px, ptr(own), ctypes.byref(fb)))
        return own, bool(fb.value)

    def densify_partition_stats(self) -> dict:
        """The last partition's {items, world, tiles, split_items}
        (dp_densify_partition_stats): distinct super-tiles, and items in the
        tiles a cut shares between two ranks."""
        st = np.zeros(4, dtype=np.int64)
        self._check(lib.dp_densify_partition_stats(self._ctx, ptr(st)))
        return {"items": int(st[0]), "world": int(st[1]), "tiles": int(st[2]), "split_items": int(st[3])}

    def densify_refine_items(self, gen: N.DpGeneration, items: np.ndarray):
        items = np.ascontiguousarray(items, dtype=np.int64)
        n = len(items) * gen.per_item
        cand = empty_patches(n)
        acc = np.zeros(n, dtype=np.uint8)
        self._check(lib.dp_densify_refine_items(self._ctx, ctypes.byref(gen), ptr(items), len(items), ptr(cand),
                                                ptr(acc)))
        return cand, acc

    # ---- the one-wait device protocol: everything on the caller's stream ----
    def densify_partition_async(self, gen: N.DpGeneration, world: int, tile_px: int = 64,
                                stream: int | None = None):
        """(device address of the rank-major item order, items per rank):
        dp_densify_partition_async -- queued on `stream`, no host wait (the
        shares are floor(r n / world) cuts; the statistics come back with the
        commit)."""
        d_order = ctypes.c_void_p()
        counts = np.zeros(world, dtype=np.int64)
        self._check(lib.dp_densify_partition_async(self._ctx, ctypes.byref(gen), world, tile_px,
                                                   ctypes.c_void_p(stream) if stream else None,
                                                   ctypes.byref(d_order), ptr(counts)))
        return int(d_order.value or 0), counts

    def densify_refine_share_async(self, gen: N.DpGeneration, d_items: int, n: int, d_slot: int, stride: int,
                                   stream: int | None = None) -> None:
        """Refine this rank's n items (device list d_items) and compact the
        accepted candidates into its exchange slot (header + stride records)."""
        self._check(lib.dp_densify_refine_share_async(self._ctx, ctypes.byref(gen), ctypes.c_void_p(d_items), n,
                                                      ctypes.c_void_p(d_slot), stride,
                                                      ctypes.c_void_p(stream) if stream else None))

    def densify_commit_gathered_device(self, gen: N.DpGeneration, d_recs: int, stride: int, world: int,
                                       stream: int | None = None) -> int:
        """Commit from the `world` gathered rank slots at d_recs (stride + 1
        records each); the generation's one host wait.  Returns the records
        exchanged."""
        ex = ctypes.c_int64()
        self._check(lib.dp_densify_commit_gathered_device(self._ctx, ctypes.byref(gen), ctypes.c_void_p(d_recs), stride,
                                                          world, ctypes.c_void_p(stream) if stream else None,
                                                          ctypes.byref(ex)))
        return int(ex.value)

    def densify_result(self, copy: bool = True):
        """dp_densify_result: (patches, stats); copy=False as in densify()."""
        out = ctypes.c_void_p()
        n = ctypes.c_int64()
        st = N.DpDensifyStats()
        self._check(lib.dp_densify_result(self._ctx, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        stats = {name: getattr(st, name) for name, _ in N.DpDensifyStats._fields_}
        return result_array(out.value, n.value, copy), stats


    # ---- resume / iterated expand-filter (include/densepoints.h dp_densify_resume) ----
    def densify_resume(self, patches: np.ndarray, keep: np.ndarray | None = None) -> N.DpGeneration:
        """dp_densify_resume: the organizer and the store rebuilt from
        patches[keep != 0] (TryInsert in index order, no refine); returns the
        first expansion generation, for densify_run and the generation API."""
        patches = np.ascontiguousarray(patches)
        assert patches.dtype == PATCH_DTYPE
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if len(keep) != len(patches):
                raise ValueError("densify_resume: one keep flag per patch")
        g = N.DpGeneration()
        self._check(lib.dp_densify_resume(self._ctx, ptr(patches), len(patches), ptr(keep), ctypes.byref(g)))
        return g

    def densify_resume_device(self, d_patches: int, n: int, d_keep: int | None,
                              stream: int | None = None) -> N.DpGeneration:
        """dp_densify_resume_device: the same from device memory (d_patches may
        be the context's own store, densify_store_device()); one host wait."""
        g = N.DpGeneration()
        self._check(lib.dp_densify_resume_device(self._ctx, ctypes.c_void_p(d_patches) if d_patches else None, int(n),
                                                 ctypes.c_void_p(d_keep) if d_keep else None, ctypes.byref(g),
                                                 ctypes.c_void_p(stream) if stream else None))
        return g

    def densify_store_device(self) -> tuple[int, int]:
        """(device address, records) of the context's patch store."""
        d = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._check(lib.dp_densify_store_device(self._ctx, ctypes.byref(d), ctypes.byref(n)))
        return int(d.value or 0), int(n.value)

    def filter_patches_device(self, d_patches: int, n: int, d_keep: int, passes: int = 3,
                              min_neighbor_frac: float = 0.25, stream: int | None = None) -> None:
        """dp_filter_patches_device: keep flags of n device-resident patches, queued on `stream`."""
        fo = N.DpFilterOptions(passes, 0, min_neighbor_frac)
        self._check(lib.dp_filter_patches_device(self._ctx, ctypes.c_void_p(d_patches) if d_patches else None, int(n),
                                                 ctypes.byref(fo), ctypes.c_void_p(d_keep) if d_keep else None,
                                                 ctypes.c_void_p(stream) if stream else None))

    def densify_iterate(self, seeds_xyz: np.ndarray, iterations: int, passes: int = 3,
                        min_neighbor_frac: float = 0.25, copy: bool = True):
        """dp_densify_iterate: `iterations` rounds of expansion then filter, the
        store resident on the device between them; (surviving patches, stats)
        with the per-round records in stats["iterations"]."""
        seeds = np.ascontiguousarray(seeds_xyz, dtype=np.float64).reshape(-1, 3)
        fo = N.DpFilterOptions(passes, 0, min_neighbor_frac)
        out = ctypes.c_void_p()
        n = ctypes.c_int64()
        st = N.DpDensifyStats()
        per = (N.DpIterateStats * max(int(iterations), 1))()
        self._check(lib.dp_densify_iterate(self._ctx, ptr(seeds), len(seeds), int(iterations), ctypes.byref(fo),
                                           ctypes.byref(out), ctypes.byref(n), ctypes.byref(st), per))
        stats = {name: getattr(st, name) for name, _ in N.DpDensifyStats._fields_}
        stats["iterations"] = [{name: getattr(per[k], name) for name, _ in N.DpIterateStats._fields_
                                if name != "reserved"} for k in range(int(iterations))]
        return result_array(out.value, n.value, copy), stats

    # ---- per-view maps (include/densepoints.h dp_render_maps) ----
    def view_sizes(self, views=None) -> list[tuple[int, int]]:
        """(width, height) of views at the current pyramid level."""
        V = self.num_views()
        return [self.level_info(self._level, v)[:2] for v in (range(V) if views is None else views)]

    def num_views(self) -> int:
        return self._V

    def render_maps(self, patches: np.ndarray, views=None, keep: np.ndarray | None = None, splat_scale: float = 1.0,
                    max_radius_px: int = 32, all_facing: bool = False, normals: bool = False,
                    scores: bool = False) -> dict:
        """dp_render_maps: every patch splatted as an oriented disc of radius
        splat_scale * rho(p) into `views` (None = all) at the current level,
        nearest disc per pixel.  Returns {"views", "depth" (f32, 0 = empty),
        "index" (int32, -1 = empty), "normal" / "score" when asked for, "stats"},
        each map a list of H x W (x 3) arrays in the order of "views"."""
        patches = np.ascontiguousarray(patches)
        assert patches.dtype == PATCH_DTYPE
        ro, vid, keep = check_render_args(len(patches), self.num_views(), views, keep, splat_scale, max_radius_px,
                                          all_facing)
        sizes = self.view_sizes(vid)
        out = {"views": [int(v) for v in vid],
               "depth": [np.zeros((h, w), np.float32) for w, h in sizes],
               "index": [np.zeros((h, w), np.int32) for w, h in sizes]}
        if normals:
            out["normal"] = [np.zeros((h, w, 3), np.float32) for w, h in sizes]
        if scores:
            out["score"] = [np.zeros((h, w), np.float32) for w, h in sizes]

        def table(key):
            return (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in out[key]]) if key in out else None

        st = N.DpRenderStats()
        self._check(lib.dp_render_maps(self._ctx, ptr(patches), len(patches), ptr(keep), ptr(vid), len(vid),
                                       ctypes.byref(ro), table("depth"), table("index"), table("normal"),
                                       table("score"), ctypes.byref(st)))
        out["stats"] = {name: getattr(st, name) for name, _ in N.DpRenderStats._fields_}
        return out

    def render_maps_device(self, d_patches: int, n: int, d_keep: int | None, views, d_depth=None, d_index=None,
                           d_normal=None, d_score=None, splat_scale: float = 1.0, max_radius_px: int = 32,
                           all_facing: bool = False, stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_render_maps_device: n device-resident patches (the context's own
        store included) and optional device keep flags into device planes --
        d_depth / d_index / d_normal / d_score are lists of device addresses, one
        per entry of `views` (None or 0 = not wanted).  Queued on `stream`;
        waits only for the statistics (stats=False: no wait, returns None)."""
        ro, vid, _ = check_render_args(int(n), self.num_views(), views, None, splat_scale, max_radius_px, all_facing)

        def table(addrs):
            if addrs is None:
                return None
            if len(addrs) != len(vid):
                raise ValueError("render_maps_device: one plane address per view")
            return (ctypes.c_void_p * len(vid))(*[int(a) if a else None for a in addrs])

        st = N.DpRenderStats()
        self._check(lib.dp_render_maps_device(self._ctx, ctypes.c_void_p(d_patches) if d_patches else None, int(n),
                                              ctypes.c_void_p(d_keep) if d_keep else None, ptr(vid), len(vid),
                                              ctypes.byref(ro), table(d_depth), table(d_index), table(d_normal),
                                              table(d_score), ctypes.byref(st) if stats else None,
                                              ctypes.c_void_p(stream) if stream else None))
        return {name: getattr(st, name) for name, _ in N.DpRenderStats._fields_} if stats else None

    # ---- depth-map fusion (include/densepoints.h dp_fuse_maps) ----
    def fuse_maps(self, depth, normal=None, views=None, depth_tol: float = 0.01, min_views: int = 2,
                  min_normal_cos: float = 0.5, suppress: bool = True):
        """dp_fuse_maps: the depth (and normal) planes of `views` (None = all),
        as render_maps returns them, fused into one cross-view-consistent cloud.
        Returns (points as a FUSED_DTYPE array in (view rank, y, x) order, stats)."""
        fo, vid = check_fuse_args(self.num_views(), views, depth_tol, min_views, min_normal_cos, suppress)
        sizes = self.view_sizes(vid)

        def planes(arrs, name, tail):
            if len(arrs) != len(vid):
                raise ValueError("fuse_maps: one %s plane per view" % name)
            out = [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
            for a, (w, h) in zip(out, sizes):
                if a.shape != (h, w) + tail:
                    raise ValueError("fuse_maps: a %s plane of shape %s, expected %s" % (name, a.shape, (h, w) + tail))
            return out, (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in out])

        depth, dtab = planes(depth, "depth", ())
        normal, ntab = planes(normal, "normal", (3,)) if normal is not None else (None, None)
        out, n, st = ctypes.c_void_p(), ctypes.c_int64(), N.DpFuseStats()
        self._check(lib.dp_fuse_maps(self._ctx, ptr(vid), len(vid), ctypes.byref(fo), dtab, ntab, ctypes.byref(out),
                                     ctypes.byref(n), ctypes.byref(st)))
        pts = np.zeros(n.value, dtype=FUSED_DTYPE)
        if n.value:
            ctypes.memmove(pts.ctypes.data, out.value, pts.nbytes)
        return pts, {name: getattr(st, name) for name, _ in N.DpFuseStats._fields_}

    def fuse_maps_device(self, views, d_depth, d_normal, d_points: int | None, cap: int, depth_tol: float = 0.01,
                         min_views: int = 2, min_normal_cos: float = 0.5, suppress: bool = True,
                         stream: int | None = None):
        """dp_fuse_maps_device: device planes (lists of device addresses, one per
        entry of `views`; d_normal None = no normals) into at most `cap`
        dp_fused_point records at d_points.  Queued on `stream`; one wait.
        Returns (the full emitted count -- above cap: an overflow --, stats)."""
        fo, vid = check_fuse_args(self.num_views(), views, depth_tol, min_views, min_normal_cos, suppress)
        if int(cap) != cap or cap < 0 or (cap > 0 and not d_points):
            raise ValueError("fuse_maps_device: cap must be >= 0, with d_points given when > 0")

        def table(addrs):
            if addrs is None:
                return None
            if len(addrs) != len(vid) or not all(addrs):
                raise ValueError("fuse_maps_device: one plane address per view")
            return (ctypes.c_void_p * len(vid))(*[int(a) for a in addrs])

        if d_depth is None:
            raise ValueError("fuse_maps_device: depth planes must be given")
        n, st = ctypes.c_int64(), N.DpFuseStats()
        self._check(lib.dp_fuse_maps_device(self._ctx, ptr(vid), len(vid), ctypes.byref(fo), table(d_depth),
                                            table(d_normal), ctypes.c_void_p(d_points) if d_points else None,
                                            int(cap), ctypes.byref(n), ctypes.byref(st),
                                            ctypes.c_void_p(stream) if stream else None))
        return int(n.value), {name: getattr(st, name) for name, _ in N.DpFuseStats._fields_}


    # ---- depth-map refinement (include/densepoints.h dp_refine_maps) ----
    def refine_maps(self, depth, normal, views=None, sources=None, **options) -> dict:
        """dp_refine_maps: one Jacobi pass over the depth and normal planes of
        `views` (None = all), as render_maps returns them.  `sources`: per view a
        list of source view ids (None = the nearest max_sources requested
        views); options: the fields of dp_mapref_options (window, sweep, step_px,
        reach, max_sources, top_k, min_ncc, keep_unscored).  Returns {"views",
        "depth", "normal", "score", "choice" (lists of planes), "stats"}."""
        mo, vid, src = check_mapref_args(self.num_views(), views, sources, **options)
        sizes = self.view_sizes(vid)

        def planes(arrs, name, tail):
            if arrs is None or len(arrs) != len(vid):
                raise ValueError("refine_maps: one %s plane per view" % name)
            out = [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
            for a, (w, h) in zip(out, sizes):
                if a.shape != (h, w) + tail:
                    raise ValueError("refine_maps: a %s plane of shape %s, expected %s" % (name, a.shape, (h, w) + tail))
            return out, (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in out])

        depth, dtab = planes(depth, "depth", ())
        normal, ntab = planes(normal, "normal", (3,))
        out = {"views": [int(v) for v in vid],
               "depth": [np.zeros((h, w), np.float32) for w, h in sizes],
               "normal": [np.zeros((h, w, 3), np.float32) for w, h in sizes],
               "score": [np.zeros((h, w), np.float32) for w, h in sizes],
               "choice": [np.zeros((h, w), np.int32) for w, h in sizes]}

        def table(key):
            return (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in out[key]])

        st = N.DpMaprefStats()
        self._check(lib.dp_refine_maps(self._ctx, ptr(vid), len(vid), ctypes.byref(mo), ptr(src), dtab, ntab,
                                       table("depth"), table("normal"), table("score"), table("choice"),
                                       ctypes.byref(st)))
        out["stats"] = {name: getattr(st, name) for name, _ in N.DpMaprefStats._fields_}
        return out

    def refine_maps_device(self, views, d_depth, d_normal, d_depth_out=None, d_normal_out=None, d_score_out=None,
                           d_choice_out=None, sources=None, stream: int | None = None, stats: bool = True,
                           **options) -> dict | None:
        """dp_refine_maps_device: device planes (lists of device addresses, one
        per entry of `views`; an output list or entry None or 0 = not wanted).
        Queued on `stream`; waits only for the statistics (stats=False: no wait,
        returns None)."""
        mo, vid, src = check_mapref_args(self.num_views(), views, sources, **options)

        def table(addrs, required):
            if addrs is None:
                if required:
                    raise ValueError("refine_maps_device: depth and normal planes must be given")
                return None
            if len(addrs) != len(vid) or (required and not all(addrs)):
                raise ValueError("refine_maps_device: one plane address per view")
            return (ctypes.c_void_p * len(vid))(*[int(a) if a else None for a in addrs])

        ins = [int(a) for a in list(d_depth or []) + list(d_normal or []) if a]
        for outs in (d_depth_out, d_normal_out, d_score_out, d_choice_out):
            if outs is not None and any(a and int(a) in ins for a in outs):
                raise ValueError("refine_maps_device: an output plane is an input plane")
        st = N.DpMaprefStats()
        self._check(lib.dp_refine_maps_device(self._ctx, ptr(vid), len(vid), ctypes.byref(mo), ptr(src),
                                              table(d_depth, True), table(d_normal, True), table(d_depth_out, False),
                                              table(d_normal_out, False), table(d_score_out, False),
                                              table(d_choice_out, False), ctypes.byref(st) if stats else None,
                                              ctypes.c_void_p(stream) if stream else None))
        return {name: getattr(st, name) for name, _ in N.DpMaprefStats._fields_} if stats else None

    # ---- TSDF volume and mesh (include/densepoints.h dp_tsdf_integrate / dp_tsdf_mesh) ----
    def tsdf_integrate(self, depth, views=None, *, origin, voxel, dim, trunc) -> dict:
        """dp_tsdf_integrate: the depth planes of `views` (None = all), as
        render_maps or refine_maps return them, integrated into one dense volume
        of dim = (nx, ny, nz) voxels of side `voxel` with its low corner at
        `origin`.  Returns {"tsdf" f32, "weight" int32, "rgb" uint32 (R | G << 8 |
        B << 16), each [nz][ny][nx], "origin", "voxel", "dim", "trunc" (the volume,
        as tsdf_mesh reads it), "views", "stats"}."""
        to, vid = check_tsdf_args(self.num_views(), views, origin, voxel, dim, trunc)
        sizes = self.view_sizes(vid)
        if depth is None or len(depth) != len(vid):
            raise ValueError("tsdf_integrate: one depth plane per view")
        planes = [np.ascontiguousarray(a, dtype=np.float32) for a in depth]
        for a, (w, h) in zip(planes, sizes):
            if a.shape != (h, w):
                raise ValueError("tsdf_integrate: a depth plane of shape %s, expected %s" % (a.shape, (h, w)))
        dtab = (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in planes])
        shape = (to.dim[2], to.dim[1], to.dim[0])
        out = {"tsdf": np.zeros(shape, np.float32), "weight": np.zeros(shape, np.int32),
               "rgb": np.zeros(shape, np.uint32)}
        st = N.DpTsdfStats()
        self._check(lib.dp_tsdf_integrate(self._ctx, ptr(vid), len(vid), ctypes.byref(to), dtab, ptr(out["tsdf"]),
                                          ptr(out["weight"]), ptr(out["rgb"]), ctypes.byref(st)))
        out.update(origin=tuple(to.origin), voxel=to.voxel, dim=tuple(to.dim), trunc=to.trunc,
                   views=[int(v) for v in vid],
                   stats={name: getattr(st, name) for name, _ in N.DpTsdfStats._fields_})
        return out

    def tsdf_integrate_device(self, views, d_depth, d_tsdf, d_weight, d_rgb, *, origin, voxel, dim, trunc,
                              stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_tsdf_integrate_device: device depth planes (a list of device
        addresses, one per entry of `views`) into device volumes (addresses;
        None or 0 = not wanted).  Queued on `stream`; waits only for the
        statistics (stats=False: no wait, returns None)."""
        to, vid = check_tsdf_args(self.num_views(), views, origin, voxel, dim, trunc)
        if d_depth is None or len(d_depth) != len(vid) or not all(d_depth):
            raise ValueError("tsdf_integrate_device: one depth plane address per view")
        dtab = (ctypes.c_void_p * len(vid))(*[int(a) for a in d_depth])
        st = N.DpTsdfStats()
        self._check(lib.dp_tsdf_integrate_device(self._ctx, ptr(vid), len(vid), ctypes.byref(to), dtab,
                                                 ctypes.c_void_p(d_tsdf) if d_tsdf else None,
                                                 ctypes.c_void_p(d_weight) if d_weight else None,
                                                 ctypes.c_void_p(d_rgb) if d_rgb else None,
                                                 ctypes.byref(st) if stats else None,
                                                 ctypes.c_void_p(stream) if stream else None))
        return {name: getattr(st, name) for name, _ in N.DpTsdfStats._fields_} if stats else None

    def tsdf_mesh(self, volume: dict, min_weight: int = 1):
        """dp_tsdf_mesh: the zero surface of a volume as tsdf_integrate returns it
        ("rgb" may be missing or None: vertex colour 0), by marching tetrahedra
        over the cells whose eight corners have weight >= min_weight.  Returns
        (vertices as a MESH_VERTEX_DTYPE array, triangles as n x 3 int32, stats)."""
        to, _ = check_tsdf_args(1, None, volume["origin"], volume["voxel"], volume["dim"], volume["trunc"], min_weight)
        shape = (to.dim[2], to.dim[1], to.dim[0])

        def plane(key, dtype):
            a = np.ascontiguousarray(volume[key], dtype=dtype)
            if a.shape != shape:
                raise ValueError("tsdf_mesh: a %s volume of shape %s, expected %s" % (key, a.shape, shape))
            return a

        tsdf, weight = plane("tsdf", np.float32), plane("weight", np.int32)
        rgb = plane("rgb", np.uint32) if volume.get("rgb") is not None else None
        pv, pt, nv, nt, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), N.DpMeshStats()
        self._check(lib.dp_tsdf_mesh(self._ctx, ctypes.byref(to), ptr(tsdf), ptr(weight), ptr(rgb), ctypes.byref(pv),
                                     ctypes.byref(nv), ctypes.byref(pt), ctypes.byref(nt), ctypes.byref(st)))
        verts = np.zeros(nv.value, dtype=N.MESH_VERTEX_DTYPE)
        tris = np.zeros((nt.value, 3), dtype=np.int32)
        if nv.value:
            ctypes.memmove(verts.ctypes.data, pv.value, verts.nbytes)
        if nt.value:
            ctypes.memmove(tris.ctypes.data, pt.value, tris.nbytes)
        return verts, tris, {name: getattr(st, name) for name, _ in N.DpMeshStats._fields_}

    def tsdf_mesh_device(self, d_tsdf, d_weight, d_rgb, d_vertices, vertex_cap: int, d_triangles, triangle_cap: int,
                         *, origin, voxel, dim, trunc, min_weight: int = 1, stream: int | None = None):
        """dp_tsdf_mesh_device: device volumes (addresses; d_rgb None or 0 = vertex
        colour 0) into at most vertex_cap dp_mesh_vertex records at d_vertices and
        triangle_cap int32 triples at d_triangles.  Queued on `stream`; one wait.
        Returns (the full vertex count, the full triangle count -- above a cap:
        an overflow --, stats)."""
        to, _ = check_tsdf_args(1, None, origin, voxel, dim, trunc, min_weight)
        if not d_tsdf or not d_weight:
            raise ValueError("tsdf_mesh_device: the tsdf and weight volumes must be given")
        for cap, buf in ((vertex_cap, d_vertices), (triangle_cap, d_triangles)):
            if int(cap) != cap or cap < 0 or (cap > 0 and not buf):
                raise ValueError("tsdf_mesh_device: a cap must be >= 0, with its buffer given when > 0")
        nv, nt, st = ctypes.c_int64(), ctypes.c_int64(), N.DpMeshStats()
        self._check(lib.dp_tsdf_mesh_device(self._ctx, ctypes.byref(to), ctypes.c_void_p(d_tsdf),
                                            ctypes.c_void_p(d_weight), ctypes.c_void_p(d_rgb) if d_rgb else None,
                                            ctypes.c_void_p(d_vertices) if d_vertices else None, int(vertex_cap),
                                            ctypes.byref(nv), ctypes.c_void_p(d_triangles) if d_triangles else None,
                                            int(triangle_cap), ctypes.byref(nt), ctypes.byref(st),
                                            ctypes.c_void_p(stream) if stream else None))
        return int(nv.value), int(nt.value), {name: getattr(st, name) for name, _ in N.DpMeshStats._fields_}

    # ---- mesh clean-up (include/densepoints.h dp_mesh_components / dp_mesh_clean) ----
    def mesh_components(self, triangles, n_vertices: int) -> dict:
        """dp_mesh_components: the connected components (by shared vertices) of
        `triangles` (n x 3 int32) over n_vertices vertices.  Returns
        {"vertex_component" int32 (-1: unused), "triangle_component" int32 (-1:
        invalid), "components" as a MESH_COMPONENT_DTYPE array in ascending root
        order, "stats"}."""
        tris = _mesh_triangles("mesh_components", triangles)
        nv = _mesh_count("mesh_components", n_vertices)
        vc, tc = np.full(nv, -1, np.int32), np.full(len(tris), -1, np.int32)
        pc, nc, st = ctypes.c_void_p(), ctypes.c_int64(), N.DpMeshCleanStats()
        self._check(lib.dp_mesh_components(self._ctx, ptr(tris) if len(tris) else None, len(tris), nv,
                                           ptr(vc) if nv else None, ptr(tc) if len(tris) else None, ctypes.byref(pc),
                                           ctypes.byref(nc), ctypes.byref(st)))
        comps = np.zeros(nc.value, dtype=N.MESH_COMPONENT_DTYPE)
        if nc.value:
            ctypes.memmove(comps.ctypes.data, pc.value, comps.nbytes)
        return dict(vertex_component=vc, triangle_component=tc, components=comps, stats=_mesh_clean_stats(st))

    def mesh_components_device(self, d_triangles, n_triangles: int, n_vertices: int, d_vertex_component=None,
                               d_triangle_component=None, d_components=None, component_cap: int = 0,
                               stream: int | None = None):
        """dp_mesh_components_device: device triangles (an address) into the
        device arrays given (addresses, None = not wanted) and at most
        component_cap table rows at d_components.  Queued on `stream`; one wait.
        Returns (the full component count, stats)."""
        nt, nv = _mesh_count("mesh_components_device", n_triangles), _mesh_count("mesh_components_device", n_vertices)
        _mesh_cap("mesh_components_device", component_cap, d_components)
        if nt and not d_triangles:
            raise ValueError("mesh_components_device: the triangles must be given")
        nc, st = ctypes.c_int64(), N.DpMeshCleanStats()
        self._check(lib.dp_mesh_components_device(self._ctx, _addr(d_triangles), nt, nv, _addr(d_vertex_component),
                                                  _addr(d_triangle_component), _addr(d_components), int(component_cap),
                                                  ctypes.byref(nc), ctypes.byref(st), _addr(stream)))
        return int(nc.value), _mesh_clean_stats(st)

    def mesh_clean(self, vertices, triangles, min_triangles: int = 1, min_fraction: float = 0.0,
                   max_components: int = 0, maps: bool = False):
        """dp_mesh_clean: the mesh without its small components -- those of fewer
        than min_triangles triangles, of less than min_fraction of the largest
        component's triangles, or (max_components > 0) not among the first
        max_components by triangle count.  Returns (vertices, triangles, stats),
        and with maps=True also (vertex_map, triangle_map): the new index of every
        input vertex and triangle, or -1."""
        mco = check_mesh_clean_args(min_triangles, min_fraction, max_components)
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_clean", triangles)
        nv, nt = len(verts), len(tris)
        vm = np.full(nv, -1, np.int32) if maps else None
        tm = np.full(nt, -1, np.int32) if maps else None
        pv, pt, no, to, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), N.DpMeshCleanStats()
        self._check(lib.dp_mesh_clean(self._ctx, ctypes.byref(mco), ptr(verts) if nv else None, nv,
                                      ptr(tris) if nt else None, nt, ctypes.byref(pv), ctypes.byref(no),
                                      ctypes.byref(pt), ctypes.byref(to), ptr(vm) if maps and nv else None,
                                      ptr(tm) if maps and nt else None, ctypes.byref(st)))
        vout = np.zeros(no.value, dtype=N.MESH_VERTEX_DTYPE)
        tout = np.zeros((to.value, 3), dtype=np.int32)
        if no.value:
            ctypes.memmove(vout.ctypes.data, pv.value, vout.nbytes)
        if to.value:
            ctypes.memmove(tout.ctypes.data, pt.value, tout.nbytes)
        out = (vout, tout, _mesh_clean_stats(st))
        return out + (vm, tm) if maps else out

    def mesh_clean_device(self, d_vertices, n_vertices: int, d_triangles, n_triangles: int, d_vertices_out,
                          vertex_cap: int, d_triangles_out, triangle_cap: int, d_vertex_map=None, d_triangle_map=None,
                          min_triangles: int = 1, min_fraction: float = 0.0, max_components: int = 0,
                          stream: int | None = None):
        """dp_mesh_clean_device: a device mesh (addresses; tsdf_mesh_device's
        output) into at most vertex_cap records at d_vertices_out and
        triangle_cap triples at d_triangles_out, and the maps (None = not wanted).
        Queued on `stream`; one wait.  Returns (the full vertex count, the full
        triangle count -- above a cap: an overflow --, stats)."""
        mco = check_mesh_clean_args(min_triangles, min_fraction, max_components)
        nv, nt = _mesh_count("mesh_clean_device", n_vertices), _mesh_count("mesh_clean_device", n_triangles)
        _mesh_cap("mesh_clean_device", vertex_cap, d_vertices_out)
        _mesh_cap("mesh_clean_device", triangle_cap, d_triangles_out)
        if (nv and not d_vertices) or (nt and not d_triangles):
            raise ValueError("mesh_clean_device: the vertices and triangles must be given")
        no, to, st = ctypes.c_int64(), ctypes.c_int64(), N.DpMeshCleanStats()
        self._check(lib.dp_mesh_clean_device(self._ctx, ctypes.byref(mco), _addr(d_vertices), nv, _addr(d_triangles), nt,
                                             _addr(d_vertices_out), int(vertex_cap), ctypes.byref(no),
                                             _addr(d_triangles_out), int(triangle_cap), ctypes.byref(to),
                                             _addr(d_vertex_map), _addr(d_triangle_map), ctypes.byref(st),
                                             _addr(stream)))
        return int(no.value), int(to.value), _mesh_clean_stats(st)

    # ---- adjacency, smoothing, normals (include/densepoints.h dp_mesh_adjacency / _smooth / _normals) ----
    def mesh_adjacency(self, triangles, n_vertices: int) -> dict:
        """dp_mesh_adjacency: the vertex adjacency of `triangles` (n x 3 int32)
        over n_vertices vertices as sorted CSR rows.  Returns {"offsets" int32
        (n_vertices + 1), "neighbours" int32, "edge_triangles" int32 (the
        triangles on each entry's edge), "vertex_flags" uint8 (bit 0: on a
        boundary edge, bit 1: on a nonmanifold edge), "stats"}."""
        tris = _mesh_triangles("mesh_adjacency", triangles)
        nv = _mesh_count("mesh_adjacency", n_vertices)
        _mesh_entries("mesh_adjacency", len(tris))
        po, pn, pe, pf = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        ne, st = ctypes.c_int64(), N.DpMeshAdjacencyStats()
        self._check(lib.dp_mesh_adjacency(self._ctx, ptr(tris) if len(tris) else None, len(tris), nv, ctypes.byref(po),
                                          ctypes.byref(pn), ctypes.byref(pe), ctypes.byref(pf), ctypes.byref(ne),
                                          ctypes.byref(st)))
        E = int(ne.value)
        off, nbr, cnt = np.zeros(nv + 1, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)
        flags = np.zeros(nv, np.uint8)
        ctypes.memmove(off.ctypes.data, po.value, off.nbytes)
        if E:
            ctypes.memmove(nbr.ctypes.data, pn.value, nbr.nbytes)
            ctypes.memmove(cnt.ctypes.data, pe.value, cnt.nbytes)
        if nv:
            ctypes.memmove(flags.ctypes.data, pf.value, flags.nbytes)
        return dict(offsets=off, neighbours=nbr, edge_triangles=cnt, vertex_flags=flags, stats=_stats_dict(st))

    def mesh_adjacency_device(self, d_triangles, n_triangles: int, n_vertices: int, d_offsets=None, d_neighbours=None,
                              d_edge_triangles=None, entry_cap: int = 0, d_vertex_flags=None,
                              stream: int | None = None):
        """dp_mesh_adjacency_device: device triangles (an address) into the
        device arrays given (addresses, None = not wanted); d_neighbours and
        d_edge_triangles get at most entry_cap entries.  Queued on `stream`; one
        wait.  Returns (the full entry count -- above the cap: an overflow --,
        stats)."""
        nt, nv = _mesh_count("mesh_adjacency_device", n_triangles), _mesh_count("mesh_adjacency_device", n_vertices)
        _mesh_entries("mesh_adjacency_device", nt)
        if isinstance(entry_cap, bool) or not isinstance(entry_cap, (int, np.integer)) or entry_cap < 0:
            raise ValueError("mesh_adjacency_device: a cap must be >= 0")
        if nt and not d_triangles:
            raise ValueError("mesh_adjacency_device: the triangles must be given")
        ne, st = ctypes.c_int64(), N.DpMeshAdjacencyStats()
        self._check(lib.dp_mesh_adjacency_device(self._ctx, _addr(d_triangles), nt, nv, _addr(d_offsets),
                                                 _addr(d_neighbours), _addr(d_edge_triangles), int(entry_cap),
                                                 _addr(d_vertex_flags), ctypes.byref(ne), ctypes.byref(st),
                                                 _addr(stream)))
        return int(ne.value), _stats_dict(st)

    def mesh_smooth(self, vertices, triangles, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                    free_boundary: bool = False):
        """dp_mesh_smooth: `iterations` Taubin iterations (a step of factor lam,
        then one of factor mu; mu = 0: plain Laplacian steps) of the vertex
        positions towards their neighbours' mean; boundary vertices stay where
        they are unless free_boundary.  Returns (vertices with pos replaced,
        stats); the triangles are untouched."""
        mso = check_mesh_smooth_args(iterations, lam, mu, free_boundary)
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_smooth", triangles)
        nv, nt = len(verts), len(tris)
        _mesh_entries("mesh_smooth", nt)
        pv, st = ctypes.c_void_p(), N.DpMeshSmoothStats()
        self._check(lib.dp_mesh_smooth(self._ctx, ctypes.byref(mso), ptr(verts) if nv else None, nv,
                                       ptr(tris) if nt else None, nt, ctypes.byref(pv), ctypes.byref(st)))
        out = np.zeros(nv, dtype=N.MESH_VERTEX_DTYPE)
        if nv:
            ctypes.memmove(out.ctypes.data, pv.value, out.nbytes)
        return out, _stats_dict(st)

    def mesh_smooth_device(self, d_vertices, n_vertices: int, d_triangles, n_triangles: int, d_vertices_out,
                           iterations: int = 10, lam: float = 0.5, mu: float = -0.53, free_boundary: bool = False,
                           stats: bool = True, stream: int | None = None):
        """dp_mesh_smooth_device: a device mesh (addresses) smoothed into the
        n_vertices records at d_vertices_out (not d_vertices).  Every step is
        queued on `stream`; with stats=False the call does not wait and returns
        None, else it waits once and returns the stats."""
        mso = check_mesh_smooth_args(iterations, lam, mu, free_boundary)
        nv, nt = _mesh_count("mesh_smooth_device", n_vertices), _mesh_count("mesh_smooth_device", n_triangles)
        _mesh_entries("mesh_smooth_device", nt)
        if (nv and not (d_vertices and d_vertices_out)) or (nt and not d_triangles):
            raise ValueError("mesh_smooth_device: the vertices, the triangles and the output must be given")
        if nv and d_vertices == d_vertices_out:
            raise ValueError("mesh_smooth_device: the output must differ from the input")
        st = N.DpMeshSmoothStats()
        self._check(lib.dp_mesh_smooth_device(self._ctx, ctypes.byref(mso), _addr(d_vertices), nv, _addr(d_triangles),
                                              nt, _addr(d_vertices_out), ctypes.byref(st) if stats else None,
                                              _addr(stream)))
        return _stats_dict(st) if stats else None

    def mesh_normals(self, vertices, triangles):
        """dp_mesh_normals: the area-weighted unit normal of every vertex (the
        zero vector where no proper triangle names it or the sum vanishes).
        Returns (normals as n x 3 float32, stats)."""
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_normals", triangles)
        nv, nt = len(verts), len(tris)
        pn, st = ctypes.c_void_p(), N.DpMeshNormalsStats()
        self._check(lib.dp_mesh_normals(self._ctx, ptr(verts) if nv else None, nv, ptr(tris) if nt else None, nt,
                                        ctypes.byref(pn), ctypes.byref(st)))
        out = np.zeros((nv, 3), np.float32)
        if nv:
            ctypes.memmove(out.ctypes.data, pn.value, out.nbytes)
        return out, _stats_dict(st)

    def mesh_normals_device(self, d_vertices, n_vertices: int, d_triangles, n_triangles: int, d_normals,
                            stats: bool = True, stream: int | None = None):
        """dp_mesh_normals_device: the normals of a device mesh (addresses) into
        the 3 * n_vertices floats at d_normals.  Queued on `stream`; with
        stats=False the call does not wait and returns None."""
        nv, nt = _mesh_count("mesh_normals_device", n_vertices), _mesh_count("mesh_normals_device", n_triangles)
        if (nv and not (d_vertices and d_normals)) or (nt and not d_triangles):
            raise ValueError("mesh_normals_device: the vertices, the triangles and the output must be given")
        st = N.DpMeshNormalsStats()
        self._check(lib.dp_mesh_normals_device(self._ctx, _addr(d_vertices), nv, _addr(d_triangles), nt,
                                               _addr(d_normals), ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- simplification (include/densepoints.h dp_mesh_decimate) ----
    def mesh_decimate(self, vertices, triangles, cell, origin=(0.0, 0.0, 0.0), quadric: bool = False,
                      maps: bool = False):
        """dp_mesh_decimate: the mesh with the vertices of every cell (side
        `cell`, the lattice anchored at `origin`) merged into one, at their mean
        or (quadric=True) where the planes of the cell's triangles meet, without
        the triangles that collapse or repeat.  Returns (vertices, triangles,
        stats), and with maps=True also (vertex_map, triangle_map): the new index
        of every input vertex and triangle, or -1."""
        mdo = check_mesh_decimate_args(cell, origin, quadric)
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_decimate", triangles)
        nv, nt = len(verts), len(tris)
        _mesh_pairs("mesh_decimate", nt)
        vm = np.full(nv, -1, np.int32) if maps else None
        tm = np.full(nt, -1, np.int32) if maps else None
        pv, pt, no, to, st = (ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(),
                              N.DpMeshDecimateStats())
        self._check(lib.dp_mesh_decimate(self._ctx, ctypes.byref(mdo), ptr(verts) if nv else None, nv,
                                         ptr(tris) if nt else None, nt, ctypes.byref(pv), ctypes.byref(no),
                                         ctypes.byref(pt), ctypes.byref(to), ptr(vm) if maps and nv else None,
                                         ptr(tm) if maps and nt else None, ctypes.byref(st)))
        vout = np.zeros(no.value, dtype=N.MESH_VERTEX_DTYPE)
        tout = np.zeros((to.value, 3), dtype=np.int32)
        if no.value:
            ctypes.memmove(vout.ctypes.data, pv.value, vout.nbytes)
        if to.value:
            ctypes.memmove(tout.ctypes.data, pt.value, tout.nbytes)
        out = (vout, tout, _stats_dict(st))
        return out + (vm, tm) if maps else out

    def mesh_decimate_device(self, d_vertices, n_vertices: int, d_triangles, n_triangles: int, d_vertices_out,
                             vertex_cap: int, d_triangles_out, triangle_cap: int, cell, origin=(0.0, 0.0, 0.0),
                             quadric: bool = False, d_vertex_map=None, d_triangle_map=None, stats: bool = True,
                             stream: int | None = None):
        """dp_mesh_decimate_device: a device mesh (addresses) into at most
        vertex_cap records at d_vertices_out and triangle_cap triples at
        d_triangles_out, and the maps (None = not wanted).  Queued on `stream`;
        one wait.  Returns (the full vertex count, the full triangle count --
        above a cap: an overflow --, stats, or None with stats=False)."""
        mdo = check_mesh_decimate_args(cell, origin, quadric)
        nv, nt = _mesh_count("mesh_decimate_device", n_vertices), _mesh_count("mesh_decimate_device", n_triangles)
        _mesh_pairs("mesh_decimate_device", nt)
        _mesh_cap("mesh_decimate_device", vertex_cap, d_vertices_out)
        _mesh_cap("mesh_decimate_device", triangle_cap, d_triangles_out)
        if (nv and not d_vertices) or (nt and not d_triangles):
            raise ValueError("mesh_decimate_device: the vertices and triangles must be given")
        no, to, st = ctypes.c_int64(), ctypes.c_int64(), N.DpMeshDecimateStats()
        self._check(lib.dp_mesh_decimate_device(self._ctx, ctypes.byref(mdo), _addr(d_vertices), nv, _addr(d_triangles),
                                                nt, _addr(d_vertices_out), int(vertex_cap), ctypes.byref(no),
                                                _addr(d_triangles_out), int(triangle_cap), ctypes.byref(to),
                                                _addr(d_vertex_map), _addr(d_triangle_map),
                                                ctypes.byref(st) if stats else None, _addr(stream)))
        return int(no.value), int(to.value), _stats_dict(st) if stats else None

    # ---- per-view maps of a mesh (include/densepoints.h dp_mesh_render) ----
    def mesh_render(self, vertices, triangles, views=None, cull_back: bool = False, normals: bool = False) -> dict:
        """dp_mesh_render: every triangle rasterised into `views` (None = all) at
        the current level, nearest triangle per pixel; cull_back skips the
        triangles that do not face the view.  Returns {"views", "depth" (f32, 0 =
        empty), "index" (int32 triangle, -1 = empty), "normal" (the winner's unit
        face normal) when asked for, "stats"}, each map a list of H x W (x 3)
        arrays in the order of "views"."""
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_render", triangles)
        nv, nt = len(verts), len(tris)
        mro, vid = check_mesh_render_args(nv, nt, self.num_views(), views, cull_back)
        sizes = self.view_sizes(vid)
        out = {"views": [int(v) for v in vid],
               "depth": [np.zeros((h, w), np.float32) for w, h in sizes],
               "index": [np.zeros((h, w), np.int32) for w, h in sizes]}
        if normals:
            out["normal"] = [np.zeros((h, w, 3), np.float32) for w, h in sizes]

        def table(key):
            return (ctypes.c_void_p * len(vid))(*[a.ctypes.data for a in out[key]]) if key in out else None

        st = N.DpMeshRenderStats()
        self._check(lib.dp_mesh_render(self._ctx, ptr(verts) if nv else None, nv, ptr(tris) if nt else None, nt,
                                       ptr(vid), len(vid), ctypes.byref(mro), table("depth"), table("index"),
                                       table("normal"), ctypes.byref(st)))
        out["stats"] = _stats_dict(st)
        return out

    def mesh_render_device(self, d_vertices, n_vertices: int, d_triangles, n_triangles: int, views, d_depth=None,
                           d_index=None, d_normal=None, cull_back: bool = False, stream: int | None = None,
                           stats: bool = True) -> dict | None:
        """dp_mesh_render_device: a device mesh (addresses) into device planes --
        d_depth / d_index / d_normal are lists of device addresses, one per entry
        of `views` (None or 0 = not wanted).  Queued on `stream`; waits only for
        the statistics (stats=False: no wait, returns None)."""
        nv, nt = _mesh_count("mesh_render_device", n_vertices), _mesh_count("mesh_render_device", n_triangles)
        mro, vid = check_mesh_render_args(nv, nt, self.num_views(), views, cull_back)
        if (nv and not d_vertices) or (nt and not d_triangles):
            raise ValueError("mesh_render_device: the vertices and triangles must be given")

        def table(addrs):
            if addrs is None:
                return None
            if len(addrs) != len(vid):
                raise ValueError("mesh_render_device: one plane address per view")
            return (ctypes.c_void_p * len(vid))(*[int(a) if a else None for a in addrs])

        st = N.DpMeshRenderStats()
        self._check(lib.dp_mesh_render_device(self._ctx, _addr(d_vertices), nv, _addr(d_triangles), nt, ptr(vid),
                                              len(vid), ctypes.byref(mro), table(d_depth), table(d_index),
                                              table(d_normal), ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- vertex colours from the views (include/densepoints.h dp_mesh_colour) ----
    def mesh_colour(self, vertices, views=None, depth=None, triangles=None, normals=None, depth_tol: float = 0.01,
                    min_cos: float = 0.2, bilinear: bool = False, clear_unseen: bool = False) -> dict:
        """dp_mesh_colour: every vertex coloured by the mean of the texels of the
        `views` (None = all, at most 64) that see it at the current level.
        `depth` is one H x W float32 plane of the mesh per view, in the order of
        `views` (mesh_render's "depth"); None renders them here from `triangles`
        (mesh_render without culling).  `normals` (n x 3 float32, mesh_normals'
        output) weights a view by the cosine between the normal and the ray to
        its camera and drops it below min_cos; depth_tol is the relative depth by
        which a vertex may lie behind the plane; bilinear samples four taps
        instead of the nearest texel; clear_unseen blacks the vertices no view
        sees instead of keeping their colour.  Returns {"vertices", "seen"
        (uint64, bit k = views[k]), "best" (int32 position in views, -1 =
        unseen), "views", "stats"}."""
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        nv = len(verts)
        mco, vid = check_mesh_colour_args(nv, self.num_views(), views, depth, depth_tol, min_cos, bilinear,
                                          clear_unseen)
        sizes = self.view_sizes(vid)
        if depth is None:
            if triangles is None:
                raise ValueError("mesh_colour: depth planes or triangles must be given")
            depth = self.mesh_render(verts, triangles, views=vid)["depth"]
        planes = [np.ascontiguousarray(d, dtype=np.float32) for d in depth]
        if any(p.shape != (h, w) for p, (w, h) in zip(planes, sizes)):
            raise ValueError("mesh_colour: a depth plane must be H x W of its view at the current level")
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float32)
            if nrm.shape != (nv, 3):
                raise ValueError("mesh_colour: normals must be n_vertices x 3")
        seen, best = np.zeros(nv, np.uint64), np.zeros(nv, np.int32)
        tab = (ctypes.c_void_p * len(vid))(*[p.ctypes.data for p in planes])
        pv, st = ctypes.c_void_p(), N.DpMeshColourStats()
        self._check(lib.dp_mesh_colour(self._ctx, ptr(verts) if nv else None, nv,
                                       ptr(nrm) if nrm is not None and nv else None, ptr(vid), len(vid),
                                       ctypes.byref(mco), tab, ctypes.byref(pv), ptr(seen) if nv else None,
                                       ptr(best) if nv else None, ctypes.byref(st)))
        out = np.zeros(nv, dtype=N.MESH_VERTEX_DTYPE)
        if nv:
            ctypes.memmove(out.ctypes.data, pv.value, out.nbytes)
        return {"vertices": out, "seen": seen, "best": best, "views": [int(v) for v in vid], "stats": _stats_dict(st)}

    def mesh_colour_device(self, d_vertices, n_vertices: int, views, d_depth, d_vertices_out, d_normals=None,
                           d_seen=None, d_best=None, depth_tol: float = 0.01, min_cos: float = 0.2,
                           bilinear: bool = False, clear_unseen: bool = False, stream: int | None = None,
                           stats: bool = True) -> dict | None:
        """dp_mesh_colour_device: device vertices (addresses) coloured into the
        n_vertices records at d_vertices_out; d_depth is a list of device plane
        addresses, one per entry of `views`; d_normals, d_seen and d_best are
        optional (None or 0 = not given / not wanted).  Queued on `stream`; waits
        only for the statistics (stats=False: no wait, returns None)."""
        nv = _mesh_count("mesh_colour_device", n_vertices)
        mco, vid = check_mesh_colour_args(nv, self.num_views(), views, d_depth, depth_tol, min_cos, bilinear,
                                          clear_unseen, inputs=(d_vertices, d_normals), outputs=(d_vertices_out, d_seen,
                                                                                                 d_best))
        if d_depth is None:
            raise ValueError("mesh_colour_device: the depth planes must be given")
        if nv and not (d_vertices and d_vertices_out):
            raise ValueError("mesh_colour_device: the vertices and the output must be given")
        tab = (ctypes.c_void_p * len(vid))(*[int(a) for a in d_depth])
        st = N.DpMeshColourStats()
        self._check(lib.dp_mesh_colour_device(self._ctx, _addr(d_vertices), nv, _addr(d_normals), ptr(vid), len(vid),
                                              ctypes.byref(mco), tab, _addr(d_vertices_out), _addr(d_seen),
                                              _addr(d_best), ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- nearest points between two clouds (include/densepoints.h dp_cloud_nearest) ----
    def cloud_nearest(self, queries, targets, max_dist: float, hist_bins: int = 0) -> dict:
        """dp_cloud_nearest: for every query the nearest target within max_dist
        (ties to the lowest index).  `queries` and `targets` are (n, 3) float32
        arrays or structured arrays with a `pos` field (patches, FUSED_DTYPE,
        MESH_VERTEX_DTYPE), which are passed with their own stride, not copied to
        packed form.  Returns {"index" (int32, -1 = none), "dist" (float32, inf
        = none), "hist" (uint64 per bin, or None), "stats"}.  Needs no views."""
        qa, qp, nq, qs = _cloud_points("cloud_nearest", queries)
        ta, tp, nt, ts = _cloud_points("cloud_nearest", targets)
        cno = check_cloud_nearest_args(nq, nt, max_dist, hist_bins, qs, ts)
        pi, pd, ph, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), N.DpCloudNearestStats()
        self._check(lib.dp_cloud_nearest(self._ctx, _addr(qp) if nq else None, nq, qs, _addr(tp) if nt else None, nt,
                                         ts, ctypes.byref(cno), ctypes.byref(pi), ctypes.byref(pd),
                                         ctypes.byref(ph) if hist_bins else None, ctypes.byref(st)))
        index, dist = np.zeros(nq, np.int32), np.zeros(nq, np.float32)
        if nq:
            ctypes.memmove(index.ctypes.data, pi.value, index.nbytes)
            ctypes.memmove(dist.ctypes.data, pd.value, dist.nbytes)
        hist = None
        if hist_bins:
            hist = np.zeros(hist_bins, np.uint64)
            ctypes.memmove(hist.ctypes.data, ph.value, hist.nbytes)
        del qa, ta
        return {"index": index, "dist": dist, "hist": hist, "stats": _stats_dict(st)}

    def cloud_nearest_device(self, d_queries, n_queries: int, query_stride: int, d_targets, n_targets: int,
                             target_stride: int, max_dist: float, d_index, d_dist, d_hist=None, hist_bins: int = 0,
                             stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_cloud_nearest_device: device clouds (the addresses of their first
        points, strides in bytes) searched into n_queries int32 at d_index and
        float32 at d_dist, and hist_bins uint64 at d_hist when that is given.
        Queued on `stream`; waits only for the statistics (stats=False: no wait,
        returns None)."""
        nq, nt = _mesh_count("cloud_nearest_device", n_queries), _mesh_count("cloud_nearest_device", n_targets)
        cno = check_cloud_nearest_args(nq, nt, max_dist, hist_bins, query_stride, target_stride,
                                       inputs=(d_queries, d_targets), outputs=(d_index, d_dist, d_hist))
        if (nq and not d_queries) or (nt and not d_targets):
            raise ValueError("cloud_nearest_device: the queries and the targets must be given")
        if nq and not (d_index and d_dist):
            raise ValueError("cloud_nearest_device: d_index and d_dist must be given")
        st = N.DpCloudNearestStats()
        self._check(lib.dp_cloud_nearest_device(self._ctx, _addr(d_queries), nq, query_stride, _addr(d_targets), nt,
                                                target_stride, ctypes.byref(cno), _addr(d_index), _addr(d_dist),
                                                _addr(d_hist), ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- the k nearest neighbours between two clouds (include/densepoints.h dp_cloud_knn) ----
    def cloud_knn(self, queries, targets, k: int, max_dist: float, exclude_self: bool = False) -> dict:
        """dp_cloud_knn: for every query its k nearest targets within max_dist,
        ordered by (distance, index).  The clouds are what cloud_nearest takes.
        With exclude_self target i is never a neighbour of query i (the clouds
        must have the same length).  Returns {"index" (n x k int32, -1 = none),
        "dist" (n x k float32, inf = none), "count" (int32 per query), "stats"}.
        Needs no views."""
        qa, qp, nq, qs = _cloud_points("cloud_knn", queries)
        ta, tp, nt, ts = _cloud_points("cloud_knn", targets)
        cko = check_cloud_knn_args(nq, nt, k, max_dist, exclude_self, qs, ts)
        pi, pd, pc, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), N.DpCloudKnnStats()
        self._check(lib.dp_cloud_knn(self._ctx, _addr(qp) if nq else None, nq, qs, _addr(tp) if nt else None, nt, ts,
                                     ctypes.byref(cko), ctypes.byref(pi), ctypes.byref(pd), ctypes.byref(pc),
                                     ctypes.byref(st)))
        index, dist = np.zeros((nq, cko.k), np.int32), np.zeros((nq, cko.k), np.float32)
        count = np.zeros(nq, np.int32)
        if nq:
            ctypes.memmove(index.ctypes.data, pi.value, index.nbytes)
            ctypes.memmove(dist.ctypes.data, pd.value, dist.nbytes)
            ctypes.memmove(count.ctypes.data, pc.value, count.nbytes)
        del qa, ta
        return {"index": index, "dist": dist, "count": count, "stats": _stats_dict(st)}

    def cloud_knn_device(self, d_queries, n_queries: int, query_stride: int, d_targets, n_targets: int,
                         target_stride: int, k: int, max_dist: float, d_index, d_dist, d_count,
                         exclude_self: bool = False, stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_cloud_knn_device: device clouds (the addresses of their first
        points, strides in bytes) searched into n_queries x k int32 at d_index
        and float32 at d_dist and n_queries int32 at d_count.  Queued on `stream`;
        waits only for the statistics (stats=False: no wait, returns None)."""
        nq, nt = _mesh_count("cloud_knn_device", n_queries), _mesh_count("cloud_knn_device", n_targets)
        cko = check_cloud_knn_args(nq, nt, k, max_dist, exclude_self, query_stride, target_stride,
                                   inputs=(d_queries, d_targets), outputs=(d_index, d_dist, d_count))
        if (nq and not d_queries) or (nt and not d_targets):
            raise ValueError("cloud_knn_device: the queries and the targets must be given")
        if nq and not (d_index and d_dist and d_count):
            raise ValueError("cloud_knn_device: d_index, d_dist and d_count must be given")
        st = N.DpCloudKnnStats()
        self._check(lib.dp_cloud_knn_device(self._ctx, _addr(d_queries), nq, query_stride, _addr(d_targets), nt,
                                            target_stride, ctypes.byref(cko), _addr(d_index), _addr(d_dist),
                                            _addr(d_count), ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- outlier removal of a cloud (include/densepoints.h dp_cloud_clean) ----
    def cloud_clean(self, points, k: int, max_dist: float, std_mul: float = 2.0, min_neighbours: int = 1,
                    radius_only: bool = False) -> dict:
        """dp_cloud_clean: statistical (or, with radius_only, radius) outlier
        removal.  `points` is what cloud_nearest takes; a structured array's pos
        field must come first, and its records move whole.  Returns {"keep"
        (uint8 per point), "mean_dist" (float32, inf = no neighbour), "map"
        (int32, -1 = removed), "points" (the kept records, of the input's
        dtype), "stats"}.  Needs no views."""
        pa, pp, n, stride = _cloud_points("cloud_clean", points)
        if pp != pa.ctypes.data:
            raise ValueError("cloud_clean: the pos field must be the first of a record")
        cco = check_cloud_clean_args(n, k, max_dist, std_mul, min_neighbours, radius_only, stride)
        pk, pm, pi, po = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n_out, st = ctypes.c_int64(0), N.DpCloudCleanStats()
        self._check(lib.dp_cloud_clean(self._ctx, _addr(pp) if n else None, n, stride, ctypes.byref(cco),
                                       ctypes.byref(pk), ctypes.byref(pm), ctypes.byref(pi), ctypes.byref(po),
                                       ctypes.byref(n_out), ctypes.byref(st)))
        keep, mean, where = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.int32)
        if n:
            ctypes.memmove(keep.ctypes.data, pk.value, keep.nbytes)
            ctypes.memmove(mean.ctypes.data, pm.value, mean.nbytes)
            ctypes.memmove(where.ctypes.data, pi.value, where.nbytes)
        kept = np.zeros((n_out.value,) + pa.shape[1:], pa.dtype)
        if n_out.value:
            ctypes.memmove(kept.ctypes.data, po.value, kept.nbytes)
        return {"keep": keep, "mean_dist": mean, "map": where, "points": kept, "stats": _stats_dict(st)}

    def cloud_clean_device(self, d_points, n: int, stride: int, k: int, max_dist: float, d_keep, d_mean_dist=None,
                           d_map=None, d_out=None, d_n_out=None, std_mul: float = 2.0, min_neighbours: int = 1,
                           radius_only: bool = False, stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_cloud_clean_device: n device records of `stride` bytes filtered
        into n uint8 at d_keep and, where given, n float32 at d_mean_dist, n
        int32 at d_map, the kept records at d_out (room for n) and their count as
        one int64 at d_n_out.  Queued on `stream`; waits only for the statistics
        (stats=False: no wait, returns None)."""
        n = _mesh_count("cloud_clean_device", n)
        cco = check_cloud_clean_args(n, k, max_dist, std_mul, min_neighbours, radius_only, stride,
                                     inputs=(d_points,), outputs=(d_keep, d_mean_dist, d_map, d_out, d_n_out))
        if n and not d_points:
            raise ValueError("cloud_clean_device: the points must be given")
        if n and not d_keep:
            raise ValueError("cloud_clean_device: d_keep must be given")
        st = N.DpCloudCleanStats()
        self._check(lib.dp_cloud_clean_device(self._ctx, _addr(d_points), n, stride, ctypes.byref(cco), _addr(d_keep),
                                              _addr(d_mean_dist), _addr(d_map), _addr(d_out), _addr(d_n_out),
                                              ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- PCA normals of a cloud (include/densepoints.h dp_cloud_normals) ----
    def cloud_normals(self, points, k: int = 16, *, max_dist: float, min_neighbours: int = 3, viewpoint=None,
                      directions=None) -> dict:
        """dp_cloud_normals: for every point the unit normal of the plane fitted
        to its k nearest points within max_dist (itself included) and the surface
        variation of that neighbourhood.  `points` is what cloud_nearest takes.
        viewpoint (one xyz, or an (n, 3) array) turns every normal toward that
        position; directions (an (n, 3) array, or True for the records' own
        `normal` field, read in place) toward that direction; without either the
        sign is the canonical one.  Returns {"normal" (n x 3 float32, zero where
        none was estimated), "variation" (float32, inf there), "count" (int32,
        the neighbourhood's size), "stats"}.  Needs no views."""
        pa, pp, n, stride = _cloud_points("cloud_normals", points)
        if viewpoint is not None and directions is not None:
            raise ValueError("cloud_normals: viewpoint and directions exclude each other")
        orient, toward, ta, ts = None, None, None, 0
        if viewpoint is not None:
            orient = "viewpoint"
            ta = np.ascontiguousarray(viewpoint, dtype=np.float32)
            if ta.shape == (3,):
                ts = 0
            elif ta.shape == (n, 3):
                ts = 12
            else:
                raise ValueError("cloud_normals: viewpoint must be one xyz or an n x 3 array")
            toward = ta.ctypes.data
        elif directions is not None:
            orient = "direction"
            if isinstance(directions, (bool, np.bool_)):
                if not directions:
                    raise ValueError("cloud_normals: directions must be an n x 3 array or True")
                toward, ts = pa.ctypes.data + _cloud_normal_offset("cloud_normals", pa, True), stride
            else:
                ta = np.ascontiguousarray(directions, dtype=np.float32)
                if ta.shape != (n, 3):
                    raise ValueError("cloud_normals: directions must be an n x 3 array or True")
                toward, ts = ta.ctypes.data, 12
        cno = check_cloud_normals_args(n, k, max_dist, min_neighbours, orient, orient is not None, ts, stride)
        pn, pv, pc, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), N.DpCloudNormalsStats()
        self._check(lib.dp_cloud_normals(self._ctx, _addr(pp) if n else None, n, stride, ctypes.byref(cno),
                                         _addr(toward) if orient else None, ts, ctypes.byref(pn), ctypes.byref(pv),
                                         ctypes.byref(pc), ctypes.byref(st)))
        normal, variation, count = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        if n:
            ctypes.memmove(normal.ctypes.data, pn.value, normal.nbytes)
            ctypes.memmove(variation.ctypes.data, pv.value, variation.nbytes)
            ctypes.memmove(count.ctypes.data, pc.value, count.nbytes)
        del pa, ta
        return {"normal": normal, "variation": variation, "count": count, "stats": _stats_dict(st)}

    def cloud_normals_device(self, d_points, n: int, stride: int, k: int, max_dist: float, d_normal, d_variation=None,
                             d_count=None, min_neighbours: int = 3, orient=None, d_toward=None,
                             toward_stride: int = 0, stream: int | None = None, stats: bool = True) -> dict | None:
        """dp_cloud_normals_device: n device records of `stride` bytes estimated
        into 3 n float32 at d_normal and, where given, n float32 at d_variation
        and n int32 at d_count.  orient is None, "viewpoint" or "direction"; with
        one, entry i of `toward` is the three float32 at d_toward + i *
        toward_stride (0 = one entry for all), which may lie in the records.
        Queued on `stream`; waits only for the statistics (stats=False: no wait,
        returns None)."""
        n = _mesh_count("cloud_normals_device", n)
        cno = check_cloud_normals_args(n, k, max_dist, min_neighbours, orient, bool(d_toward), toward_stride, stride,
                                       inputs=(d_points, d_toward), outputs=(d_normal, d_variation, d_count))
        if n and not d_points:
            raise ValueError("cloud_normals_device: the points must be given")
        if n and not d_normal:
            raise ValueError("cloud_normals_device: d_normal must be given")
        st = N.DpCloudNormalsStats()
        self._check(lib.dp_cloud_normals_device(self._ctx, _addr(d_points), n, stride, ctypes.byref(cno),
                                                _addr(d_toward), int(toward_stride), _addr(d_normal),
                                                _addr(d_variation), _addr(d_count),
                                                ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None

    # ---- a cloud's records under a 3 x 4 transform (include/densepoints.h dp_cloud_transform) ----
    def cloud_transform(self, points, matrix, normals: bool = False) -> np.ndarray:
        """dp_cloud_transform: the records of `points` ((n, 3) float32, or a
        structured array whose pos field comes first) with their positions under
        the 3 x 4 float64 `matrix` [A | t]; with normals=True the structured
        array's `normal` field becomes the unit A * normal.  Records move whole;
        a point that is not finite is left as it is.  Returns a new array of the
        input's dtype.  Needs no views."""
        pa, pp, n, stride = _cloud_points("cloud_transform", points)
        if pp != pa.ctypes.data:
            raise ValueError("cloud_transform: the pos field must be the first of a record")
        off = _cloud_normal_offset("cloud_transform", pa, normals)
        m = check_cloud_transform_args(n, matrix, stride, off)
        po = ctypes.c_void_p()
        self._check(lib.dp_cloud_transform(self._ctx, _addr(pp) if n else None, n, stride, ptr(m), off,
                                           ctypes.byref(po)))
        out = np.zeros(pa.shape, pa.dtype)
        if n:
            ctypes.memmove(out.ctypes.data, po.value, out.nbytes)
        return out

    def cloud_transform_device(self, d_points, n: int, stride: int, matrix, d_out, normal_offset: int = -1,
                               stream: int | None = None) -> None:
        """dp_cloud_transform_device: n device records of `stride` bytes at
        d_points transformed into d_out (which may be d_points: in place), the
        normal at the byte offset normal_offset (-1 = none).  Queued on `stream`;
        does not wait."""
        n = _mesh_count("cloud_transform_device", n)
        m = check_cloud_transform_args(n, matrix, stride, normal_offset)
        if n and not (d_points and d_out):
            raise ValueError("cloud_transform_device: the points and d_out must be given")
        self._check(lib.dp_cloud_transform_device(self._ctx, _addr(d_points), n, stride, ptr(m), int(normal_offset),
                                                  _addr(d_out), _addr(stream)))

    # ---- registration of one cloud to another (include/densepoints.h dp_cloud_align) ----
    def cloud_align(self, source, target, max_dist: float, iterations: int = 30, scale: bool = False, init=None,
                    rms_tol: float = 0.0, min_pairs: int = 3, correspondences: bool = False) -> dict:
        """dp_cloud_align: point-to-point ICP of `source` onto `target` (clouds as
        cloud_nearest takes them), trimmed at max_dist; scale=True estimates a
        similarity.  Returns {"matrix" (3 x 4 float64, source -> target),
        "scale", "trace" (iterations + 1 records of matched and rms, zero after
        the stop), "index" and "dist" of the last pass (with correspondences,
        else None), "stats"}.  Needs no views."""
        sa, sp, n, ss = _cloud_points("cloud_align", source)
        ta, tp, nt, ts = _cloud_points("cloud_align", target)
        cao, m0 = check_cloud_align_args(n, nt, max_dist, iterations, scale, init, rms_tol, min_pairs, ss, ts)
        M, s = np.zeros((3, 4), np.float64), ctypes.c_double(0.0)
        trace = np.zeros(cao.iterations + 1, N.CLOUD_ALIGN_STEP_DTYPE)
        pi, pd, st = ctypes.c_void_p(), ctypes.c_void_p(), N.DpCloudAlignStats()
        self._check(lib.dp_cloud_align(self._ctx, _addr(sp) if n else None, n, ss, _addr(tp) if nt else None, nt, ts,
                                       ctypes.byref(cao), ptr(m0) if m0 is not None else None, ptr(M), ctypes.byref(s),
                                       ptr(trace), ctypes.byref(pi) if correspondences else None,
                                       ctypes.byref(pd) if correspondences else None, ctypes.byref(st)))
        index = dist = None
        if correspondences:
            index, dist = np.zeros(n, np.int32), np.zeros(n, np.float32)
            if n:
                ctypes.memmove(index.ctypes.data, pi.value, index.nbytes)
                ctypes.memmove(dist.ctypes.data, pd.value, dist.nbytes)
        del sa, ta
        return {"matrix": M, "scale": s.value, "trace": trace, "index": index, "dist": dist, "stats": _stats_dict(st)}

    def cloud_align_device(self, d_source, n_source: int, source_stride: int, d_target, n_target: int,
                           target_stride: int, max_dist: float, iterations: int = 30, scale: bool = False, init=None,
                           rms_tol: float = 0.0, min_pairs: int = 3, d_index=None, d_dist=None,
                           stream: int | None = None) -> dict:
        """dp_cloud_align_device: device clouds (the addresses of their first
        points, strides in bytes); the last pass's index and dist go to n_source
        int32 at d_index and float32 at d_dist when both are given.  The call
        waits once per pass.  Returns cloud_align's dict without index and dist."""
        n, nt = _mesh_count("cloud_align_device", n_source), _mesh_count("cloud_align_device", n_target)
        cao, m0 = check_cloud_align_args(n, nt, max_dist, iterations, scale, init, rms_tol, min_pairs, source_stride,
                                         target_stride, inputs=(d_source, d_target), outputs=(d_index, d_dist))
        if (n and not d_source) or (nt and not d_target):
            raise ValueError("cloud_align_device: the source and the target must be given")
        if bool(d_index) != bool(d_dist):
            raise ValueError("cloud_align_device: d_index and d_dist must be given together")
        M, s = np.zeros((3, 4), np.float64), ctypes.c_double(0.0)
        trace = np.zeros(cao.iterations + 1, N.CLOUD_ALIGN_STEP_DTYPE)
        st = N.DpCloudAlignStats()
        self._check(lib.dp_cloud_align_device(self._ctx, _addr(d_source), n, source_stride, _addr(d_target), nt,
                                              target_stride, ctypes.byref(cao), ptr(m0) if m0 is not None else None,
                                              ptr(M), ctypes.byref(s), ptr(trace), _addr(d_index), _addr(d_dist),
                                              ctypes.byref(st), _addr(stream)))
        return {"matrix": M, "scale": s.value, "trace": trace, "stats": _stats_dict(st)}

    # ---- nearest triangles of a mesh (include/densepoints.h dp_mesh_nearest) ----
    def mesh_nearest(self, queries, vertices, triangles, max_dist: float, hist_bins: int = 0,
                     closest: bool = False) -> dict:
        """dp_mesh_nearest: for every query the nearest triangle of the mesh
        within max_dist (ties to the lowest index).  `queries` is what
        cloud_nearest takes; `vertices` MESH_VERTEX_DTYPE records or an (n, 3)
        array; `triangles` n x 3 integers.  Returns {"index" (int32, -1 = none),
        "dist" (float32, inf = none), "closest" (n x 3 float32, or None), "hist"
        (uint64 per bin, or None), "stats"}.  Needs no views."""
        qa, qp, nq, qs = _cloud_points("mesh_nearest", queries)
        verts = _mesh_vertices("mesh_nearest", vertices)
        tris = _mesh_triangles("mesh_nearest", triangles)
        nv, nt = len(verts), len(tris)
        mno = check_mesh_nearest_args(nq, nv, nt, max_dist, hist_bins, qs)
        pi, pd, pc, ph = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        st = N.DpMeshNearestStats()
        self._check(lib.dp_mesh_nearest(self._ctx, _addr(qp) if nq else None, nq, qs, ptr(verts) if nv else None, nv,
                                        ptr(tris) if nt else None, nt, ctypes.byref(mno), ctypes.byref(pi),
                                        ctypes.byref(pd), ctypes.byref(pc) if closest else None,
                                        ctypes.byref(ph) if hist_bins else None, ctypes.byref(st)))
        index, dist = np.zeros(nq, np.int32), np.zeros(nq, np.float32)
        where = np.zeros((nq, 3), np.float32) if closest else None
        if nq:
            ctypes.memmove(index.ctypes.data, pi.value, index.nbytes)
            ctypes.memmove(dist.ctypes.data, pd.value, dist.nbytes)
            if closest:
                ctypes.memmove(where.ctypes.data, pc.value, where.nbytes)
        hist = None
        if hist_bins:
            hist = np.zeros(hist_bins, np.uint64)
            ctypes.memmove(hist.ctypes.data, ph.value, hist.nbytes)
        del qa
        return {"index": index, "dist": dist, "closest": where, "hist": hist, "stats": _stats_dict(st)}

    def mesh_nearest_device(self, d_queries, n_queries: int, query_stride: int, d_vertices, n_vertices: int,
                            d_triangles, n_triangles: int, max_dist: float, d_index, d_dist, d_closest=None,
                            d_hist=None, hist_bins: int = 0, stream: int | None = None,
                            stats: bool = True) -> dict | None:
        """dp_mesh_nearest_device: device queries (the address of the first
        point, the stride in bytes) against a device mesh (addresses) into
        n_queries int32 at d_index and float32 at d_dist, 3 * n_queries float32 at
        d_closest and hist_bins uint64 at d_hist when those are given.  Queued on
        `stream`; waits only for the statistics (stats=False: no wait, returns
        None)."""
        who = "mesh_nearest_device"
        nq, nv, nt = _mesh_count(who, n_queries), _mesh_count(who, n_vertices), _mesh_count(who, n_triangles)
        mno = check_mesh_nearest_args(nq, nv, nt, max_dist, hist_bins, query_stride,
                                      inputs=(d_queries, d_vertices, d_triangles),
                                      outputs=(d_index, d_dist, d_closest, d_hist))
        if (nq and not d_queries) or (nv and not d_vertices) or (nt and not d_triangles):
            raise ValueError("mesh_nearest_device: the queries, the vertices and the triangles must be given")
        if nq and not (d_index and d_dist):
            raise ValueError("mesh_nearest_device: d_index and d_dist must be given")
        st = N.DpMeshNearestStats()
        self._check(lib.dp_mesh_nearest_device(self._ctx, _addr(d_queries), nq, query_stride, _addr(d_vertices), nv,
                                               _addr(d_triangles), nt, ctypes.byref(mno), _addr(d_index),
                                               _addr(d_dist), _addr(d_closest), _addr(d_hist),
                                               ctypes.byref(st) if stats else None, _addr(stream)))
        return _stats_dict(st) if stats else None


def _cloud_points(who: str, a):
    """A cloud as dp_cloud_nearest takes it: (the array that owns the memory,
    the address of the first point, the count, the stride in bytes)."""
    a = np.asarray(a)
    if a.dtype.names:
        if "pos" not in a.dtype.names or a.dtype.fields["pos"][0] != np.dtype(("<f4", 3)):
            raise ValueError("%s: a structured cloud needs a pos field of three float32" % who)
        a = np.ascontiguousarray(a).reshape(-1)
        stride = a.dtype.itemsize
        if stride % 4 or a.dtype.fields["pos"][1] % 4:
            raise ValueError("%s: a record's size and its pos offset must be multiples of 4" % who)
        return a, a.ctypes.data + a.dtype.fields["pos"][1], _mesh_count(who, len(a)), stride
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: a cloud must be n x 3 float32 or a structured array with a pos field" % who)
    return a, a.ctypes.data, _mesh_count(who, len(a)), 12


def check_cloud_nearest_args(n_queries, n_targets, max_dist, hist_bins=0, query_stride=12, target_stride=12, flags=0,
                             inputs=(), outputs=()):
    """Argument validation of Engine.cloud_nearest[_device] (the limits of
    dp_cloud_nearest, raised as ValueError before any device call); returns the
    dp_cloud_nearest_options.  max_dist is judged as the float32 the struct
    holds; `inputs` and `outputs`: the device form's addresses, of which no
    output may equal an input."""
    def whole(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

    _mesh_count("cloud_nearest", n_queries)
    _mesh_count("cloud_nearest", n_targets)
    for name, s in (("query_stride", query_stride), ("target_stride", target_stride)):
        if not whole(s) or s < 12 or s % 4:
            raise ValueError("cloud_nearest: %s must be a multiple of 4 and at least 12" % name)
    with np.errstate(over="ignore"):
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(np.float32(max_dist)) and np.float32(max_dist) > 0):
            raise ValueError("cloud_nearest: max_dist must be finite and > 0")
    if not whole(hist_bins) or not 0 <= hist_bins <= 65536:
        raise ValueError("cloud_nearest: hist_bins must be in 0..65536")
    if not whole(flags) or flags != 0:
        raise ValueError("cloud_nearest: unknown flags")
    ins = [a for a in inputs if isinstance(a, (int, np.integer)) and a]
    if any(isinstance(o, (int, np.integer)) and o and o in ins for o in outputs):
        raise ValueError("cloud_nearest: an output equals an input")
    return N.DpCloudNearestOptions(float(max_dist), int(hist_bins), int(flags))


def _cloud_search_args(who: str, k, max_dist):
    """k and max_dist as dp_cloud_knn and dp_cloud_clean judge them."""
    with np.errstate(over="ignore"):
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(np.float32(max_dist)) and np.float32(max_dist) > 0):
            raise ValueError("%s: max_dist must be finite and > 0" % who)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 32:
        raise ValueError("%s: k must be in 1..32" % who)


def _cloud_aliases(who: str, inputs, outputs, among_outputs=False):
    ins = [a for a in inputs if isinstance(a, (int, np.integer)) and a]
    outs = [o for o in outputs if isinstance(o, (int, np.integer)) and o]
    if any(o in ins for o in outs):
        raise ValueError("%s: an output equals an input" % who)
    if among_outputs and len(set(outs)) != len(outs):
        raise ValueError("%s: two outputs are equal" % who)


def check_cloud_knn_args(n_queries, n_targets, k, max_dist, exclude_self=False, query_stride=12, target_stride=12,
                         inputs=(), outputs=()):
    """Argument validation of Engine.cloud_knn[_device] (the limits of
    dp_cloud_knn, raised as ValueError before any device call); returns the
    dp_cloud_knn_options.  max_dist is judged as the float32 the struct holds."""
    nq, nt = _mesh_count("cloud_knn", n_queries), _mesh_count("cloud_knn", n_targets)
    for name, s in (("query_stride", query_stride), ("target_stride", target_stride)):
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 12 or s % 4:
            raise ValueError("cloud_knn: %s must be a multiple of 4 and at least 12" % name)
    _cloud_search_args("cloud_knn", k, max_dist)
    if not isinstance(exclude_self, (bool, np.bool_)):
        raise ValueError("cloud_knn: exclude_self must be a bool")
    if exclude_self and nq != nt:
        raise ValueError("cloud_knn: exclude_self needs as many queries as targets")
    _cloud_aliases("cloud_knn", inputs, outputs)
    return N.DpCloudKnnOptions(float(max_dist), int(k), N.CLOUD_KNN_EXCLUDE_SELF if exclude_self else 0)


def check_cloud_clean_args(n, k, max_dist, std_mul=2.0, min_neighbours=1, radius_only=False, stride=12, inputs=(),
                           outputs=()):
    """Argument validation of Engine.cloud_clean[_device] (the limits of
    dp_cloud_clean, raised as ValueError before any device call); returns the
    dp_cloud_clean_options.  max_dist and std_mul are judged as the float32 the
    struct holds."""
    _mesh_count("cloud_clean", n)
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 12 or stride % 4:
        raise ValueError("cloud_clean: stride must be a multiple of 4 and at least 12")
    _cloud_search_args("cloud_clean", k, max_dist)
    if isinstance(min_neighbours, bool) or not isinstance(min_neighbours, (int, np.integer)) or \
            not 1 <= min_neighbours <= k:
        raise ValueError("cloud_clean: min_neighbours must be in 1..k")
    with np.errstate(over="ignore"):
        if isinstance(std_mul, bool) or not isinstance(std_mul, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(np.float32(std_mul)) and np.float32(std_mul) >= 0):
            raise ValueError("cloud_clean: std_mul must be finite and >= 0")
    if not isinstance(radius_only, (bool, np.bool_)):
        raise ValueError("cloud_clean: radius_only must be a bool")
    _cloud_aliases("cloud_clean", inputs, outputs, among_outputs=True)
    return N.DpCloudCleanOptions(float(max_dist), int(k), int(min_neighbours), float(std_mul),
                                 N.CLOUD_CLEAN_RADIUS_ONLY if radius_only else 0)


def check_cloud_normals_args(n, k=16, max_dist=None, min_neighbours=3, orient=None, toward=False, toward_stride=0,
                             stride=12, inputs=(), outputs=()):
    """Argument validation of Engine.cloud_normals[_device] (the limits of
    dp_cloud_normals, raised as ValueError before any device call); returns the
    dp_cloud_normals_options.  orient is None, "viewpoint" or "direction";
    `toward` says whether the entries are given (required with an orient mode,
    refused without one) and toward_stride is 0 or a multiple of 4 that is at
    least 12.  max_dist is judged as the float32 the struct holds."""
    def whole(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

    _mesh_count("cloud_normals", n)
    if not whole(stride) or stride < 12 or stride % 4:
        raise ValueError("cloud_normals: stride must be a multiple of 4 and at least 12")
    _cloud_search_args("cloud_normals", k, max_dist)
    if k < 3:
        raise ValueError("cloud_normals: k must be in 3..32")
    if not whole(min_neighbours) or not 3 <= min_neighbours <= k:
        raise ValueError("cloud_normals: min_neighbours must be in 3..k")
    if orient not in (None, "viewpoint", "direction"):
        raise ValueError("cloud_normals: orient must be None, 'viewpoint' or 'direction'")
    if not whole(toward_stride):
        raise ValueError("cloud_normals: toward_stride must be a whole number")
    if orient is None:
        if toward or toward_stride != 0:
            raise ValueError("cloud_normals: toward and toward_stride need an orient mode")
    else:
        if not toward:
            raise ValueError("cloud_normals: an orient mode needs toward")
        if toward_stride != 0 and (toward_stride < 12 or toward_stride % 4):
            raise ValueError("cloud_normals: toward_stride must be 0 or a multiple of 4 and at least 12")
    _cloud_aliases("cloud_normals", inputs, outputs, among_outputs=True)
    flags = {None: 0, "viewpoint": N.CLOUD_NORMALS_ORIENT_VIEWPOINT, "direction": N.CLOUD_NORMALS_ORIENT_DIRECTION}
    return N.DpCloudNormalsOptions(float(max_dist), int(k), int(min_neighbours), flags[orient])


def _cloud_matrix(who: str, name: str, m) -> np.ndarray:
    """a 3 x 4 (or 12) array of finite numbers as contiguous float64"""
    try:
        a = np.array(m, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.size != 12 or a.shape not in ((3, 4), (12,)) or not np.isfinite(a).all():
        raise ValueError("%s: %s must be 3 x 4 finite numbers" % (who, name))
    return np.ascontiguousarray(a.reshape(3, 4))


def _cloud_normal_offset(who: str, a: np.ndarray, normals) -> int:
    """the byte offset of a structured cloud's normal field, -1 without normals"""
    if not isinstance(normals, (bool, np.bool_)):
        raise ValueError("%s: normals must be a bool" % who)
    if not normals:
        return -1
    if not a.dtype.names or "normal" not in a.dtype.names or a.dtype.fields["normal"][0] != np.dtype(("<f4", 3)):
        raise ValueError("%s: normals needs a structured cloud with a normal field of three float32" % who)
    return int(a.dtype.fields["normal"][1])


def check_cloud_transform_args(n, matrix, stride=12, normal_offset=-1) -> np.ndarray:
    """Argument validation of Engine.cloud_transform[_device] (the limits of
    dp_cloud_transform, raised as ValueError before any device call); returns
    the matrix as 3 x 4 float64."""
    def whole(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

    _mesh_count("cloud_transform", n)
    if not whole(stride) or stride < 12 or stride % 4:
        raise ValueError("cloud_transform: stride must be a multiple of 4 and at least 12")
    m = _cloud_matrix("cloud_transform", "matrix", matrix)
    if not whole(normal_offset) or (normal_offset != -1 and
                                    (normal_offset < 12 or normal_offset % 4 or normal_offset > stride - 12)):
        raise ValueError("cloud_transform: normal_offset must be -1 or a multiple of 4 in 12..stride - 12")
    return m


def check_cloud_align_args(n_source, n_target, max_dist, iterations=30, scale=False, init=None, rms_tol=0.0,
                           min_pairs=3, source_stride=12, target_stride=12, inputs=(), outputs=()):
    """Argument validation of Engine.cloud_align[_device] (the limits of
    dp_cloud_align, raised as ValueError before any device call); returns the
    dp_cloud_align_options and init as 3 x 4 float64 (None = the identity).
    max_dist is judged as the float32 the struct holds."""
    def whole(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)

    _mesh_count("cloud_align", n_source)
    _mesh_count("cloud_align", n_target)
    for name, s in (("source_stride", source_stride), ("target_stride", target_stride)):
        if not whole(s) or s < 12 or s % 4:
            raise ValueError("cloud_align: %s must be a multiple of 4 and at least 12" % name)
    with np.errstate(over="ignore"):
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(np.float32(max_dist)) and np.float32(max_dist) > 0):
            raise ValueError("cloud_align: max_dist must be finite and > 0")
    if not whole(iterations) or not 1 <= iterations <= 1000:
        raise ValueError("cloud_align: iterations must be in 1..1000")
    if not whole(min_pairs) or not 3 <= min_pairs <= 2**31 - 1:
        raise ValueError("cloud_align: min_pairs must be at least 3")
    if isinstance(rms_tol, bool) or not isinstance(rms_tol, (int, float, np.integer, np.floating)) or \
            not (np.isfinite(rms_tol) and rms_tol >= 0):
        raise ValueError("cloud_align: rms_tol must be finite and >= 0")
    if not isinstance(scale, (bool, np.bool_)):
        raise ValueError("cloud_align: scale must be a bool")
    m0 = None if init is None else _cloud_matrix("cloud_align", "init", init)
    _cloud_aliases("cloud_align", inputs, outputs)
    return N.DpCloudAlignOptions(float(max_dist), int(iterations), int(min_pairs),
                                 N.CLOUD_ALIGN_SCALE if scale else 0, float(rms_tol)), m0


ALIGN_KEYS = ("iterations", "max_dist", "scale", "init", "rms_tol", "min_pairs")


def check_compare_align(align, max_dist: float):
    """The `align` argument of cloud_compare, mesh_compare and PMVS.evaluate:
    None, or a dict of Engine.cloud_align's keyword arguments (iterations,
    max_dist -- by default the comparison's --, scale, init, rms_tol,
    min_pairs), judged by check_cloud_align_args.  Returns the completed dict."""
    if align is None:
        return None
    if not isinstance(align, dict) or not set(align) <= set(ALIGN_KEYS):
        raise ValueError("cloud_compare: align is a dict of " + ", ".join(ALIGN_KEYS))
    kw = dict(align)
    kw.setdefault("max_dist", max_dist)
    check_cloud_align_args(0, 0, **kw)
    return kw


def _compare_aligned(eng, cloud, truth, kw: dict):
    """registers `cloud` to `truth`: (the transformed cloud, the "align" entry)"""
    cloud = np.asarray(cloud)
    pos = np.ascontiguousarray(cloud["pos"] if cloud.dtype.names else cloud, dtype=np.float32).reshape(-1, 3)
    res = eng.cloud_align(pos, truth, **kw)
    moved = eng.cloud_transform(pos, res["matrix"])
    return moved, {"matrix": res["matrix"], "scale": res["scale"], "trace": res["trace"], "stats": res["stats"]}


def cloud_quantile(sorted_d: np.ndarray, p: float) -> float:
    """The p-quantile (0 <= p <= 1) of ascending fp64 values by linear
    interpolation between the two nearest ranks: pos = p * (m - 1), lo =
    floor(pos), d[lo] + (d[min(lo + 1, m - 1)] - d[lo]) * (pos - lo); NaN when
    there are none."""
    m = len(sorted_d)
    if m == 0:
        return float("nan")
    pos = p * (m - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, m - 1)
    return float(sorted_d[lo] + (sorted_d[hi] - sorted_d[lo]) * (pos - lo))


def cloud_side(nearest: dict, tau: float) -> dict:
    """One direction of cloud_compare from a cloud_nearest result: n (queries
    taking part), matched, within_tau (matched with dist <= tau), ratio =
    within_tau / n (0.0 when n is 0), and mean, median (the 0.5-quantile) and p90
    (cloud_quantile) of the matched float32 distances in fp64, NaN when none
    matched."""
    d = nearest["dist"][nearest["index"] >= 0].astype(np.float64)
    n, matched = int(nearest["stats"]["queries"]), int(nearest["stats"]["matched"])
    within = int(np.count_nonzero(d <= float(tau)))
    ds = np.sort(d)
    return {"n": n, "matched": matched, "within_tau": within, "ratio": within / n if n else 0.0,
            "mean": float(d.mean()) if len(d) else float("nan"), "median": cloud_quantile(ds, 0.5),
            "p90": cloud_quantile(ds, 0.9)}


def check_cloud_compare_args(tau, max_dist=None) -> float:
    """tau must be finite and > 0; max_dist (None = 10 * tau) at least tau.
    Returns max_dist."""
    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

    if not number(tau) or not (np.isfinite(tau) and tau > 0):
        raise ValueError("cloud_compare: tau must be finite and > 0")
    if max_dist is None:
        max_dist = 10.0 * float(tau)
    if not number(max_dist) or not (np.isfinite(max_dist) and max_dist >= tau):
        raise ValueError("cloud_compare: max_dist must be finite and at least tau")
    return float(max_dist)


def cloud_normal_error(recon_normals, truth_normals, index, dist, tau) -> dict:
    """The error of a reconstruction's normals against a truth's, over the
    matches of a cloud_nearest call (recon -> truth): query i counts iff index[i]
    >= 0, dist[i] <= tau, and its own normal a and the truth's normal b =
    truth_normals[index[i]] are both finite and not zero.  Its angle is the
    unsigned one, in degrees and fp64: with dot = (a.x * b.x + a.y * b.y) + a.z *
    b.z and |a| = sqrt((a.x * a.x + a.y * a.y) + a.z * a.z),
    degrees(arccos(min(1, |dot| / (|a| * |b|)))) -- a truth normal has no sign.
    Returns n, mean_deg, median_deg and p90_deg (cloud_quantile), NaN when n is 0."""
    a = np.asarray(recon_normals, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(truth_normals, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(index).reshape(-1)
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    if not (len(a) == len(index) == len(dist)):
        raise ValueError("cloud_normal_error: recon_normals, index and dist must have one entry per query")
    if len(index) and int(index.max()) >= len(t):
        raise ValueError("cloud_normal_error: index must point into truth_normals")
    with np.errstate(invalid="ignore"):
        ok = (index >= 0) & (dist <= float(tau))
    a = a[ok]
    b = t[index[ok]] if len(t) else np.zeros((0, 3))
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & (a != 0).any(axis=1) & (b != 0).any(axis=1)
    a, b = a[ok], b[ok]
    with np.errstate(over="ignore", invalid="ignore"):
        dot = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
        la = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        lb = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        deg = np.degrees(np.arccos(np.minimum(1.0, dot / (la * lb))))
    ds = np.sort(deg)
    return {"n": int(len(deg)), "mean_deg": float(deg.mean()) if len(deg) else float("nan"),
            "median_deg": cloud_quantile(ds, 0.5), "p90_deg": cloud_quantile(ds, 0.9)}


NORMALS_KEYS = ("k", "max_dist")


def check_compare_normals(normals, max_dist: float):
    """The `normals` argument of cloud_compare and PMVS.evaluate: None, or a dict
    of k (16 by default) and max_dist (by default the comparison's) for the
    Engine.cloud_normals call on the truth, judged by check_cloud_normals_args.
    Returns the completed dict."""
    if normals is None:
        return None
    if not isinstance(normals, dict) or not set(normals) <= set(NORMALS_KEYS):
        raise ValueError("cloud_compare: normals is a dict of " + ", ".join(NORMALS_KEYS))
    kw = dict(normals)
    kw.setdefault("k", 16)
    kw.setdefault("max_dist", max_dist)
    check_cloud_normals_args(0, **kw)
    return kw


def cloud_compare(eng, recon, truth, tau: float, max_dist=None, align=None, normals=None) -> dict:
    """Accuracy, completeness and F-score of a reconstructed cloud against a
    ground truth at the threshold tau, by two Engine.cloud_nearest calls with the
    radius max_dist (None = 10 * tau): accuracy is recon -> truth, completeness
    truth -> recon (each a cloud_side), fscore = 2pr / (p + r) of their ratios,
    0.0 when p + r is 0.  The clouds are what cloud_nearest takes.  align (a dict
    of Engine.cloud_align's iterations, max_dist, scale, init, rms_tol,
    min_pairs; max_dist defaults to the comparison's) first registers recon to
    truth, compares the transformed positions and adds "align": the matrix, the
    scale, the trace and the statistics of the registration.  normals (a dict of
    k = 16 and max_dist = the comparison's) needs recon records with a `normal`
    field (patches, FUSED_DTYPE): the truth's normals are estimated once by
    Engine.cloud_normals, and "normals" is the cloud_normal_error of the
    records' own normals over the accuracy direction's matches; with align the
    records are moved whole by cloud_transform(normals=True), so the normals
    turn with them."""
    max_dist = check_cloud_compare_args(tau, max_dist)
    kw = check_compare_align(align, max_dist)
    nkw = check_compare_normals(normals, max_dist)
    if nkw is not None:
        recon = np.asarray(recon)
        _cloud_normal_offset("cloud_compare", recon, True)
    extra = {}
    if kw is not None:
        moved, extra["align"] = _compare_aligned(eng, recon, truth, kw)
        recon = moved if nkw is None else eng.cloud_transform(recon, extra["align"]["matrix"], normals=True)
    near = eng.cloud_nearest(recon, truth, max_dist)
    acc = cloud_side(near, tau)
    com = cloud_side(eng.cloud_nearest(truth, recon, max_dist), tau)
    if nkw is not None:
        tn = eng.cloud_normals(truth, **nkw)["normal"]
        extra["normals"] = cloud_normal_error(recon["normal"], tn, near["index"], near["dist"], tau)
    p, r = acc["ratio"], com["ratio"]
    return dict({"accuracy": acc, "completeness": com, "fscore": 2.0 * p * r / (p + r) if p + r > 0 else 0.0}, **extra)


def _mesh_vertices(who: str, vertices) -> np.ndarray:
    """Mesh vertices as dp_mesh_vertex records: MESH_VERTEX_DTYPE as it is, an
    (n, 3) array as records with zero colours."""
    v = np.asarray(vertices)
    if v.dtype.names:
        return np.ascontiguousarray(v, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
    if v.size == 0:
        return np.zeros(0, N.MESH_VERTEX_DTYPE)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("%s: vertices must be MESH_VERTEX_DTYPE records or an n x 3 array" % who)
    out = np.zeros(len(v), N.MESH_VERTEX_DTYPE)
    out["pos"] = v
    return out


def check_mesh_nearest_args(n_queries, n_vertices, n_triangles, max_dist, hist_bins=0, query_stride=12, flags=0,
                            inputs=(), outputs=()):
    """Argument validation of Engine.mesh_nearest[_device] (the limits of
    dp_mesh_nearest, raised as ValueError before any device call); returns the
    dp_mesh_nearest_options.  The rules are check_cloud_nearest_args'."""
    try:
        _mesh_count("mesh_nearest", n_vertices)
        cno = check_cloud_nearest_args(n_queries, n_triangles, max_dist, hist_bins, query_stride, 12, flags, inputs,
                                       outputs)
    except ValueError as e:
        raise ValueError(str(e).replace("cloud_nearest", "mesh_nearest").replace("n_targets", "n_triangles")) from None
    return N.DpMeshNearestOptions(cno.max_dist, cno.hist_bins, cno.flags)


def mesh_compare(eng, vertices, triangles, truth, tau: float, max_dist=None, align=None) -> dict:
    """cloud_compare for a mesh: accuracy is the mesh's vertices -> the truth
    points (Engine.cloud_nearest, as for a cloud), completeness the truth points
    -> the mesh's surface (Engine.mesh_nearest), each a cloud_side, and fscore
    from their ratios as in cloud_compare.  align registers the mesh's vertices
    to the truth first, as in cloud_compare."""
    max_dist = check_cloud_compare_args(tau, max_dist)
    kw = check_compare_align(align, max_dist)
    verts = _mesh_vertices("mesh_compare", vertices)
    if kw is not None:
        moved, entry = _compare_aligned(eng, verts, truth, kw)
        verts = verts.copy()
        verts["pos"] = moved
        acc = cloud_side(eng.cloud_nearest(verts, truth, max_dist), tau)
        com = cloud_side(eng.mesh_nearest(truth, verts, triangles, max_dist), tau)
        p, r = acc["ratio"], com["ratio"]
        return {"accuracy": acc, "completeness": com, "fscore": 2.0 * p * r / (p + r) if p + r > 0 else 0.0,
                "align": entry}
    acc = cloud_side(eng.cloud_nearest(verts, truth, max_dist), tau)
    com = cloud_side(eng.mesh_nearest(truth, verts, triangles, max_dist), tau)
    p, r = acc["ratio"], com["ratio"]
    return {"accuracy": acc, "completeness": com, "fscore": 2.0 * p * r / (p + r) if p + r > 0 else 0.0}


def deviation_side(nearest: dict) -> dict:
    """One direction of mesh_deviation from a mesh_nearest result: n (queries
    taking part), matched, and mean, median, p90 (cloud_quantile) and max of the
    matched float32 distances in fp64, NaN when none matched."""
    d = np.sort(nearest["dist"][nearest["index"] >= 0].astype(np.float64))
    nan = float("nan")
    return {"n": int(nearest["stats"]["queries"]), "matched": int(nearest["stats"]["matched"]),
            "mean": float(d.mean()) if len(d) else nan, "median": cloud_quantile(d, 0.5), "p90": cloud_quantile(d, 0.9),
            "max": float(d[-1]) if len(d) else nan}


def mesh_deviation(eng, a, b, max_dist: float) -> dict:
    """How far two meshes a = (vertices, triangles) and b lie apart: the vertices
    of a against the surface of b ("a_to_b") and b's against a's ("b_to_a"), each
    a deviation_side of an Engine.mesh_nearest call with the radius max_dist, and
    "max", the larger of the two maxima (NaN when nothing matched either way).
    Vertices beyond max_dist of the other surface are unmatched and enter no
    figure but n - matched."""
    (va, ta), (vb, tb) = a, b
    va, vb = _mesh_vertices("mesh_deviation", va), _mesh_vertices("mesh_deviation", vb)
    ab = deviation_side(eng.mesh_nearest(va, vb, tb, max_dist))
    ba = deviation_side(eng.mesh_nearest(vb, va, ta, max_dist))
    tops = [s["max"] for s in (ab, ba) if not np.isnan(s["max"])]
    return {"a_to_b": ab, "b_to_a": ba, "max": max(tops) if tops else float("nan")}


def _stats_dict(st) -> dict:
    return {name: getattr(st, name) for name, _ in st._fields_}


def _mesh_entries(who: str, nt: int) -> None:
    if 6 * nt > 2**31 - 1:
        raise ValueError("%s: 6 * n_triangles must be <= 2^31 - 1" % who)


def _mesh_pairs(who: str, nt: int) -> None:
    if 3 * nt > 2**31 - 1:
        raise ValueError("%s: 3 * n_triangles must be <= 2^31 - 1" % who)


def check_mesh_decimate_args(cell, origin=(0.0, 0.0, 0.0), quadric=False):
    """Argument validation of Engine.mesh_decimate[_device] (the limits of
    dp_mesh_decimate_options, raised as ValueError before any device call);
    returns the dp_mesh_decimate_options.  The values are judged as the float32
    the struct holds."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))

    with np.errstate(over="ignore"):
        if not real(cell) or not (np.isfinite(np.float32(cell)) and np.float32(cell) > 0):
            raise ValueError("mesh_decimate: cell must be finite and > 0")
        try:
            org = tuple(origin)
        except TypeError:
            org = ()
        if len(org) != 3 or not all(real(o) and np.isfinite(np.float32(o)) for o in org):
            raise ValueError("mesh_decimate: origin must be three finite numbers")
    if not isinstance(quadric, (bool, np.bool_)):
        raise ValueError("mesh_decimate: quadric must be a bool")
    return N.DpMeshDecimateOptions((ctypes.c_float * 3)(*(float(o) for o in org)), float(cell),
                                   N.DP_DECIMATE_QUADRIC if quadric else N.DP_DECIMATE_MEAN, 0, 0)


def check_mesh_render_args(n_vertices, n_triangles, V: int, views=None, cull_back=False):
    """Argument validation of Engine.mesh_render[_device] (the limits of
    dp_mesh_render, raised as ValueError before any device call); returns
    (dp_mesh_render_options, view ids as int32)."""
    _mesh_count("mesh_render", n_vertices)
    _mesh_count("mesh_render", n_triangles)
    if not isinstance(cull_back, (bool, np.bool_)):
        raise ValueError("mesh_render: cull_back must be a bool")
    vid = _check_view_ids("mesh_render", V, views, cap=None)
    return (N.DpMeshRenderOptions(N.DP_MESH_RENDER_CULL_BACK if cull_back else 0),
            np.ascontiguousarray(vid, dtype=np.int32))


def check_mesh_colour_args(n_vertices, V: int, views=None, depth=None, depth_tol=0.01, min_cos=0.2, bilinear=False,
                           clear_unseen=False, inputs=(), outputs=()):
    """Argument validation of Engine.mesh_colour[_device] (the limits of
    dp_mesh_colour, raised as ValueError before any device call); returns
    (dp_mesh_colour_options, view ids as int32).  `depth`: the planes or their
    addresses, one per view and none of them None or 0 (None here: not checked,
    Engine.mesh_colour renders them); `inputs` and `outputs`: the device form's
    addresses, of which no output may equal an input or a plane."""
    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

    _mesh_count("mesh_colour", n_vertices)
    if not (number(depth_tol) and 0 <= depth_tol <= 3.4028234663852886e38):
        raise ValueError("mesh_colour: depth_tol must be finite and >= 0")
    if not (number(min_cos) and 0 <= min_cos <= 1):
        raise ValueError("mesh_colour: min_cos must be in 0..1")
    if not isinstance(bilinear, (bool, np.bool_)) or not isinstance(clear_unseen, (bool, np.bool_)):
        raise ValueError("mesh_colour: bilinear and clear_unseen must be bools")
    vid = _check_view_ids("mesh_colour", V, views)
    planes = []
    if depth is not None:
        planes = list(depth)
        if len(planes) != len(vid) or any(p is None or (isinstance(p, (int, np.integer)) and not p) for p in planes):
            raise ValueError("mesh_colour: one depth plane per view, none of them missing")
    ins = [a for a in list(inputs) + planes if isinstance(a, (int, np.integer)) and a]
    if any(isinstance(o, (int, np.integer)) and o and o in ins for o in outputs):
        raise ValueError("mesh_colour: an output equals an input")
    flags = (N.DP_MESH_COLOUR_BILINEAR if bilinear else 0) | (N.DP_MESH_COLOUR_CLEAR_UNSEEN if clear_unseen else 0)
    return N.DpMeshColourOptions(float(depth_tol), float(min_cos), flags), np.ascontiguousarray(vid, dtype=np.int32)


def _colour_on_device(eng, device: int, verts, tris, normals, colour: dict):
    """PMVS.mesh's last stage: the host mesh uploaded once, rendered into the
    views of `colour` and coloured there (mesh_render_device, then
    mesh_colour_device on the planes it left); returns (vertices, stats)."""
    import torch

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    nv, nt = len(verts), len(tris)
    _, vid = check_mesh_colour_args(nv, eng.num_views(), colour.get("views"))
    dev = torch.device("cuda", device)
    d_verts, d_tris = up(verts), up(tris)
    d_nrm = up(normals) if normals is not None else None
    d_out = torch.empty(max(nv, 1) * N.MESH_VERTEX_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    depth = [torch.empty((h, w), dtype=torch.float32, device=dev) for w, h in eng.view_sizes(vid)]
    torch.cuda.synchronize(dev)
    planes = [t.data_ptr() for t in depth]
    eng.mesh_render_device(d_verts.data_ptr() if nv else 0, nv, d_tris.data_ptr() if nt else 0, nt, vid, planes,
                           stats=False)
    st = eng.mesh_colour_device(d_verts.data_ptr() if nv else 0, nv, vid, planes, d_out.data_ptr() if nv else 0,
                                d_normals=d_nrm.data_ptr() if d_nrm is not None and nv else 0,
                                **{k: v for k, v in colour.items() if k != "views"})
    out = d_out[:nv * N.MESH_VERTEX_DTYPE.itemsize].cpu().numpy().view(N.MESH_VERTEX_DTYPE).copy()
    return out, st


def decimate_cell(decimate, voxel) -> dict:
    """PMVS.mesh's `decimate` dict as Engine.mesh_decimate's options without the
    origin: `cell` in world units, or `factor` times the volume's voxel (the
    float32 the volume holds; the product rounded to float32 once), and
    optionally `quadric`."""
    d = dict(decimate)
    unknown = set(d) - {"cell", "factor", "quadric", "origin"}
    if unknown:
        raise ValueError("mesh: unknown decimate options %s" % sorted(unknown))
    if ("cell" in d) == ("factor" in d):
        raise ValueError("mesh: decimate takes either cell or factor")
    if "factor" in d:
        f = d.pop("factor")
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not (np.isfinite(f) and f > 0):
            raise ValueError("mesh: decimate's factor must be finite and > 0")
        with np.errstate(over="ignore"):
            d["cell"] = float(np.float32(float(f) * float(np.float32(voxel))))
    return d


def check_mesh_smooth_args(iterations=10, lam=0.5, mu=-0.53, free_boundary=False):
    """Argument validation of Engine.mesh_smooth[_device] (the limits of
    dp_mesh_smooth_options, raised as ValueError before any device call); returns
    the dp_mesh_smooth_options.  lam is the struct's lambda."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))

    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= 1000:
        raise ValueError("mesh_smooth: iterations must be a whole number in 0..1000")
    if not real(lam) or not 0.0 < float(np.float32(lam)) <= 1.0:
        raise ValueError("mesh_smooth: lam must be in (0, 1]")
    if not real(mu) or not float(np.float32(mu)) <= 0.0 or np.isinf(np.float32(mu)):
        raise ValueError("mesh_smooth: mu must be finite and <= 0")
    if not isinstance(free_boundary, (bool, np.bool_)):
        raise ValueError("mesh_smooth: free_boundary must be a bool")
    return N.DpMeshSmoothOptions(int(iterations), float(lam), float(mu),
                                 N.DP_SMOOTH_FREE_BOUNDARY if free_boundary else 0, 0)


def _addr(a):
    return ctypes.c_void_p(a) if a else None


def _mesh_clean_stats(st) -> dict:
    return {name: getattr(st, name) for name, _ in N.DpMeshCleanStats._fields_}


def _mesh_count(who: str, n) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 2**31 - 1:
        raise ValueError("%s: a count must be a whole number in 0..2^31 - 1" % who)
    return int(n)


def _mesh_cap(who: str, cap, buf) -> None:
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0 or (cap > 0 and not buf):
        raise ValueError("%s: a cap must be >= 0, with its buffer given when > 0" % who)


def _mesh_triangles(who: str, triangles) -> np.ndarray:
    tris = np.asarray(triangles)
    if tris.size == 0:
        return np.zeros((0, 3), np.int32)
    if tris.ndim != 2 or tris.shape[1] != 3 or not np.issubdtype(tris.dtype, np.integer):
        raise ValueError("%s: triangles must be an n x 3 integer array" % who)
    if tris.dtype != np.int32 and ((tris < -2**31).any() or (tris > 2**31 - 1).any()):
        raise ValueError("%s: a triangle index does not fit int32" % who)
    return np.ascontiguousarray(tris, dtype=np.int32)


def _check_view_ids(who: str, V: int, views, cap=64):
    """The `views` argument of a map stage (None = all V): 1..cap ids (cap None:
    at least one), unique and < V, raised as ValueError; returns them as int64."""
    vid = np.arange(V, dtype=np.int64) if views is None else np.asarray(list(views), dtype=np.int64)
    if cap is None and (vid.ndim != 1 or len(vid) == 0):
        raise ValueError("%s: no views" % who)
    if cap is not None and (vid.ndim != 1 or not 1 <= len(vid) <= cap):
        raise ValueError("%s: 1..%d views" % (who, cap))
    if (vid < 0).any() or (vid >= V).any() or len(set(vid.tolist())) != len(vid):
        raise ValueError("%s: view ids must be unique and < %d" % (who, V))
    return vid


def check_mesh_clean_args(min_triangles=1, min_fraction=0.0, max_components=0):
    """Argument validation of Engine.mesh_clean[_device] (the limits of
    dp_mesh_clean_options, raised as ValueError before any device call); returns
    the dp_mesh_clean_options."""
    def whole(x, hi):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= int(x) <= hi

    if not whole(min_triangles, 2**63 - 1):
        raise ValueError("mesh_clean: min_triangles must be a whole number >= 0")
    if (isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating))
            or not 0.0 <= float(np.float32(min_fraction)) <= 1.0):
        raise ValueError("mesh_clean: min_fraction must be in 0..1")
    if not whole(max_components, 2**31 - 1):
        raise ValueError("mesh_clean: max_components must be a whole number in 0..2^31 - 1")
    return N.DpMeshCleanOptions(int(min_triangles), float(min_fraction), int(max_components), 0, 0)


def check_tsdf_args(V: int, views, origin, voxel, dim, trunc, min_weight: int = 1):
    """Argument validation of Engine.tsdf_integrate[_device] and tsdf_mesh[_device]
    (the limits of dp_tsdf_options and the view rules of dp_tsdf_integrate,
    raised as ValueError before any device call); returns (dp_tsdf_options, view
    ids as int32)."""
    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

    def f32(x):
        with np.errstate(over="ignore"):
            return float(np.float32(x))

    try:
        origin = tuple(origin)
    except TypeError:
        origin = ()
    if len(origin) != 3 or not all(number(c) and np.isfinite(f32(c)) for c in origin):
        raise ValueError("tsdf: origin must be three finite numbers")
    if not (number(voxel) and np.isfinite(f32(voxel)) and f32(voxel) > 0):
        raise ValueError("tsdf: voxel must be finite and > 0")
    if not (number(trunc) and np.isfinite(f32(trunc)) and f32(trunc) > 0):
        raise ValueError("tsdf: trunc must be finite and > 0")
    try:
        dim = tuple(dim)
    except TypeError:
        dim = ()
    if len(dim) != 3 or not all(number(d) and int(d) == d and 2 <= int(d) <= 1024 for d in dim):
        raise ValueError("tsdf: dim must be three sizes in 2..1024")
    if int(dim[0]) * int(dim[1]) * int(dim[2]) > 2**30:
        raise ValueError("tsdf: at most 2^30 voxels")
    if not (number(min_weight) and int(min_weight) == min_weight and 1 <= int(min_weight) <= 64):
        raise ValueError("tsdf: min_weight must be in 1..64")
    vid = _check_view_ids("tsdf", V, views)
    to = N.DpTsdfOptions((ctypes.c_float * 3)(*[float(c) for c in origin]), float(voxel),
                         (ctypes.c_int32 * 3)(*[int(d) for d in dim]), float(trunc), int(min_weight), 0)
    return to, np.ascontiguousarray(vid, dtype=np.int32)


def mesh_volume(positions: np.ndarray, voxel=None, dim: int = 256, trunc=None) -> dict:
    """The volume PMVS.mesh integrates into: the bounding box of `positions`
    (n x 3) padded by trunc on every side.  voxel defaults to the box's longest
    side / dim, trunc to 4 * voxel; the sizes are ceil(padded side / voxel),
    clipped to 2..1024.  Returns dict(origin, voxel, dim, trunc)."""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    pos = pos[np.isfinite(pos).all(axis=1)]
    if len(pos) == 0:
        raise ValueError("mesh: no patch positions to bound the volume")
    if isinstance(dim, bool) or int(dim) != dim or not 2 <= int(dim) <= 1024:
        raise ValueError("mesh: dim must be in 2..1024")
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    if voxel is None:
        voxel = float((hi - lo).max()) / int(dim)
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("mesh: voxel must be finite and > 0 (a single point bounds no volume: give voxel)")
    if trunc is None:
        trunc = 4.0 * voxel
    if not (np.isfinite(trunc) and trunc > 0):
        raise ValueError("mesh: trunc must be finite and > 0")
    sizes = np.ceil((hi - lo + 2.0 * trunc) / voxel)
    return dict(origin=tuple(float(c) for c in lo - trunc), voxel=float(voxel),
                dim=tuple(int(min(max(s, 2), 1024)) for s in sizes), trunc=float(trunc))


MAPREF_DEFAULTS = dict(window=7, sweep=2, step_px=1.0, reach=(1, 4), max_sources=4, top_k=2, min_ncc=0.5,
                       keep_unscored=False)


def check_mapref_args(V: int, views=None, sources=None, **options):
    """Argument validation of Engine.refine_maps[_device] (the limits of
    dp_refine_maps, raised as ValueError before any device call); returns
    (dp_mapref_options, view ids as int32, the sources table as K x max_sources
    int32 or None)."""
    unknown = set(options) - set(MAPREF_DEFAULTS)
    if unknown:
        raise ValueError("refine_maps: unknown options %s" % sorted(unknown))
    o = dict(MAPREF_DEFAULTS, **options)

    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

    def whole(x, lo, hi):
        return number(x) and int(x) == x and lo <= int(x) <= hi

    if not (whole(o["window"], 3, 11) and int(o["window"]) % 2 == 1):
        raise ValueError("refine_maps: window must be odd and in 3..11")
    if not whole(o["sweep"], 0, 8):
        raise ValueError("refine_maps: sweep must be in 0..8")
    if not (number(o["step_px"]) and np.isfinite(o["step_px"]) and o["step_px"] > 0):
        raise ValueError("refine_maps: step_px must be finite and > 0")
    reach = o["reach"]
    if not (isinstance(reach, (tuple, list)) and len(reach) == 2 and all(whole(d, 0, 16) for d in reach)):
        raise ValueError("refine_maps: reach must be two distances in 0..16")
    if not whole(o["max_sources"], 1, 8):
        raise ValueError("refine_maps: max_sources must be in 1..8")
    if not whole(o["top_k"], 1, int(o["max_sources"])):
        raise ValueError("refine_maps: top_k must be in 1..max_sources")
    if not (number(o["min_ncc"]) and -1 <= o["min_ncc"] <= 1):
        raise ValueError("refine_maps: min_ncc must be in -1..1")
    vid = _check_view_ids("refine_maps", V, views)
    src = None
    if sources is not None:
        ms = int(o["max_sources"])
        rows = [list(r) for r in sources]
        if len(rows) != len(vid):
            raise ValueError("refine_maps: one sources row per view")
        src = np.full((len(vid), ms), -1, dtype=np.int32)
        for k, row in enumerate(rows):
            while row and row[-1] == -1:
                row.pop()
            if len(row) > ms:
                raise ValueError("refine_maps: a sources row holds more than max_sources ids")
            ids = [int(s) for s in row]
            if any(s not in vid.tolist() or s == int(vid[k]) for s in ids) or len(set(ids)) != len(ids):
                raise ValueError("refine_maps: a sources row must hold requested views other than its own, "
                                 "without repeats")
            src[k, :len(ids)] = ids
    mo = N.DpMaprefOptions(int(o["window"]), int(o["sweep"]), float(o["step_px"]),
                           (ctypes.c_int32 * 2)(int(reach[0]), int(reach[1])), int(o["max_sources"]), int(o["top_k"]),
                           float(o["min_ncc"]), N.MAPREF_KEEP_UNSCORED if o["keep_unscored"] else 0)
    return mo, np.ascontiguousarray(vid, dtype=np.int32), src


def split_refine_args(who: str, refine, kw: dict):
    """(passes, the dp_refine_maps options among kw, the rest of kw) for
    PMVS.depth_maps / fused_cloud; the options need refine > 0"""
    if isinstance(refine, bool) or int(refine) != refine or not 0 <= int(refine) <= 64:
        raise ValueError("%s: refine must be a pass count in 0..64" % who)
    names = set(MAPREF_DEFAULTS) | {"sources"}
    mkw = {k: v for k, v in kw.items() if k in names}
    if mkw and not refine:
        raise ValueError("%s: %s given without refine > 0" % (who, sorted(mkw)))
    return int(refine), mkw, {k: v for k, v in kw.items() if k not in names}


def check_fuse_args(V: int, views, depth_tol: float, min_views: int, min_normal_cos: float, suppress: bool):
    """Argument validation of Engine.fuse_maps[_device] (the limits of
    dp_fuse_maps, raised as ValueError before any device call); returns
    (dp_fuse_options, view ids as int32)."""
    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

    if not (number(depth_tol) and np.isfinite(depth_tol) and depth_tol >= 0):
        raise ValueError("fuse_maps: depth_tol must be finite and >= 0")
    if not (number(min_views) and int(min_views) == min_views and 0 <= int(min_views) <= 63):
        raise ValueError("fuse_maps: min_views must be in 0..63")
    if not (number(min_normal_cos) and 0 <= min_normal_cos <= 1):
        raise ValueError("fuse_maps: min_normal_cos must be in 0..1")
    vid = _check_view_ids("fuse_maps", V, views)
    fo = N.DpFuseOptions(float(depth_tol), int(min_views), float(min_normal_cos), 0 if suppress else N.FUSE_NO_SUPPRESS)
    return fo, np.ascontiguousarray(vid, dtype=np.int32)


def check_render_args(n: int, V: int, views, keep, splat_scale: float, max_radius_px: int, all_facing: bool):
    """Argument validation of Engine.render_maps[_device] (the limits of
    dp_render_maps, raised as ValueError before any device call); returns
    (dp_render_options, view ids as int32, keep as uint8 or None)."""
    if not 0 <= n <= 2**31 - 1:
        raise ValueError("render_maps: at most 2^31 - 1 patches")
    if not (isinstance(splat_scale, (int, float)) and splat_scale > 0 and np.isfinite(splat_scale)):
        raise ValueError("render_maps: splat_scale must be > 0")
    if int(max_radius_px) != max_radius_px or not 1 <= int(max_radius_px) <= 255:
        raise ValueError("render_maps: max_radius_px must be in 1..255")
    vid = _check_view_ids("render_maps", V, views, cap=None)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != (n,):
            raise ValueError("render_maps: one keep flag per patch")
    ro = N.DpRenderOptions(float(splat_scale), int(max_radius_px), N.RENDER_ALL_FACING if all_facing else 0)
    return ro, np.ascontiguousarray(vid, dtype=np.int32), keep


def write_pfm(path: str, array: np.ndarray) -> None:
    """Little-endian PFM ("Pf" 1 channel, "PF" 3 channels; scale -1.0), rows
    stored bottom-up as the format requires."""
    a = np.asarray(array, dtype=np.float32)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("write_pfm: H x W or H x W x 3 expected")
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.0\n" % (b"PF" if a.ndim == 3 else b"Pf", a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def read_pfm(path: str) -> np.ndarray:
    """A PFM written by write_pfm or any conforming writer (either byte order),
    as an H x W (x 3) float32 array with row 0 at the top."""
    with open(path, "rb") as f:
        data = f.read()
    parts, pos = [], 0
    while len(parts) < 4:  # magic, width, height, scale: whitespace-separated
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        parts.append(data[pos:end])
        pos = end
    pos += 1  # the single whitespace byte after the scale
    if parts[0] not in (b"PF", b"Pf"):
        raise ValueError("read_pfm: not a PFM file")
    ch = 3 if parts[0] == b"PF" else 1
    w, h, scale = int(parts[1]), int(parts[2]), float(parts[3])
    a = np.frombuffer(data, dtype="<f4" if scale < 0 else ">f4", count=w * h * ch, offset=pos)
    a = a.reshape((h, w, 3) if ch == 3 else (h, w))[::-1]
    return np.ascontiguousarray(a, dtype=np.float32)


def check_iterations(iterations: int, filter_passes: int) -> int:
    """the rounds of an iterated densify (PMVS.run, dist.densify_partitioned*):
    1..16, and more than one only with a filter, which is what tells them apart"""
    iterations = int(iterations)
    if not 1 <= iterations <= 16:
        raise ValueError("iterations must be in 1..16")
    if iterations > 1 and not filter_passes:
        raise ValueError("iterations > 1 needs filter_passes != 0 (the filter separates the rounds)")
    return iterations


class PMVS:
    """PMVS::PMVS (methods/pmvs/pmvs.h:14-35): AddCamera, Run, GetPointCloud.

    Seed points come from the caller (feature matching is out of scope; the
    reference's Matcher::GenerateSeeds output is just a list of 3-D points).
    """

    def __init__(self, options: Options | None = None, device: int = 0, fast: FastOptions | None = None):
        """fast: FastOptions with densify = 1 runs the whole loop in performance
        mode (no reference counterpart; dp_fast_options.densify)"""
        self.options = options or Options()
        self.device = device
        self.fast = fast
        self.views: list[View] = []
        self.patches = empty_patches(0)
        self.stats: dict = {}
        self._ran = False

    def add_camera(self, view: View) -> None:
        # PMVS::AddCamera (pmvs.cpp:11-20): views whose image failed to load are dropped
        if view.image is None or view.image.size == 0:
            return
        self.views.append(view)

    def run(self, seeds_xyz=None, filter_passes: int = 0, matcher_options=None, iterations: int = 1) -> bool:
        """PMVS::Run (pmvs.cpp:22-43).  With seeds_xyz None the seeds come from
        Matcher::GenerateSeeds on the device (PMVS::InsertSeeds, pmvs.cpp:29-34);
        filter_passes != 0 then applies FilterPatches (pmvs.h:27; spec in
        dp_filter_patches).  iterations > 1 alternates expansion and filter that
        many times (dp_densify_iterate: each round re-expands from the previous
        round's survivors); the filter is what tells the rounds apart, so it
        needs filter_passes != 0."""
        from .matcher import Matcher

        iterations = check_iterations(iterations, filter_passes)

        with Engine(self.options, self.device) as eng:
            eng.set_views(self.views)
            if self.fast is not None:
                eng.set_fast_options(self.fast)
            seed_stats = None
            if seeds_xyz is None:
                m = Matcher(eng, matcher_options)
                seeds_xyz = m.generate_seeds()
                seed_stats = m.stats
            if iterations > 1:
                self.patches, self.stats = eng.densify_iterate(np.asarray(seeds_xyz, dtype=np.float64), iterations,
                                                               filter_passes)
                self.stats["filtered_out"] = int(sum(r["filtered_out"] for r in self.stats["iterations"]))
                if seed_stats is not None:
                    self.stats["seed_generation"] = seed_stats
                self._ran = True
                return True
            self.patches, self.stats = eng.densify(np.asarray(seeds_xyz, dtype=np.float64))
            if seed_stats is not None:
                self.stats["seed_generation"] = seed_stats
            if filter_passes:
                keep = eng.filter_patches(self.patches, filter_passes)
                self.stats["filtered_out"] = int(len(keep) - keep.sum())
                self.patches = self.patches[keep == 1]
        self._ran = True
        return True

    def get_point_cloud(self) -> np.ndarray:
        return self.patches

    def depth_maps(self, refine: int = 0, **kw) -> dict:
        """Per-view depth / index (and normal, score) maps of the last run()'s
        result -- the survivors after run(iterations=N) or filter_passes != 0 --
        by Engine.render_maps, whose keyword arguments pass through.  refine = N
        > 0 runs N passes of Engine.refine_maps on the rendered planes (its
        options -- window, sweep, ..., sources -- pass through too): "depth",
        "normal" and "score" are then the refined planes, "choice" the last
        pass's, "index" still names the rendered patch, and "refine_stats" lists
        each pass's statistics."""
        if not self._ran:
            raise ValueError("depth_maps: call run() first")
        refine, mkw, kw = split_refine_args("depth_maps", refine, kw)
        with Engine(self.options, self.device) as eng:
            eng.set_views(self.views)
            if not refine:
                return eng.render_maps(self.patches, **kw)
            check_mapref_args(eng.num_views(), kw.get("views"), **mkw)
            out = eng.render_maps(self.patches, **dict(kw, normals=True))
            out["refine_stats"] = []
            for _ in range(refine):
                ref = eng.refine_maps(out["depth"], out["normal"], views=out["views"], **mkw)
                for key in ("depth", "normal", "score", "choice"):
                    out[key] = ref[key]
                out["refine_stats"].append(ref["stats"])
            return out

    def fused_cloud(self, views=None, splat_scale: float = 1.0, max_radius_px: int = 32, all_facing: bool = False,
                    normals: bool = True, refine: int = 0, clean=None, **fuse_kw) -> np.ndarray:
        """The last run()'s result as a dense fused cloud (a FUSED_DTYPE array):
        its depth and normal maps rendered on the device (Engine.render_maps_device)
        and fused there (Engine.fuse_maps_device, whose keyword arguments pass
        through) -- the planes never visit the host.  refine = N > 0 runs N
        passes of Engine.refine_maps_device between the two (its options pass
        through; it needs normals).  clean = dict(k=8, max_dist=R, std_mul=2.0,
        min_neighbours=1, radius_only=False) removes the outliers of the fused
        cloud on the device (Engine.cloud_clean_device; max_dist is required)
        and returns the cleaned cloud.  The statistics of the calls are left in
        self.stats["render"], self.stats["refine"] (a list), self.stats["fused"]
        and self.stats["cloud_clean"]."""
        if not self._ran:
            raise ValueError("fused_cloud: call run() first")
        if clean is not None:
            if not isinstance(clean, dict) or "max_dist" not in clean or \
                    set(clean) - {"k", "max_dist", "std_mul", "min_neighbours", "radius_only"}:
                raise ValueError("fused_cloud: clean is a dict of k, max_dist (required), std_mul, min_neighbours "
                                 "and radius_only")
            clean = dict(dict(k=8), **clean)
            check_cloud_clean_args(0, stride=FUSED_DTYPE.itemsize, **clean)
        refine, mkw, fuse_kw = split_refine_args("fused_cloud", refine, fuse_kw)
        if refine and not normals:
            raise ValueError("fused_cloud: refine needs normals")
        import torch

        with Engine(self.options, self.device) as eng:
            eng.set_views(self.views)
            if refine:
                check_mapref_args(eng.num_views(), views, **mkw)
            _, vid = check_fuse_args(eng.num_views(), views, fuse_kw.get("depth_tol", 0.01),
                                     fuse_kw.get("min_views", 2), fuse_kw.get("min_normal_cos", 0.5),
                                     fuse_kw.get("suppress", True))
            dev = torch.device("cuda", self.device)
            pat = torch.from_numpy(np.ascontiguousarray(self.patches).view(np.uint8).reshape(-1).copy()).to(dev)
            depth = [torch.empty((h, w), dtype=torch.float32, device=dev) for w, h in eng.view_sizes(vid)]
            normal = [torch.empty((h, w, 3), dtype=torch.float32, device=dev) for w, h in eng.view_sizes(vid)]
            torch.cuda.synchronize(dev)
            rst = eng.render_maps_device(pat.data_ptr() if len(self.patches) else 0, len(self.patches), None, vid,
                                         [t.data_ptr() for t in depth], None,
                                         [t.data_ptr() for t in normal] if normals else None,
                                         splat_scale=splat_scale, max_radius_px=max_radius_px, all_facing=all_facing)
            # an empty pixel is never emitted: the covered pixels bound the cloud
            cap = int(rst["covered_pixels"])
            mst = []
            for _ in range(refine):
                depth2 = [torch.empty_like(t) for t in depth]
                normal2 = [torch.empty_like(t) for t in normal]
                torch.cuda.synchronize(dev)
                mst.append(eng.refine_maps_device(vid, [t.data_ptr() for t in depth], [t.data_ptr() for t in normal],
                                                  [t.data_ptr() for t in depth2], [t.data_ptr() for t in normal2],
                                                  **mkw))
                depth, normal = depth2, normal2
                cap = int(mst[-1]["kept"])
            if refine:
                self.stats["refine"] = mst
            pts = torch.empty((max(cap, 1), FUSED_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            n, fst = eng.fuse_maps_device(vid, [t.data_ptr() for t in depth],
                                          [t.data_ptr() for t in normal] if normals else None, pts.data_ptr(), cap,
                                          **fuse_kw)
            if clean is not None:
                keep = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
                kept = torch.empty_like(pts)
                n_out = torch.zeros(1, dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                self.stats["cloud_clean"] = eng.cloud_clean_device(pts.data_ptr() if n else 0, n, FUSED_DTYPE.itemsize,
                                                                   d_keep=keep.data_ptr(), d_out=kept.data_ptr(),
                                                                   d_n_out=n_out.data_ptr(), **clean)
                pts, n = kept, int(n_out.item())
            out = pts[:n].cpu().numpy().reshape(-1).view(FUSED_DTYPE).copy()
        self.stats["render"], self.stats["fused"] = rst, fst
        return out

    def mesh(self, refine: int = 0, voxel=None, dim: int = 256, trunc=None, min_weight: int = 2, clean=None,
             smooth=None, normals: bool = False, decimate=None, colour=None, **kw):
        """The last run()'s result as a triangle mesh: (vertices as a
        MESH_VERTEX_DTYPE array, triangles as n x 3 int32).  The depth maps of
        depth_maps(refine, **kw) -- kw: its render and refinement options --
        are integrated into one TSDF volume (Engine.tsdf_integrate) around the
        patches (mesh_volume: their bounding box padded by trunc; voxel defaults
        to its longest side / dim, trunc to 4 * voxel) and the volume's zero
        surface is extracted (Engine.tsdf_mesh) over the voxels that at least
        min_weight views observed.  clean: a dict of Engine.mesh_clean's options
        (min_triangles, min_fraction, max_components) drops the mesh's small
        components; None (the default) leaves the mesh as extracted.  smooth: a
        dict of Engine.mesh_smooth's options (iterations, lam, mu,
        free_boundary) relaxes the vertex positions after the clean-up; None
        leaves them.  decimate: a dict with either cell (world units) or factor
        (cell = factor x the volume's voxel), and optionally quadric and origin
        (default: the volume's origin), simplifies the mesh after the smoothing
        (Engine.mesh_decimate); None leaves it.  normals=True returns (vertices, triangles, normals), the
        normals (Engine.mesh_normals, n x 3 float32) of the mesh as returned.
        colour: a dict of Engine.mesh_colour's options (views, depth_tol,
        min_cos, bilinear, clear_unseen) replaces the vertex colours, as the
        last stage, by the colours of the views that see each vertex: the mesh
        as returned is rendered into the views and coloured on the device
        (Engine.mesh_render_device, Engine.mesh_colour_device), with the normals
        as weights when normals=True; None leaves the TSDF's colours.
        The volume and the statistics of the calls are left in
        self.stats["mesh"] (the later stages' under "clean", "smooth",
        "decimate" and "normals"), the colouring's in self.stats["mesh_colour"]."""
        if not self._ran:
            raise ValueError("mesh: call run() first")
        if clean is not None:
            check_mesh_clean_args(**dict(clean))
        if smooth is not None:
            check_mesh_smooth_args(**dict(smooth))
        if colour is not None:
            colour = dict(colour)
            check_mesh_colour_args(0, max(len(self.views), 1), colour.get("views"), None,
                                   **{k: v for k, v in colour.items() if k != "views"})
        refine, mkw, kw = split_refine_args("mesh", refine, kw)
        vol = mesh_volume(self.patches["pos"], voxel, dim, trunc)
        if decimate is not None:
            decimate = dict(dict(origin=vol["origin"]), **decimate_cell(decimate, vol["voxel"]))
            check_mesh_decimate_args(**decimate)
        check_tsdf_args(max(len(self.views), 1), kw.get("views"), min_weight=min_weight, **vol)
        with Engine(self.options, self.device) as eng:
            eng.set_views(self.views)
            maps = eng.render_maps(self.patches, **dict(kw, normals=bool(refine) or kw.get("normals", False)))
            for _ in range(refine):
                ref = eng.refine_maps(maps["depth"], maps["normal"], views=maps["views"], **mkw)
                maps["depth"], maps["normal"] = ref["depth"], ref["normal"]
            volume = eng.tsdf_integrate(maps["depth"], maps["views"], **vol)
            verts, tris, mst = eng.tsdf_mesh(volume, min_weight)
            if clean is not None:
                verts, tris, cst = eng.mesh_clean(verts, tris, **dict(clean))
            if smooth is not None:
                verts, sst = eng.mesh_smooth(verts, tris, **dict(smooth))
            if decimate is not None:
                verts, tris, dst = eng.mesh_decimate(verts, tris, **decimate)
            if normals:
                nrm, nst = eng.mesh_normals(verts, tris)
            if colour is not None:
                verts, self.stats["mesh_colour"] = _colour_on_device(eng, self.device, verts, tris,
                                                                     nrm if normals else None, colour)
        self.stats["mesh"] = dict(vol, min_weight=int(min_weight), integrate=volume["stats"], mesh=mst)
        if clean is not None:
            self.stats["mesh"]["clean"] = cst
        if smooth is not None:
            self.stats["mesh"]["smooth"] = sst
        if decimate is not None:
            self.stats["mesh"]["decimate"] = dst
        if normals:
            self.stats["mesh"]["normals"] = nst
            return verts, tris, nrm
        return verts, tris

    def mesh_depth_maps(self, vertices, triangles, **kw) -> dict:
        """A mesh as the views of the last run() see it: Engine.mesh_render's
        hole-free depth (and, with normals=True, face-normal) maps, whose keyword
        arguments (views, cull_back, normals) pass through.  The round trip:
        v, t = pm.mesh(...), then pm.mesh_depth_maps(v, t); the maps feed
        Engine.fuse_maps and Engine.tsdf_integrate like depth_maps' own.  The
        statistics are left in self.stats["mesh_render"]."""
        if not self._ran:
            raise ValueError("mesh_depth_maps: call run() first")
        verts = np.ascontiguousarray(vertices, dtype=N.MESH_VERTEX_DTYPE).reshape(-1)
        tris = _mesh_triangles("mesh_depth_maps", triangles)
        check_mesh_render_args(len(verts), len(tris), max(len(self.views), 1), kw.get("views"),
                               kw.get("cull_back", False))
        with Engine(self.options, self.device) as eng:
            eng.set_views(self.views)
            out = eng.mesh_render(verts, tris, **kw)
        self.stats["mesh_render"] = out["stats"]
        return out

    def evaluate(self, truth, tau: float, max_dist=None, cloud="patches", mesh=None, align=None,
                 normals=None) -> dict:
        """Accuracy, completeness and F-score (cloud_compare) of a cloud of the
        last run() against the ground-truth cloud `truth` at the threshold tau.
        cloud: "patches" (the stored patches), "fused" (fused_cloud()'s points),
        or a cloud of the caller's -- an (n, 3) array or a structured array with
        a pos field, for example the vertices mesh() returned.  mesh = (vertices,
        triangles) evaluates that mesh's surface instead (mesh_compare).  align
        (cloud_compare's dict) registers the cloud, or the mesh's vertices, to
        the truth first.  normals (cloud_compare's dict) adds the error of the
        cloud's own normals against normals estimated on the truth; it needs
        "patches", "fused" or records with a normal field, and no mesh."""
        check_compare_align(align, check_cloud_compare_args(tau, max_dist))
        check_compare_normals(normals, check_cloud_compare_args(tau, max_dist))
        if mesh is not None and normals is not None:
            raise ValueError("evaluate: normals needs a cloud, not a mesh")
        if mesh is not None:
            with Engine(self.options, self.device) as eng:
                return mesh_compare(eng, mesh[0], mesh[1], truth, tau, max_dist, align)
        if isinstance(cloud, str):
            if cloud not in ("patches", "fused"):
                raise ValueError('evaluate: cloud must be "patches", "fused" or an array')
            if not self._ran:
                raise ValueError("evaluate: call run() first")
            cloud = self.patches if cloud == "patches" else self.fused_cloud()
        with Engine(self.options, self.device) as eng:
            return cloud_compare(eng, cloud, truth, tau, max_dist, align, normals)


def ncc_score(a: np.ndarray, b: np.ndarray, denom_min: float = 0.1) -> float:
    """NCCScore (error_measurements.cpp:36-60) on integer-valued textures: exact
    integer moments, finished by the library's fp64 NCC (same code as the
    kernels).  Empty input -> -1 like the reference."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.size == 0 or b.size == 0:
        return -1.0
    ai = a.astype(np.int64).ravel()
    bi = b.astype(np.int64).ravel()
    return float(lib.dp_probe_ncc(int(ai.size), int(ai.sum()), int((ai * ai).sum()), int(bi.sum()),
                                  int((bi * bi).sum()), int((ai * bi).sum()), float(denom_min)))


def read_scene_json(path: str) -> tuple[str, list[tuple[str, np.ndarray]]]:
    """IO::JSONReader (json_reader.cpp:9-29): {"imagesPath", "views": [{"filename",
    "projectionMatrix": [[4],[4],[4]]}]}."""
    with open(path) as f:
        d = json.load(f)
    images_path = d["imagesPath"]
    views = []
    for v in d["views"]:
        P = np.asarray(v["projectionMatrix"], dtype=np.float64).reshape(3, 4)
        views.append((os.path.join(images_path, v["filename"]), P))
    return images_path, views


def write_ply(path: str, patches: np.ndarray) -> None:
    """PMVS::PrintCloud (utils.cpp:9-50) through rplycpp's ASCII writer:
    x y z (float, %g) red green blue (uchar) nx ny nz (float)."""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {len(patches)}\n")
        for n in ("x", "y", "z"):
            f.write(f"property float {n}\n")
        for n in ("red", "green", "blue"):
            f.write(f"property uchar {n}\n")
        for n in ("nx", "ny", "nz"):
            f.write(f"property float {n}\n")
        f.write("end_header\n")
        for p in patches:
            x, y, z = (float(v) for v in p["pos"])
            r, g, b = (int(v) for v in p["rgb"])
            nx, ny, nz = (float(v) for v in p["normal"])
            f.write(f"{x:g} {y:g} {z:g} {r} {g} {b} {nx:g} {ny:g} {nz:g}\n")


def write_mesh_ply(path: str, vertices: np.ndarray, triangles: np.ndarray, normals=None) -> None:
    """A triangle mesh (Engine.tsdf_mesh's vertices and triangles) as an ASCII
    PLY: vertex x y z (float, %.9g: an f32 round-trips) red green blue (uchar),
    face vertex_indices (list uchar int).  With normals (Engine.mesh_normals's,
    one row per vertex) every vertex also carries nx ny nz (float, %.9g) after
    its colour."""
    triangles = np.asarray(triangles).reshape(-1, 3)
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(normals) != len(vertices):
            raise ValueError("write_mesh_ply: one normal per vertex")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {len(vertices)}\n")
        for n in ("x", "y", "z"):
            f.write(f"property float {n}\n")
        for n in ("red", "green", "blue"):
            f.write(f"property uchar {n}\n")
        if normals is not None:
            for n in ("nx", "ny", "nz"):
                f.write(f"property float {n}\n")
        f.write(f"element face {len(triangles)}\n")
        f.write("property list uchar int vertex_indices\n")
        f.write("end_header\n")
        for k, v in enumerate(vertices):
            x, y, z = (float(c) for c in v["pos"])
            r, g, b = (int(c) for c in v["rgb"])
            if normals is None:
                f.write(f"{x:.9g} {y:.9g} {z:.9g} {r} {g} {b}\n")
            else:
                nx, ny, nz = (float(c) for c in normals[k])
                f.write(f"{x:.9g} {y:.9g} {z:.9g} {r} {g} {b} {nx:.9g} {ny:.9g} {nz:.9g}\n")
        for t in triangles:
            f.write(f"3 {int(t[0])} {int(t[1])} {int(t[2])}\n")
