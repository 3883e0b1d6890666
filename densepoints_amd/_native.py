"""ctypes binding of libdensepoints.so (the C ABI in include/densepoints.h).

The product path is the HIP library: if it is missing, importing this module
raises -- there is no CPU fallback anywhere in densepoints_amd.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DP_LIB_VARIANT=<file name in lib/>: load a differently-compiled build of the
# same sources (A/B measurements in one GPU session, tools/ab_variants.sh)
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("DP_LIB_VARIANT") or "libdensepoints.so")

# dp_patch (include/densepoints.h) -- 80 bytes
PATCH_DTYPE = np.dtype(
    [
        ("pos", "<f4", 3),
        ("normal", "<f4", 3),
        ("ref", "<u4"),
        ("seq", "<u4"),
        ("vis", "<u8", 2),
        ("cand", "<u8", 2),
        ("score", "<f4"),
        ("evals", "<u4"),
        ("rgb", "u1", 3),
        ("flags", "u1"),
        ("parent", "<u4"),
    ],
    align=True,
)
assert PATCH_DTYPE.itemsize == 80

DP_OK = 0
DP_E_ARG = -1
DP_E_HIP = -2
DP_E_OOM = -3
DP_E_DEGENERATE = -4
DP_E_STATE = -5
DP_E_NODEVICE = -6

MODE_EVAL, MODE_FILTER, MODE_NM, MODE_SEED, MODE_EXPAND = range(5)
MODE_FAST_EVAL, MODE_FAST_REFINE = 5, 6  # performance mode (dp_fast_options)
PATCH_ACCEPTED = 1
PATCH_DEGENERATE = 2


class DpOptions(ctypes.Structure):
    _fields_ = [
        ("seed_cell_size", ctypes.c_int32),
        ("expand_cell_size", ctypes.c_int32),
        ("grid_scale", ctypes.c_int32),
        ("max_patches_per_cell", ctypes.c_int32),
        ("min_visible", ctypes.c_int32),
        ("min_expand_visible", ctypes.c_int32),
        ("nm_max_evals", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("ncc_threshold", ctypes.c_double),
        ("visible_angle", ctypes.c_double),
        ("candidate_angle", ctypes.c_double),
        ("nm_step", ctypes.c_double * 3),
        ("nm_eps", ctypes.c_double),
        ("ncc_denom_min", ctypes.c_double),
        ("max_pops", ctypes.c_int64),
    ]


class DpImage(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("stride", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("bgr", ctypes.c_void_p),
    ]


class DpDensifyStats(ctypes.Structure):
    _fields_ = [
        ("seeds_in", ctypes.c_int64),
        ("seed_patches", ctypes.c_int64),
        ("patches", ctypes.c_int64),
        ("pops", ctypes.c_int64),
        ("candidates", ctypes.c_int64),
        ("evals", ctypes.c_int64),
        ("generations", ctypes.c_int32),
        ("stalls", ctypes.c_int32),
        ("refine_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class DpGeneration(ctypes.Structure):
    _fields_ = [
        ("items", ctypes.c_int64),
        ("head", ctypes.c_int64),
        ("per_item", ctypes.c_int32),
        ("cell", ctypes.c_int32),
        ("seq0", ctypes.c_uint32),
        ("index", ctypes.c_int32),
    ]


class DpIterateStats(ctypes.Structure):
    """dp_iterate_stats: one expand-filter round of dp_densify_iterate."""
    _fields_ = [
        ("offered", ctypes.c_int64),
        ("reinserted", ctypes.c_int64),
        ("patches", ctypes.c_int64),
        ("filtered_out", ctypes.c_int64),
        ("candidates", ctypes.c_int64),
        ("evals", ctypes.c_int64),
        ("generations", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("refine_ms", ctypes.c_double),
        ("filter_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class DpFilterOptions(ctypes.Structure):
    _fields_ = [
        ("passes", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("min_neighbor_frac", ctypes.c_double),
    ]


FILTER_VISIBILITY, FILTER_NEIGHBORS = 1, 2


class DpRenderOptions(ctypes.Structure):
    _fields_ = [
        ("splat_scale", ctypes.c_float),
        ("max_radius_px", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


class DpRenderStats(ctypes.Structure):
    _fields_ = [
        ("patches", ctypes.c_int64),
        ("pairs", ctypes.c_int64),
        ("pixel_tests", ctypes.c_int64),
        ("covered_pixels", ctypes.c_int64),
        ("render_ms", ctypes.c_double),
    ]


RENDER_ALL_FACING = 1


class DpFuseOptions(ctypes.Structure):
    _fields_ = [
        ("depth_tol", ctypes.c_float),
        ("min_views", ctypes.c_int32),
        ("min_normal_cos", ctypes.c_float),
        ("flags", ctypes.c_int32),
    ]


class DpFuseStats(ctypes.Structure):
    _fields_ = [
        ("depth_pixels", ctypes.c_int64),
        ("matched_pairs", ctypes.c_int64),
        ("consistent_pairs", ctypes.c_int64),
        ("fusable", ctypes.c_int64),
        ("emitted", ctypes.c_int64),
        ("fuse_ms", ctypes.c_double),
    ]


FUSE_NO_SUPPRESS = 1

# dp_fused_point (include/densepoints.h) -- 40 bytes; pos, rgb and normal are
# named as in PATCH_DTYPE, so write_ply takes either
FUSED_DTYPE = np.dtype(
    [
        ("pos", "<f4", 3),
        ("normal", "<f4", 3),
        ("rgb", "u1", 3),
        ("n_views", "u1"),
        ("view", "<i4"),
        ("x", "<i4"),
        ("y", "<i4"),
    ],
    align=True,
)
assert FUSED_DTYPE.itemsize == 40


class DpMaprefOptions(ctypes.Structure):
    """dp_mapref_options: the knobs of dp_refine_maps (include/densepoints.h)."""
    _fields_ = [
        ("window", ctypes.c_int32),
        ("sweep", ctypes.c_int32),
        ("step_px", ctypes.c_float),
        ("reach", ctypes.c_int32 * 2),
        ("max_sources", ctypes.c_int32),
        ("top_k", ctypes.c_int32),
        ("min_ncc", ctypes.c_float),
        ("flags", ctypes.c_int32),
    ]


class DpMaprefStats(ctypes.Structure):
    _fields_ = [
        ("depth_pixels_in", ctypes.c_int64),
        ("candidates", ctypes.c_int64),
        ("source_scores", ctypes.c_int64),
        ("kept", ctypes.c_int64),
        ("filled", ctypes.c_int64),
        ("moved", ctypes.c_int64),
        ("refine_ms", ctypes.c_double),
    ]


MAPREF_KEEP_UNSCORED = 1


class DpTsdfOptions(ctypes.Structure):
    """dp_tsdf_options: the volume of dp_tsdf_integrate / dp_tsdf_mesh (include/densepoints.h)."""
    _fields_ = [
        ("origin", ctypes.c_float * 3),
        ("voxel", ctypes.c_float),
        ("dim", ctypes.c_int32 * 3),
        ("trunc", ctypes.c_float),
        ("min_weight", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


class DpTsdfStats(ctypes.Structure):
    _fields_ = [
        ("voxels", ctypes.c_int64),
        ("observations", ctypes.c_int64),
        ("observed_voxels", ctypes.c_int64),
        ("near_voxels", ctypes.c_int64),
        ("integrate_ms", ctypes.c_double),
    ]


class DpMeshStats(ctypes.Structure):
    _fields_ = [
        ("active_cells", ctypes.c_int64),
        ("vertices", ctypes.c_int64),
        ("triangles", ctypes.c_int64),
        ("mesh_ms", ctypes.c_double),
    ]


# dp_mesh_vertex (include/densepoints.h) -- 16 bytes
MESH_VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("rgb", "u1", 3), ("pad", "u1")])
assert MESH_VERTEX_DTYPE.itemsize == 16


class DpMeshCleanOptions(ctypes.Structure):
    """dp_mesh_clean_options: the selection of dp_mesh_clean (include/densepoints.h)."""
    _fields_ = [
        ("min_triangles", ctypes.c_int64),
        ("min_fraction", ctypes.c_float),
        ("max_components", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class DpMeshCleanStats(ctypes.Structure):
    _fields_ = [
        ("vertices_in", ctypes.c_int64),
        ("triangles_in", ctypes.c_int64),
        ("invalid_triangles", ctypes.c_int64),
        ("unused_vertices", ctypes.c_int64),
        ("components", ctypes.c_int64),
        ("largest_triangles", ctypes.c_int64),
        ("components_kept", ctypes.c_int64),
        ("vertices_out", ctypes.c_int64),
        ("triangles_out", ctypes.c_int64),
        ("clean_ms", ctypes.c_double),
    ]


# dp_mesh_component (include/densepoints.h) -- 16 bytes
MESH_COMPONENT_DTYPE = np.dtype([("root", "<i4"), ("vertices", "<i4"), ("triangles", "<i4"), ("rank", "<i4")])
assert MESH_COMPONENT_DTYPE.itemsize == 16 and ctypes.sizeof(DpMeshCleanOptions) == 24


DP_VERTEX_BOUNDARY = 1
DP_VERTEX_NONMANIFOLD = 2
DP_SMOOTH_FREE_BOUNDARY = 1


class DpMeshSmoothOptions(ctypes.Structure):
    """dp_mesh_smooth_options: the steps of dp_mesh_smooth (include/densepoints.h).
    `lambda` is a Python keyword: read it with getattr."""
    _fields_ = [
        ("iterations", ctypes.c_int32),
        ("lambda", ctypes.c_float),
        ("mu", ctypes.c_float),
        ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


_ADJACENCY_COUNTS = ["vertices_in", "triangles_in", "invalid_triangles", "degenerate_triangles", "isolated_vertices",
                     "edges", "boundary_edges", "nonmanifold_edges", "boundary_vertices", "max_valence"]


class DpMeshAdjacencyStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in _ADJACENCY_COUNTS] + [("adjacency_ms", ctypes.c_double)]


class DpMeshSmoothStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int64) for n in _ADJACENCY_COUNTS + ["movable_vertices", "pinned_vertices", "steps"]]
                + [("adjacency_ms", ctypes.c_double), ("smooth_ms", ctypes.c_double)])


class DpMeshNormalsStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("vertices_in", "triangles_in", "invalid_triangles",
                                              "degenerate_triangles", "zero_normals")] + [("normals_ms", ctypes.c_double)]


assert ctypes.sizeof(DpMeshSmoothOptions) == 20 and ctypes.sizeof(DpMeshAdjacencyStats) == 88
assert ctypes.sizeof(DpMeshSmoothStats) == 120 and ctypes.sizeof(DpMeshNormalsStats) == 48


DP_DECIMATE_MEAN, DP_DECIMATE_QUADRIC = 0, 1


class DpMeshDecimateOptions(ctypes.Structure):
    """dp_mesh_decimate_options: the cluster lattice and the placement of dp_mesh_decimate (include/densepoints.h)."""
    _fields_ = [
        ("origin", ctypes.c_float * 3),
        ("cell", ctypes.c_float),
        ("mode", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class DpMeshDecimateStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "vertices_in", "triangles_in", "invalid_triangles", "degenerate_triangles", "unused_vertices", "clamped_vertices",
        "clusters", "orphan_clusters", "max_cluster", "collapsed_triangles", "duplicate_triangles", "quadric_vertices",
        "mean_vertices", "vertices_out", "triangles_out")] + [("decimate_ms", ctypes.c_double)]


assert ctypes.sizeof(DpMeshDecimateOptions) == 28 and ctypes.sizeof(DpMeshDecimateStats) == 128


DP_MESH_RENDER_CULL_BACK = 1


class DpMeshRenderOptions(ctypes.Structure):
    """dp_mesh_render_options: the flags of dp_mesh_render (include/densepoints.h)."""
    _fields_ = [("flags", ctypes.c_int32)]


class DpMeshRenderStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "triangles", "invalid_triangles", "pairs", "clipped_pairs", "culled_pairs", "pixel_tests",
        "covered_pixels")] + [("render_ms", ctypes.c_double)]


assert ctypes.sizeof(DpMeshRenderOptions) == 4 and ctypes.sizeof(DpMeshRenderStats) == 64


DP_MESH_COLOUR_BILINEAR = 1
DP_MESH_COLOUR_CLEAR_UNSEEN = 2


class DpMeshColourOptions(ctypes.Structure):
    """dp_mesh_colour_options: the options of dp_mesh_colour (include/densepoints.h)."""
    _fields_ = [("depth_tol", ctypes.c_float), ("min_cos", ctypes.c_float), ("flags", ctypes.c_int32)]


class DpMeshColourStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "vertices", "projected_pairs", "occluded_pairs", "grazing_pairs", "visible_pairs", "coloured_vertices",
        "unseen_vertices")] + [("colour_ms", ctypes.c_double)]


assert ctypes.sizeof(DpMeshColourOptions) == 12 and ctypes.sizeof(DpMeshColourStats) == 64


class DpCloudNearestOptions(ctypes.Structure):
    """dp_cloud_nearest_options: the options of dp_cloud_nearest (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("hist_bins", ctypes.c_int32), ("flags", ctypes.c_int32)]


class DpCloudNearestStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "queries", "targets", "skipped_queries", "skipped_targets", "matched", "unmatched", "grid_cells",
        "max_cell_targets")] + [("build_ms", ctypes.c_double), ("query_ms", ctypes.c_double)]


assert ctypes.sizeof(DpCloudNearestOptions) == 12 and ctypes.sizeof(DpCloudNearestStats) == 80


class DpMeshNearestOptions(ctypes.Structure):
    """dp_mesh_nearest_options: the options of dp_mesh_nearest (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("hist_bins", ctypes.c_int32), ("flags", ctypes.c_int32)]


class DpMeshNearestStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "queries", "skipped_queries", "matched", "unmatched", "triangles", "invalid_triangles", "degenerate_triangles",
        "nonfinite_triangles", "grid_cells", "grid_entries", "max_cell_entries")] + [
        ("build_ms", ctypes.c_double), ("query_ms", ctypes.c_double)]


assert ctypes.sizeof(DpMeshNearestOptions) == 12 and ctypes.sizeof(DpMeshNearestStats) == 104


class DpCloudKnnOptions(ctypes.Structure):
    """dp_cloud_knn_options: the options of dp_cloud_knn (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("k", ctypes.c_int32), ("flags", ctypes.c_int32)]


class DpCloudKnnStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "queries", "targets", "skipped_queries", "skipped_targets", "full", "partial", "empty", "neighbours",
        "grid_cells", "max_cell_targets")] + [("build_ms", ctypes.c_double), ("query_ms", ctypes.c_double)]


class DpCloudCleanOptions(ctypes.Structure):
    """dp_cloud_clean_options: the options of dp_cloud_clean (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("k", ctypes.c_int32), ("min_neighbours", ctypes.c_int32),
                ("std_mul", ctypes.c_float), ("flags", ctypes.c_int32)]


class DpCloudCleanStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "points", "skipped", "eligible", "kept", "removed_sparse", "removed_far", "grid_cells",
        "max_cell_targets")] + [(n, ctypes.c_double) for n in ("mu", "sigma", "threshold", "knn_ms", "clean_ms")]


assert ctypes.sizeof(DpCloudKnnOptions) == 12 and ctypes.sizeof(DpCloudKnnStats) == 96
assert ctypes.sizeof(DpCloudCleanOptions) == 20 and ctypes.sizeof(DpCloudCleanStats) == 104
CLOUD_KNN_EXCLUDE_SELF = 1
CLOUD_CLEAN_RADIUS_ONLY = 1


class DpCloudNormalsOptions(ctypes.Structure):
    """dp_cloud_normals_options: the options of dp_cloud_normals (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("k", ctypes.c_int32), ("min_neighbours", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class DpCloudNormalsStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "points", "skipped", "estimated", "sparse", "degenerate", "flipped", "unoriented", "grid_cells",
        "max_cell_targets")] + [("knn_ms", ctypes.c_double), ("normals_ms", ctypes.c_double)]


assert ctypes.sizeof(DpCloudNormalsOptions) == 16 and ctypes.sizeof(DpCloudNormalsStats) == 88
CLOUD_NORMALS_ORIENT_VIEWPOINT, CLOUD_NORMALS_ORIENT_DIRECTION = 1, 2


class DpCloudAlignOptions(ctypes.Structure):
    """dp_cloud_align_options: the options of dp_cloud_align (include/densepoints.h)."""
    _fields_ = [("max_dist", ctypes.c_float), ("iterations", ctypes.c_int32), ("min_pairs", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("rms_tol", ctypes.c_double)]


class DpCloudAlignStep(ctypes.Structure):
    _fields_ = [("matched", ctypes.c_int64), ("rms", ctypes.c_double)]


class DpCloudAlignStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "queries", "targets", "skipped_queries", "skipped_targets", "matched", "unmatched", "grid_cells",
        "max_cell_targets", "iterations_run", "stop_reason")] + [("grid_ms", ctypes.c_double),
                                                                 ("iterate_ms", ctypes.c_double)]


assert ctypes.sizeof(DpCloudAlignOptions) == 24 and ctypes.sizeof(DpCloudAlignStep) == 16
assert ctypes.sizeof(DpCloudAlignStats) == 96
CLOUD_ALIGN_SCALE = 1
CLOUD_ALIGN_STOP_ITERATIONS, CLOUD_ALIGN_STOP_RMS, CLOUD_ALIGN_STOP_PAIRS = 0, 1, 2
CLOUD_ALIGN_STOP_DEGENERATE, CLOUD_ALIGN_STOP_EMPTY = 3, 4
# a dp_cloud_align_step as numpy reads it
CLOUD_ALIGN_STEP_DTYPE = np.dtype([("matched", "<i8"), ("rms", "<f8")])


class DpSynthConfig(ctypes.Structure):
    _fields_ = [
        ("n_views", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("kind", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("spread_deg", ctypes.c_double),
        ("seed_stride_px", ctypes.c_double),
        ("depth_noise", ctypes.c_double),
    ]


class DpMatcherOptions(ctypes.Structure):
    """dp_matcher_options: Features::MatcherOptions (matcher.h:14-33) + cv::ORB knobs."""

    _fields_ = [
        ("n_features", ctypes.c_int32),
        ("n_levels", ctypes.c_int32),
        ("scale_factor", ctypes.c_double),
        ("edge_threshold", ctypes.c_int32),
        ("fast_threshold", ctypes.c_int32),
        ("cell_size", ctypes.c_int32),
        ("max_keypoints_per_cell", ctypes.c_int32),
        ("epipolar_matching", ctypes.c_int32),
        ("max_epipolar_distance", ctypes.c_float),
        ("nn_match_ratio", ctypes.c_float),
        ("matcher_type", ctypes.c_int32),
        ("detector_type", ctypes.c_int32),
        ("akaze_threshold", ctypes.c_float),
    ]


class DpSeedStats(ctypes.Structure):
    _fields_ = [
        ("keypoints_detected", ctypes.c_int64),
        ("keypoints", ctypes.c_int64),
        ("pairs", ctypes.c_int64),
        ("ratio_matches", ctypes.c_int64),
        ("matches", ctypes.c_int64),
        ("points", ctypes.c_int64),
        ("detect_ms", ctypes.c_double),
        ("describe_ms", ctypes.c_double),
        ("match_ms", ctypes.c_double),
        ("triangulate_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class DpFastOptions(ctypes.Structure):
    """dp_fast_options: the performance mode's knobs (include/densepoints.h)."""
    _fields_ = [
        ("iters", ctypes.c_int32),
        ("margin", ctypes.c_int32),
        ("tile_budget", ctypes.c_int32),
        ("max_views", ctypes.c_int32),
        ("fd_step", ctypes.c_float),
        ("ls_step", ctypes.c_float),
        ("densify", ctypes.c_int32),
        ("gradient", ctypes.c_int32),
        ("filter_max_views", ctypes.c_int32),
    ]


class DpFastStats(ctypes.Structure):
    _fields_ = [("patches", ctypes.c_int64), ("evals", ctypes.c_int64), ("view_evals", ctypes.c_int64),
                ("staged_bytes", ctypes.c_int64), ("clipped_stagings", ctypes.c_int64)]


# dp_keypoint: the cv::KeyPoint fields the matcher reads
KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("reserved", "<i4")]
)

_P = ctypes.c_void_p
_I = ctypes.c_int
_D = ctypes.c_double

# (name, restype, argtypes) of every exported symbol in include/densepoints.h
# and include/densepoints_probe.h
SIGNATURES = [
    ("dp_default_options", None, [_P]),
    ("dp_abi_version", _I, []),
    ("dp_device_count", _I, []),
    ("dp_ctx_create", _I, [_P, _I, _P]),
    ("dp_ctx_destroy", _I, [_P]),
    ("dp_last_error", ctypes.c_char_p, [_P]),
    ("dp_set_options", _I, [_P, _P]),
    ("dp_set_views", _I, [_P, _I, _P, _P]),
    ("dp_set_views_device", _I, [_P, _I, _P, _P, _P, _P, _P]),
    ("dp_build_pyramid", _I, [_P, _I]),
    ("dp_set_level", _I, [_P, _I]),
    ("dp_level_info", _I, [_P, _I, _I, _P, _P, _P]),
    ("dp_read_level", _I, [_P, _I, _I, _P]),
    ("dp_view_geometry", _I, [_P, _P, _P, _P, _P]),
    ("dp_seeds_to_patches", _I, [_P, _P, _I, _P]),
    ("dp_eval_batch", _I, [_P, _P, _I, _I, _P]),
    ("dp_refine_batch", _I, [_P, _P, _I, _I, _I, _P]),
    ("dp_refine_batch_device", _I, [_P, _P, _I, _I, _I, _P, _P]),
    ("dp_expand_batch", _I, [_P, _P, _I, _P, _P]),
    ("dp_expand_batch_device", _I, [_P, _P, _I, _P, _P, _P]),
    ("dp_densify", _I, [_P, _P, _I, _P, _P, _P]),
    ("dp_densify_begin", _I, [_P, _P, _I, _P]),
    ("dp_densify_commit", _I, [_P, _P, _P, _P, ctypes.c_int64]),
    ("dp_densify_result", _I, [_P, _P, _P, _P]),
    ("dp_densify_run", _I, [_P, _P, ctypes.c_int32]),
    ("dp_densify_run_until", _I, [_P, _P, ctypes.c_int32, ctypes.c_int64, _P]),
    ("dp_densify_owners", _I, [_P, _P, _I, _I, _P, _P]),
    ("dp_densify_partition_stats", _I, [_P, _P]),
    ("dp_densify_refine_items", _I, [_P, _P, _P, ctypes.c_int64, _P, _P]),
    ("dp_densify_partition_async", _I, [_P, _P, _I, _I, _P, _P, _P]),
    ("dp_densify_refine_share_async", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    ("dp_densify_commit_gathered_device", _I, [_P, _P, _P, ctypes.c_int64, _I, _P, _P]),
    ("dp_densify_resume", _I, [_P, _P, ctypes.c_int64, _P, _P]),
    ("dp_densify_resume_device", _I, [_P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_densify_store_device", _I, [_P, _P, _P]),
    ("dp_densify_iterate", _I, [_P, _P, _I, _I, _P, _P, _P, _P, _P]),
    ("dp_default_filter_options", None, [_P]),
    ("dp_filter_patches", _I, [_P, _P, ctypes.c_int64, _P, _P]),
    ("dp_filter_patches_device", _I, [_P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_default_render_options", None, [_P]),
    ("dp_render_maps", _I, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    ("dp_render_maps_device", _I, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_default_fuse_options", None, [_P]),
    ("dp_fuse_maps", _I, [_P, _P, _I, _P, _P, _P, _P, _P, _P]),
    ("dp_fuse_maps_device", _I, [_P, _P, _I, _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_default_mapref_options", None, [_P]),
    ("dp_refine_maps", _I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_refine_maps_device", _I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_default_tsdf_options", None, [_P]),
    ("dp_tsdf_integrate", _I, [_P, _P, _I, _P, _P, _P, _P, _P, _P]),
    ("dp_tsdf_integrate_device", _I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_tsdf_mesh", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_tsdf_mesh_device", _I, [_P, _P, _P, _P, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_default_mesh_clean_options", None, [_P]),
    ("dp_mesh_components", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("dp_mesh_components_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_mesh_clean", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_mesh_clean_device", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P,
                                  ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("dp_default_mesh_smooth_options", None, [_P]),
    ("dp_mesh_adjacency", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    ("dp_mesh_adjacency_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                      _P]),
    ("dp_mesh_smooth", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
    ("dp_mesh_smooth_device", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_mesh_normals", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
    ("dp_mesh_normals_device", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_default_mesh_decimate_options", None, [_P]),
    ("dp_mesh_decimate", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_mesh_decimate_device", _I, [_P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P,
                                     ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("dp_default_mesh_render_options", None, [_P]),
    ("dp_mesh_render", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _I, _P, _P, _P, _P, _P]),
    ("dp_mesh_render_device", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _I, _P, _P, _P, _P, _P, _P]),
    ("dp_default_mesh_colour_options", None, [_P]),
    ("dp_mesh_colour", _I, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    ("dp_mesh_colour_device", _I, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_cloud_nearest", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P,
                              _P]),
    ("dp_cloud_nearest_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P,
                                     _P, _P, _P, _P]),
    ("dp_mesh_nearest", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P,
                             _P, _P]),
    ("dp_mesh_nearest_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64, _P,
                                    _P, _P, _P, _P, _P, _P]),
    ("dp_cloud_knn", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("dp_cloud_knn_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P,
                                 _P, _P, _P]),
    ("dp_cloud_clean", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_cloud_clean_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("dp_cloud_normals", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P, _P]),
    ("dp_cloud_normals_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("dp_cloud_transform", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    ("dp_cloud_transform_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
    ("dp_cloud_align", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P,
                            _P, _P, _P]),
    ("dp_cloud_align_device", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P,
                                   _P, _P, _P, _P, _P, _P]),
    ("dp_last_kernel_ms", _I, [_P, _P]),
    ("dp_default_matcher_options", None, [_P]),
    ("dp_orb_pattern", _I, [_P]),
    ("dp_generate_seeds", _I, [_P, _P, _P, _P, _P]),
    ("dp_seed_keypoints", _I, [_P, _I, _P, _P, _P]),
    ("dp_seed_matches", _I, [_P, _I, _P, _P, _P, _P]),
    ("dp_knn_match", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
    ("dp_knn_match_wide", _I, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _I, _P, _P]),
    ("dp_seed_descriptor_bytes", _I, [_P]),
    ("dp_fundamental_matrix", _I, [_P, _P, _P]),
    ("dp_triangulate", _I, [_P, ctypes.c_int64, _P, _P, _P, _P]),
    ("dp_synth_default", None, [_P]),
    ("dp_synth_cameras", _I, [_P, _P]),
    ("dp_synth_render_host", _I, [_P, _P, _I, _P]),
    ("dp_synth_render_device", _I, [_P, _P, _P, _I, _P, _P]),
    ("dp_synth_seeds", ctypes.c_int64, [_P, _P, _P, ctypes.c_int64]),
    ("dp_synth_surface", _I, [_P, ctypes.c_int64, _P, _P, _P]),
    ("dp_default_fast_options", None, [_P]),
    ("dp_set_fast_options", _I, [_P, _P]),
    ("dp_build_gray", _I, [_P]),
    ("dp_read_gray", _I, [_P, _I, _P]),
    ("dp_fast_expand_batch", _I, [_P, _P, _I, _P, _P]),
    ("dp_fast_expand_batch_device", _I, [_P, _P, _I, _P, _P, _P]),
    ("dp_fast_last_stats", _I, [_P, _P]),
    ("dp_probe_sincos", None, [_D, _P, _P]),
    ("dp_probe_acos", _D, [_D]),
    ("dp_probe_texture", _I, [_P, ctypes.c_int32, ctypes.c_int32, _P, _P, _I, _P]),
    ("dp_probe_ncc", _D, [ctypes.c_int32] * 6 + [_D]),
    ("dp_probe_math_device", _I, [_P, _I, _P]),
    ("dp_probe_texel_device", _I, [_P, _P, _P, _I, _P]),
    ("dp_probe_recip_f32_device", _I, [_P, _I, _P]),
    ("dp_probe_grad_q24_device", _I, [_P, _I, _P]),
    ("dp_probe_lds_unaligned_device", _I, [_P]),
    ("dp_debug_stamps", _I, [_P]),
    ("dp_probe_keep_gather", _I, [_P, _P, ctypes.c_int64, _P, _P, _P]),
    ("dp_probe_akaze_plane", _I, [_P, _I, _I, _I, _P, ctypes.c_int64, _P]),
    ("dp_probe_orb_level", _I, [_P, _I, _I, _I, _D, _P, ctypes.c_int64, _P]),
    ("dp_probe_seed_stages", _I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    ("dp_probe_seed_t2q", _I, [_P, _I, _P, _P]),
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"densepoints_amd: HIP library {LIB_PATH} is missing; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class DensePointsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"densepoints error {code}: {msg}")
        self.code = code


def check(rc: int, ctx=None) -> None:
    if rc != DP_OK:
        msg = lib.dp_last_error(ctx).decode() if ctx else ""
        raise DensePointsError(rc, msg)


def ptr(a) -> int | None:
    if a is None:
        return None
    return a.ctypes.data


def default_options() -> DpOptions:
    o = DpOptions()
    lib.dp_default_options(ctypes.byref(o))
    return o
