"""densepoints_amd -- MI355X-native PMVS patch loop (seed -> expand -> filter).

The compute path is libdensepoints.so (hand-written gfx950 HIP kernels behind
the C ABI in include/densepoints.h); this package is the host-side mirror of
the reference's methods/pmvs interface.  Importing fails loudly if the HIP
library has not been built: there is no CPU fallback.
"""
from ._native import (  # noqa: F401
    MODE_EVAL,
    MODE_EXPAND,
    MODE_FAST_EVAL,
    MODE_FAST_REFINE,
    MODE_FILTER,
    MODE_NM,
    MODE_SEED,
    PATCH_ACCEPTED,
    PATCH_DEGENERATE,
    PATCH_DTYPE,
    DensePointsError,
    FUSED_DTYPE,
    LIB_PATH,
    MESH_COMPONENT_DTYPE,
    MESH_VERTEX_DTYPE,
)
from .pmvs import (  # noqa: F401
    PMVS,
    Engine,
    FastOptions,
    Options,
    View,
    check_cloud_align_args,
    check_cloud_clean_args,
    check_cloud_knn_args,
    check_cloud_nearest_args,
    check_cloud_normals_args,
    check_cloud_transform_args,
    check_fuse_args,
    check_mapref_args,
    check_mesh_clean_args,
    check_mesh_colour_args,
    check_mesh_decimate_args,
    check_mesh_nearest_args,
    check_mesh_render_args,
    check_mesh_smooth_args,
    check_tsdf_args,
    cloud_compare,
    cloud_normal_error,
    empty_patches,
    mask_from_list,
    mesh_compare,
    mesh_deviation,
    ncc_score,
    read_pfm,
    read_scene_json,
    visible_list,
    write_pfm,
    write_mesh_ply,
    write_ply,
)
from . import synth  # noqa: F401

__version__ = "0.1.0"
