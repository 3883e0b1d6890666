// cli_args.h -- the densify CLI's options and their parsing; no GPU dependency
// (include/densepoints.h for the option structs and their defaults only).
#pragma once

#include "../../include/densepoints.h"

#include <string>

struct Args {
    std::string input, settings, output = "points.ply", seeds_path;
    std::string synth, scene_dir; // --synthetic V,W,H,KIND --write-scene DIR
    int device = 0, gpus = 1;
    bool force_multi = false; // --multi: the multi-GPU protocol at any --gpus
    std::string exchange_mode = "auto";
    long long replicate_below = -1; // parse_args resolves < 0 to 1024 x gpus
    long long max_pops = -1;        // < 0: the settings' value
    int level = 0;
    bool check_only = false, do_filter = false;
    int iterations = 1;
    dp_matcher_options matcher; // MatcherOptions defaults (matcher.h:21-32), ORB::create(40000)
    dp_fast_options fast;       // --mode fast: fast.densify = 1
    std::string depth_dir, fuse_path;
    double splat_scale = 1.0;
    bool depth_normals = false;
    dp_fuse_options fuse;
    // --fuse-clean-k K --fuse-clean-radius R [--fuse-clean-std A]
    // [--fuse-clean-min-neighbours M] [--fuse-clean-radius-only]: dp_cloud_clean of
    // the fused cloud on the device before it is written and evaluated.  Only
    // with --fuse; K and R go together.
    int fuse_clean_k = 0;              // 0: not given, no clean-up
    double fuse_clean_radius = 0.0;    // 0: not given
    double fuse_clean_std = -1.0;      // < 0: not given; parse_args resolves it to 2 with K
    int fuse_clean_min_neighbours = 0; // 0: not given; parse_args resolves it to 1 with K
    bool fuse_clean_radius_only = false;
    bool fuse_clean() const { return fuse_clean_k > 0; }
    // --refine-maps N: dp_refine_maps passes between the render and its users
    int refine_passes = 0;
    int refine_window = 0;        // 0: the library's default
    double refine_min_ncc = -2.0; // < -1: the library's default
    // --mesh FILE.ply: dp_tsdf_integrate + dp_tsdf_mesh on the (refined) maps
    std::string mesh_path;
    int mesh_dim = 256;           // voxels along the patches' longest side
    double mesh_voxel = 0.0;      // 0: that side / mesh_dim
    double mesh_trunc = 0.0;      // 0: 4 voxels
    int mesh_min_weight = 2;
    // --mesh-min-component N, --mesh-min-component-frac F, --mesh-keep-largest K:
    // dp_mesh_clean on the mesh before it is written; none given: no clean-up
    long long mesh_min_component = -1; // < 0: not given (the library's default)
    double mesh_min_component_frac = -1.0;
    long long mesh_keep_largest = -1;
    bool mesh_clean() const
    {
        return mesh_min_component >= 0 || mesh_min_component_frac >= 0.0 || mesh_keep_largest >= 0;
    }
    // --mesh-smooth N [--mesh-smooth-lambda L] [--mesh-smooth-mu M]
    // [--mesh-smooth-free-boundary]: dp_mesh_smooth on the (cleaned) mesh;
    // --mesh-normals: dp_mesh_normals of the mesh as written.  Only with --mesh.
    int mesh_smooth = -1;              // < 0: not given, no smoothing
    double mesh_smooth_lambda = 0.0;   // 0: the library's default
    double mesh_smooth_mu = 1.0;       // > 0: the library's default
    bool mesh_smooth_free_boundary = false;
    bool mesh_normals = false;
    // --mesh-decimate F [--mesh-decimate-quadric]: dp_mesh_decimate on the
    // (cleaned, smoothed) mesh, cluster cell = F x the volume's voxel, the
    // lattice anchored at the volume's origin.  Only with --mesh.
    double mesh_decimate = 0.0; // 0: not given, no simplification
    bool mesh_decimate_quadric = false;
    // --mesh-depth-maps DIR [--mesh-depth-normals] [--mesh-cull-back]:
    // dp_mesh_render of the final mesh into every view.  Only with --mesh.
    std::string mesh_depth_dir;
    bool mesh_depth_normals = false, mesh_cull_back = false;
    // --mesh-colour [--mesh-colour-bilinear] [--mesh-colour-tol T]
    // [--mesh-colour-min-cos C]: dp_mesh_colour of the final mesh from every
    // view.  Only with --mesh.
    bool mesh_colour = false, mesh_colour_bilinear = false;
    double mesh_colour_tol = -1.0, mesh_colour_min_cos = -1.0; // < 0: the library's default
    // --evaluate truth.xyz --eval-tau T [--eval-max-dist D]: accuracy,
    // completeness and F-score of the written clouds against the ground-truth
    // points of the file (dp_cloud_nearest, both directions) in the report
    std::string eval_path;
    double eval_tau = 0.0;      // 0: not given
    double eval_max_dist = 0.0; // 0: not given; parse_args resolves it to 10 x eval_tau
    // --eval-mesh-surface: with --evaluate and --mesh, the mesh's surface against
    // the truth (dp_mesh_nearest) and, with --mesh-decimate, the deviation of the
    // decimated surface from the one before, in the report
    bool eval_mesh_surface = false;
    // --eval-align [--eval-align-iterations N] [--eval-align-radius R]
    // [--eval-align-scale]: with --evaluate, the patches are registered to the
    // truth first (dp_cloud_align) and every evaluated cloud is moved by that
    // transform, on copies; the report gains "align"
    bool eval_align = false, eval_align_scale = false;
    int eval_align_iterations = 0;  // 0: not given; parse_args resolves it to 30
    double eval_align_radius = 0.0; // 0: not given; parse_args resolves it to eval_max_dist
    // --eval-normals [--eval-normals-k K] [--eval-normals-radius R]: with
    // --evaluate, the truth's normals are estimated once (dp_cloud_normals) and
    // the patches' and the fused points' own normals compared with those of
    // their matches; their entries gain "normals"
    bool eval_normals = false;
    int eval_normals_k = 0;           // 0: not given; parse_args resolves it to 16
    double eval_normals_radius = 0.0; // 0: not given; parse_args resolves it to eval_max_dist

    Args();
};

enum class Parse { Run, Help, UsageError };

// Reads argv into `a`.  On UsageError `error` holds the message to print after
// "densify: ", or is empty where the usage text is the message.
Parse parse_args(int argc, char **argv, Args &a, std::string &error);

// the usage text, to stderr
void usage();
