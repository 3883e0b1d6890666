#include "cli_args.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

void usage()
{
    std::fprintf(stderr,
                 "usage: densify -i scene.json [--seeds seeds.xyz] [-s settings.json] [-o points.ply]\n"
                 "               [--device N] [--max-pops N] [--level L] [--filter] [--check-only]\n"
                 "               [--iterations N]  (1..16 rounds of expansion then filter, each round\n"
                 "                             re-expanding from the previous round's survivors with the\n"
                 "                             store resident on the device; N > 1 implies --filter)\n"
                 "               [--features N] [--fast-threshold T] [--epipolar-matching]\n"
                 "               [--matcher knn|flann]  (MatcherType, matcher.h:12)\n"
                 "               [--detector orb|akaze] [--akaze-threshold T]  (DetectorType, matcher.h:11)\n"
                 "               [--gpus N]   (one context per GPU, generations partitioned by\n"
                 "                             reference-view super-tile, accepted candidates\n"
                 "                             all-gathered device to device; output identical to 1 GPU)\n"
                 "               [--exchange auto|rccl|copy]  (auto: RCCL when every context has its\n"
                 "                             own GPU, else peer copies; --multi: that protocol at 1 GPU)\n"
                 "               [--replicate-below N]  (generations of fewer items run on every\n"
                 "                             context, device-resident, no exchange; default 1024 x gpus)\n"
                 "               [--mode parity|fast] [--fast-iters N] [--fast-gradient 0|1]\n"
                 "                            (fast: the performance-mode refine -- LDS-staged gray\n"
                 "                             tiles, fused CG -- for the seed stage and every expansion;\n"
                 "                             gradient 1: analytic, 0: forward differences)\n"
                 "               [--depth-maps DIR [--splat-scale S] [--depth-normals]]  (after the PLY:\n"
                 "                             DIR/depth_%%04d.pfm, and normal_%%04d.pfm, of every view --\n"
                 "                             the written patches as discs of radius S x rho, nearest\n"
                 "                             per pixel: dp_render_maps)\n"
                 "               [--fuse FILE.ply [--fuse-min-views K] [--fuse-depth-tol T]]  (after those:\n"
                 "                             the depth and normal maps of every view, rendered and fused\n"
                 "                             on the device into one cross-view-consistent cloud --\n"
                 "                             dp_fuse_maps; K = 0..63 agreeing other views, default 2;\n"
                 "                             T = relative depth tolerance, default 0.01)\n"
                 "               [--refine-maps N [--refine-window W] [--refine-min-ncc T]]  (N passes of the\n"
                 "                             per-pixel photometric refinement, dp_refine_maps, on the\n"
                 "                             rendered maps before --depth-maps writes them -- then also\n"
                 "                             score_%%04d.pfm -- and before --fuse fuses them; W = odd\n"
                 "                             window side 3..11, default 7; T = least score, default 0.5)\n"
                 "               [--mesh FILE.ply [--mesh-dim N] [--mesh-voxel S] [--mesh-trunc T]\n"
                 "                [--mesh-min-weight M] [--mesh-min-component N]\n"
                 "                [--mesh-min-component-frac F] [--mesh-keep-largest K]]\n"
                 "                            (after those: the depth maps of every view,\n"
                 "                             rendered -- and refined, with --refine-maps -- on the device,\n"
                 "                             integrated into one TSDF volume around the written patches\n"
                 "                             and meshed by marching tetrahedra -- dp_tsdf_integrate,\n"
                 "                             dp_tsdf_mesh; N = voxels along the patches' longest side,\n"
                 "                             2..1024, default 256; S = voxel side, default that side / N;\n"
                 "                             T = truncation, default 4 S; M = least views per voxel,\n"
                 "                             1..64, default 2; with N, F or K the mesh's connected\n"
                 "                             components are labelled on the device and the small ones\n"
                 "                             dropped before the PLY is written -- dp_mesh_clean: those of\n"
                 "                             fewer than N triangles, of less than the share F, 0..1, of the\n"
                 "                             largest component's triangles, or not among the K largest)\n"
                 "               [--mesh-smooth N [--mesh-smooth-lambda L] [--mesh-smooth-mu M]\n"
                 "                [--mesh-smooth-free-boundary]] [--mesh-normals]\n"
                 "                            (only with --mesh, after the clean-up, on the device: N =\n"
                 "                             0..1000 Taubin iterations of the vertex positions --\n"
                 "                             dp_mesh_smooth; L = the shrinking factor in (0, 1], default\n"
                 "                             0.5; M = the inflating factor <= 0, default -0.53, 0 = plain\n"
                 "                             Laplacian; boundary vertices stay unless freed;\n"
                 "                             --mesh-normals: nx ny nz per vertex -- dp_mesh_normals)\n"
                 "               [--mesh-decimate F [--mesh-decimate-quadric]]\n"
                 "                            (only with --mesh, between the smoothing and the normals, on\n"
                 "                             the device: the vertices of every cell of side F voxels, F > 0,\n"
                 "                             merged into one at their mean -- or, with -quadric, where the\n"
                 "                             planes of the cell's triangles meet -- and the triangles that\n"
                 "                             collapse or repeat dropped -- dp_mesh_decimate)\n"
                 "               [--mesh-depth-maps DIR [--mesh-depth-normals] [--mesh-cull-back]]\n"
                 "                            (only with --mesh, after the final mesh, on the device: the\n"
                 "                             mesh rendered into every view -- dp_mesh_render -- as\n"
                 "                             DIR/mesh_depth_NNNN.pfm and, with -normals, the face normals\n"
                 "                             as mesh_normal_NNNN.pfm; -cull-back skips the triangles that\n"
                 "                             face away from a view)\n"
                 "               [--mesh-colour [--mesh-colour-bilinear] [--mesh-colour-tol T]\n"
                 "                [--mesh-colour-min-cos C]]\n"
                 "                            (only with --mesh, after the final mesh, on the device: every\n"
                 "                             vertex coloured by the views that see it -- dp_mesh_colour --\n"
                 "                             against the mesh's own depth maps, weighted by the cosine\n"
                 "                             between its normal and the ray; T: relative depth tolerance,\n"
                 "                             0.01; C: least cosine, 0.2; -bilinear: four taps per view)\n"
                 "               [--fuse-clean-k K --fuse-clean-radius R [--fuse-clean-std A]\n"
                 "                [--fuse-clean-min-neighbours M] [--fuse-clean-radius-only]]\n"
                 "                            (with --fuse: outlier removal of the fused cloud on the device\n"
                 "                             before it is written and evaluated -- dp_cloud_clean; a point\n"
                 "                             stays when it has M (1) of its K (1..32) nearest neighbours\n"
                 "                             within R and its mean distance to them is at most the cloud's\n"
                 "                             mean + A (2) standard deviations; -radius-only: the first alone)\n"
                 "               [--evaluate truth.xyz --eval-tau T [--eval-max-dist D]]\n"
                 "                            (after the outputs are written: the patches -- and the fused\n"
                 "                             cloud and the mesh's vertices, with --fuse and --mesh --\n"
                 "                             against the ground-truth points of the file, one x y z per\n"
                 "                             line as --seeds reads them, on the device -- dp_cloud_nearest;\n"
                 "                             the report gains accuracy, completeness and F-score at the\n"
                 "                             threshold T > 0; D = search radius >= T, default 10 T)\n"
                 "               [--eval-mesh-surface]\n"
                 "                            (with --evaluate and --mesh: the report gains mesh_surface, the\n"
                 "                             mesh's vertices against the truth and the truth against the\n"
                 "                             mesh's surface -- dp_mesh_nearest -- and, with --mesh-decimate,\n"
                 "                             decimate_deviation: how far the decimated surface lies from\n"
                 "                             the one it was made of, within the radius D)\n"
                 "               [--eval-align [--eval-align-iterations N] [--eval-align-radius R]\n"
                 "                [--eval-align-scale]]\n"
                 "                            (with --evaluate: the patches are first registered to the truth\n"
                 "                             by point-to-point ICP on the device -- dp_cloud_align, N (30)\n"
                 "                             iterations in 1..1000, pairs trimmed at R, default D; -scale\n"
                 "                             estimates a similarity -- and every evaluated cloud is moved\n"
                 "                             by that transform, on copies: the files are not changed; the\n"
                 "                             report gains align: the matrix, the scale, the iterations run,\n"
                 "                             the pairs and the rms before and after)\n"
                 "               [--eval-normals [--eval-normals-k K] [--eval-normals-radius R]]\n"
                 "                            (with --evaluate: the normals of the truth are estimated on the\n"
                 "                             device -- dp_cloud_normals, K (16) neighbours in 3..32 within R,\n"
                 "                             default D -- and the patches and fused entries of the report\n"
                 "                             gain normals: n, mean_deg, median_deg and p90_deg of the unsigned\n"
                 "                             angle between a point's own normal and that of its match within\n"
                 "                             T; with --eval-align the normals are those of the moved copies)\n"
                 "       densify --synthetic V,W,H,KIND --write-scene DIR\n");
}

Args::Args()
{
    dp_default_matcher_options(&matcher);
    dp_default_fast_options(&fast);
    fast.densify = 0;
    dp_default_fuse_options(&fuse);
}

namespace {

// The strict value parsers: the whole of `v` must be the value.  (Options read
// with atoi / atof below take what those take: a leading number, else 0.)
bool int_in_range(const std::string &v, long lo, long hi, long &out)
{
    char *end = nullptr;
    out = std::strtol(v.c_str(), &end, 10);
    return !v.empty() && !*end && out >= lo && out <= hi;
}

// a NaN fails both comparisons
bool number_in_range(const std::string &v, double lo, double hi, double &out)
{
    char *end = nullptr;
    out = std::strtod(v.c_str(), &end);
    return !v.empty() && !*end && out >= lo && out <= hi;
}

// the index of `v` among `words`, -1 when it is none of them
int one_of(const std::string &v, std::initializer_list<const char *> words)
{
    int k = 0;
    for (const char *w : words) {
        if (v == w)
            return k;
        ++k;
    }
    return -1;
}

// the options that take no value; false when `o` is not one of them
bool set_flag(const std::string &o, Args &a)
{
    if (o == "--multi") a.force_multi = true;
    else if (o == "--filter") a.do_filter = true;
    else if (o == "--check-only") a.check_only = true;
    else if (o == "--depth-normals") a.depth_normals = true;
    else if (o == "--fuse-clean-radius-only") a.fuse_clean_radius_only = true;
    else if (o == "--mesh-smooth-free-boundary") a.mesh_smooth_free_boundary = true;
    else if (o == "--mesh-normals") a.mesh_normals = true;
    else if (o == "--mesh-decimate-quadric") a.mesh_decimate_quadric = true;
    else if (o == "--mesh-depth-normals") a.mesh_depth_normals = true;
    else if (o == "--mesh-cull-back") a.mesh_cull_back = true;
    else if (o == "--mesh-colour") a.mesh_colour = true;
    else if (o == "--mesh-colour-bilinear") a.mesh_colour_bilinear = true;
    else if (o == "--eval-mesh-surface") a.eval_mesh_surface = true;
    else if (o == "--eval-align") a.eval_align = true;
    else if (o == "--eval-align-scale") a.eval_align_scale = true;
    else if (o == "--eval-normals") a.eval_normals = true;
    else if (o == "--epipolar-matching") a.matcher.epipolar_matching = 1;
    else return false;
    return true;
}

} // namespace

Parse parse_args(int argc, char **argv, Args &a, std::string &error)
{
    error.clear();
    int fast_iters = -1, fast_gradient = -1; // < 0: the library's default
    for (int i = 1; i < argc; ++i) {
        const std::string o = argv[i];
        if (o == "-h" || o == "--help")
            return Parse::Help;
        if (set_flag(o, a))
            continue;
        // every other option takes one value
        if (i + 1 >= argc)
            return Parse::UsageError;
        const std::string v = argv[++i];
        long k = 0;
        double t = 0.0;
        int w = 0;
        if (o == "-i" || o == "--input") a.input = v;
        else if (o == "-s" || o == "--settings") a.settings = v;
        else if (o == "-o" || o == "--output") a.output = v;
        else if (o == "--seeds") a.seeds_path = v;
        else if (o == "--synthetic") a.synth = v;
        else if (o == "--write-scene") a.scene_dir = v;
        else if (o == "--depth-maps") a.depth_dir = v;
        else if (o == "--mesh-depth-maps") a.mesh_depth_dir = v;
        else if (o == "--fuse") a.fuse_path = v;
        else if (o == "--evaluate") a.eval_path = v;
        else if (o == "--device") a.device = std::atoi(v.c_str());
        else if (o == "--gpus") a.gpus = std::atoi(v.c_str());
        else if (o == "--replicate-below") a.replicate_below = std::atoll(v.c_str());
        else if (o == "--max-pops") a.max_pops = std::atoll(v.c_str());
        else if (o == "--level") a.level = std::atoi(v.c_str());
        else if (o == "--features") a.matcher.n_features = std::atoi(v.c_str());
        else if (o == "--fast-threshold") a.matcher.fast_threshold = std::atoi(v.c_str());
        else if (o == "--akaze-threshold") a.matcher.akaze_threshold = (float)std::atof(v.c_str());
        else if (o == "--fast-iters") fast_iters = std::atoi(v.c_str());
        else if (o == "--fast-gradient") fast_gradient = std::atoi(v.c_str());
        else if (o == "--iterations") {
            a.iterations = std::atoi(v.c_str());
            if (a.iterations < 1 || a.iterations > 16)
                error = "--iterations expects 1..16";
        } else if (o == "--splat-scale") {
            a.splat_scale = std::atof(v.c_str());
            if (!(a.splat_scale > 0.0))
                error = "--splat-scale expects a positive number";
        } else if (o == "--fuse-min-views") {
            if (int_in_range(v, 0, 63, k))
                a.fuse.min_views = (int32_t)k;
            else
                error = "--fuse-min-views expects 0..63";
        } else if (o == "--fuse-depth-tol") {
            if (number_in_range(v, 0.0, 3.0e38, t))
                a.fuse.depth_tol = (float)t;
            else
                error = "--fuse-depth-tol expects a finite number >= 0";
        } else if (o == "--fuse-clean-k") {
            if (int_in_range(v, 1, 32, k))
                a.fuse_clean_k = (int)k;
            else
                error = "--fuse-clean-k expects 1..32";
        } else if (o == "--fuse-clean-radius") {
            if (number_in_range(v, 0.0, 3.0e38, t) && (float)t > 0.0f)
                a.fuse_clean_radius = t;
            else
                error = "--fuse-clean-radius expects a finite number > 0";
        } else if (o == "--fuse-clean-std") {
            if (number_in_range(v, 0.0, 3.0e38, t))
                a.fuse_clean_std = t;
            else
                error = "--fuse-clean-std expects a finite number >= 0";
        } else if (o == "--fuse-clean-min-neighbours") {
            if (int_in_range(v, 1, 32, k))
                a.fuse_clean_min_neighbours = (int)k;
            else
                error = "--fuse-clean-min-neighbours expects 1..32";
        } else if (o == "--refine-maps") {
            if (int_in_range(v, 0, 64, k))
                a.refine_passes = (int)k;
            else
                error = "--refine-maps expects 0..64";
        } else if (o == "--refine-window") {
            if (int_in_range(v, 3, 11, k) && (k & 1))
                a.refine_window = (int)k;
            else
                error = "--refine-window expects an odd number in 3..11";
        } else if (o == "--refine-min-ncc") {
            if (number_in_range(v, -1.0, 1.0, t))
                a.refine_min_ncc = t;
            else
                error = "--refine-min-ncc expects a number in -1..1";
        } else if (o == "--mesh") {
            a.mesh_path = v;
        } else if (o == "--mesh-dim") {
            if (int_in_range(v, 2, 1024, k))
                a.mesh_dim = (int)k;
            else
                error = "--mesh-dim expects 2..1024";
        } else if (o == "--mesh-voxel") {
            if (number_in_range(v, 0.0, 3.0e38, t) && t > 0.0)
                a.mesh_voxel = t;
            else
                error = "--mesh-voxel expects a finite number > 0";
        } else if (o == "--mesh-trunc") {
            if (number_in_range(v, 0.0, 3.0e38, t) && t > 0.0)
                a.mesh_trunc = t;
            else
                error = "--mesh-trunc expects a finite number > 0";
        } else if (o == "--mesh-min-weight") {
            if (int_in_range(v, 1, 64, k))
                a.mesh_min_weight = (int)k;
            else
                error = "--mesh-min-weight expects 1..64";
        } else if (o == "--mesh-min-component") {
            if (int_in_range(v, 0, 2147483647L, k))
                a.mesh_min_component = k;
            else
                error = "--mesh-min-component expects 0..2147483647";
        } else if (o == "--mesh-min-component-frac") {
            if (number_in_range(v, 0.0, 1.0, t))
                a.mesh_min_component_frac = t;
            else
                error = "--mesh-min-component-frac expects a number in 0..1";
        } else if (o == "--mesh-keep-largest") {
            if (int_in_range(v, 1, 2147483647L, k))
                a.mesh_keep_largest = k;
            else
                error = "--mesh-keep-largest expects 1..2147483647";
        } else if (o == "--mesh-smooth") {
            if (int_in_range(v, 0, 1000, k))
                a.mesh_smooth = (int)k;
            else
                error = "--mesh-smooth expects 0..1000";
        } else if (o == "--mesh-smooth-lambda") {
            if (number_in_range(v, 0.0, 1.0, t) && (float)t > 0.0f)
                a.mesh_smooth_lambda = t;
            else
                error = "--mesh-smooth-lambda expects a number in (0, 1]";
        } else if (o == "--mesh-smooth-mu") {
            if (number_in_range(v, -3.0e38, 0.0, t))
                a.mesh_smooth_mu = t;
            else
                error = "--mesh-smooth-mu expects a finite number <= 0";
        } else if (o == "--mesh-decimate") {
            if (number_in_range(v, 0.0, 3.0e38, t) && t > 0.0)
                a.mesh_decimate = t;
            else
                error = "--mesh-decimate expects a finite number > 0";
        } else if (o == "--mesh-colour-tol") {
            if (number_in_range(v, 0.0, 3.0e38, t))
                a.mesh_colour_tol = t;
            else
                error = "--mesh-colour-tol expects a finite number >= 0";
        } else if (o == "--mesh-colour-min-cos") {
            if (number_in_range(v, 0.0, 1.0, t))
                a.mesh_colour_min_cos = t;
            else
                error = "--mesh-colour-min-cos expects a number in 0..1";
        } else if (o == "--eval-tau") {
            if (number_in_range(v, 0.0, 3.0e38, t) && (float)t > 0.0f)
                a.eval_tau = t;
            else
                error = "--eval-tau expects a finite number > 0";
        } else if (o == "--eval-max-dist") {
            if (number_in_range(v, 0.0, 3.0e38, t) && (float)t > 0.0f)
                a.eval_max_dist = t;
            else
                error = "--eval-max-dist expects a finite number > 0";
        } else if (o == "--eval-align-iterations") {
            if (int_in_range(v, 1, 1000, k))
                a.eval_align_iterations = (int)k;
            else
                error = "--eval-align-iterations expects 1..1000";
        } else if (o == "--eval-align-radius") {
            if (number_in_range(v, 0.0, 3.0e38, t) && (float)t > 0.0f)
                a.eval_align_radius = t;
            else
                error = "--eval-align-radius expects a finite number > 0";
        } else if (o == "--eval-normals-k") {
            if (int_in_range(v, 3, 32, k))
                a.eval_normals_k = (int)k;
            else
                error = "--eval-normals-k expects 3..32";
        } else if (o == "--eval-normals-radius") {
            if (number_in_range(v, 0.0, 3.0e38, t) && (float)t > 0.0f)
                a.eval_normals_radius = t;
            else
                error = "--eval-normals-radius expects a finite number > 0";
        } else if (o == "--exchange") {
            a.exchange_mode = v;
            if (one_of(v, {"auto", "rccl", "copy"}) < 0)
                error = "--exchange expects auto, rccl or copy";
        } else if (o == "--matcher") {
            if ((w = one_of(v, {"knn", "flann"})) < 0)
                error = "--matcher expects knn or flann";
            else
                a.matcher.matcher_type = w == 0 ? DP_MATCHER_KNN : DP_MATCHER_FLANN;
        } else if (o == "--detector") {
            if ((w = one_of(v, {"orb", "akaze"})) < 0)
                error = "--detector expects orb or akaze";
            else
                a.matcher.detector_type = w == 0 ? DP_DETECTOR_ORB : DP_DETECTOR_AKAZE;
        } else if (o == "--mode") {
            if ((w = one_of(v, {"parity", "fast"})) < 0)
                return Parse::UsageError;
            a.fast.densify = w;
        } else
            return Parse::UsageError; // an option nobody knows
        if (!error.empty())
            return Parse::UsageError;
    }
    if (a.synth.empty() && a.input.empty())
        return Parse::UsageError;
    const bool clean_any = a.fuse_clean_k > 0 || a.fuse_clean_radius > 0.0 || a.fuse_clean_std >= 0.0 ||
                           a.fuse_clean_min_neighbours > 0 || a.fuse_clean_radius_only;
    if (clean_any && a.fuse_path.empty()) {
        error = "--fuse-clean-k, -radius, -std, -min-neighbours and -radius-only need --fuse";
        return Parse::UsageError;
    }
    if (clean_any && !(a.fuse_clean_k > 0 && a.fuse_clean_radius > 0.0)) {
        error = "--fuse-clean-k and --fuse-clean-radius go together, and the other --fuse-clean options need both";
        return Parse::UsageError;
    }
    if (a.fuse_clean_min_neighbours > a.fuse_clean_k) {
        error = "--fuse-clean-min-neighbours expects 1..K of --fuse-clean-k";
        return Parse::UsageError;
    }
    if (a.fuse_clean()) {
        if (a.fuse_clean_std < 0.0)
            a.fuse_clean_std = 2.0;
        if (a.fuse_clean_min_neighbours == 0)
            a.fuse_clean_min_neighbours = 1;
    }
    const bool smooth_detail = a.mesh_smooth_lambda != 0.0 || a.mesh_smooth_mu <= 0.0 || a.mesh_smooth_free_boundary;
    if (a.mesh_path.empty() && (a.mesh_smooth >= 0 || smooth_detail || a.mesh_normals)) {
        error = "--mesh-smooth, its options and --mesh-normals need --mesh";
        return Parse::UsageError;
    }
    if (smooth_detail && a.mesh_smooth < 0) {
        error = "--mesh-smooth-lambda, -mu and -free-boundary need --mesh-smooth";
        return Parse::UsageError;
    }
    if (a.mesh_path.empty() && (a.mesh_decimate > 0.0 || a.mesh_decimate_quadric)) {
        error = "--mesh-decimate and --mesh-decimate-quadric need --mesh";
        return Parse::UsageError;
    }
    if (a.mesh_decimate_quadric && !(a.mesh_decimate > 0.0)) {
        error = "--mesh-decimate-quadric needs --mesh-decimate";
        return Parse::UsageError;
    }
    if (a.mesh_path.empty() && (!a.mesh_depth_dir.empty() || a.mesh_depth_normals || a.mesh_cull_back)) {
        error = "--mesh-depth-maps, --mesh-depth-normals and --mesh-cull-back need --mesh";
        return Parse::UsageError;
    }
    if (a.mesh_depth_dir.empty() && (a.mesh_depth_normals || a.mesh_cull_back)) {
        error = "--mesh-depth-normals and --mesh-cull-back need --mesh-depth-maps";
        return Parse::UsageError;
    }
    const bool colour_detail = a.mesh_colour_bilinear || a.mesh_colour_tol >= 0.0 || a.mesh_colour_min_cos >= 0.0;
    if (a.mesh_path.empty() && (a.mesh_colour || colour_detail)) {
        error = "--mesh-colour and its options need --mesh";
        return Parse::UsageError;
    }
    if (!a.mesh_colour && colour_detail) {
        error = "--mesh-colour-bilinear, -tol and -min-cos need --mesh-colour";
        return Parse::UsageError;
    }
    if (a.eval_path.empty() && (a.eval_tau > 0.0 || a.eval_max_dist > 0.0)) {
        error = "--eval-tau and --eval-max-dist need --evaluate";
        return Parse::UsageError;
    }
    if (a.eval_mesh_surface && (a.eval_path.empty() || a.mesh_path.empty())) {
        error = "--eval-mesh-surface needs --evaluate and --mesh";
        return Parse::UsageError;
    }
    if (!a.eval_align && (a.eval_align_iterations > 0 || a.eval_align_radius > 0.0 || a.eval_align_scale)) {
        error = "--eval-align-iterations, -radius and -scale need --eval-align";
        return Parse::UsageError;
    }
    if (a.eval_align && a.eval_path.empty()) {
        error = "--eval-align needs --evaluate";
        return Parse::UsageError;
    }
    if (!a.eval_normals && (a.eval_normals_k > 0 || a.eval_normals_radius > 0.0)) {
        error = "--eval-normals-k and -radius need --eval-normals";
        return Parse::UsageError;
    }
    if (a.eval_normals && a.eval_path.empty()) {
        error = "--eval-normals needs --evaluate";
        return Parse::UsageError;
    }
    if (!a.eval_path.empty()) {
        if (!(a.eval_tau > 0.0)) {
            error = "--evaluate needs --eval-tau";
            return Parse::UsageError;
        }
        if (a.eval_max_dist == 0.0)
            a.eval_max_dist = 10.0 * a.eval_tau;
        if (!(a.eval_max_dist >= a.eval_tau) || !((float)a.eval_max_dist <= 3.0e38f)) {
            error = "--eval-max-dist expects a finite number of at least --eval-tau";
            return Parse::UsageError;
        }
    }
    if (a.eval_align) {
        if (a.eval_align_iterations == 0)
            a.eval_align_iterations = 30;
        if (a.eval_align_radius == 0.0)
            a.eval_align_radius = a.eval_max_dist;
    }
    if (a.eval_normals) {
        if (a.eval_normals_k == 0)
            a.eval_normals_k = 16;
        if (a.eval_normals_radius == 0.0)
            a.eval_normals_radius = a.eval_max_dist;
    }
    if (a.iterations > 1)
        a.do_filter = true; // the filter is what tells the rounds apart
    if (a.replicate_below < 0)
        a.replicate_below = 1024 * (long long)a.gpus;
    if (fast_iters >= 0)
        a.fast.iters = fast_iters;
    if (fast_gradient >= 0)
        a.fast.gradient = fast_gradient;
    return Parse::Run;
}
