// densify -- command-line front end of the MI355X patch loop.
//
// Mirrors the reference's programs/densify/main.cpp (-i scene.json, -s
// settings.json; PMVS::AddCamera per view, then PMVS::Run) and adds what
// SURVEY 8b asks of the build: -o out.ply (PMVS::PrintCloud format), --seeds
// (seed points from a file instead of Matcher::GenerateSeeds), --device,
// option overrides.  All compute goes through the C ABI of libdensepoints.so
// (include/densepoints.h): dp_set_views, dp_generate_seeds, dp_densify.
// The options: usage() in cli_args.cpp.  main() runs the stages below in order.
#include "cli_args.h"
#include "cli_error.h"
#include "dp_buf.h"
#include "multi_gpu.h"
#include "scene_io.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

namespace {

// settings JSON: any dp_options field by name (reference defaults otherwise)
void apply_settings(const dpio::Json &j, dp_options &o)
{
    if (j.kind != dpio::Json::Object)
        throw std::runtime_error("settings: expected a JSON object");
    for (const auto &kv : j.obj) {
        const std::string &k = kv.first;
        const double v = kv.second.num;
        if (k == "seed_cell_size") o.seed_cell_size = (int32_t)v;
        else if (k == "expand_cell_size") o.expand_cell_size = (int32_t)v;
        else if (k == "grid_scale") o.grid_scale = (int32_t)v;
        else if (k == "max_patches_per_cell") o.max_patches_per_cell = (int32_t)v;
        else if (k == "min_visible") o.min_visible = (int32_t)v;
        else if (k == "min_expand_visible") o.min_expand_visible = (int32_t)v;
        else if (k == "nm_max_evals") o.nm_max_evals = (int32_t)v;
        else if (k == "ncc_threshold") o.ncc_threshold = v;
        else if (k == "visible_angle") o.visible_angle = v;
        else if (k == "candidate_angle") o.candidate_angle = v;
        else if (k == "nm_eps") o.nm_eps = v;
        else if (k == "ncc_denom_min") o.ncc_denom_min = v;
        else if (k == "max_pops") o.max_pops = (int64_t)v;
        else if (k == "nm_step" && kv.second.kind == dpio::Json::Array && kv.second.arr.size() == 3)
            for (int i = 0; i < 3; ++i) o.nm_step[i] = kv.second.arr[i].num;
        else
            throw std::runtime_error("settings: unknown option '" + k + "'");
    }
}

int write_synthetic(const std::string &spec, const std::string &dir)
{
    dp_synth_config cfg;
    dp_synth_default(&cfg);
    if (std::sscanf(spec.c_str(), "%d,%d,%d,%d", &cfg.n_views, &cfg.width, &cfg.height, &cfg.kind) != 4)
        throw std::runtime_error("--synthetic expects V,W,H,KIND");
    std::vector<double> P(12 * (size_t)cfg.n_views);
    if (dp_synth_cameras(&cfg, P.data()) != DP_OK)
        throw std::runtime_error("dp_synth_cameras failed");
    mkdir(dir.c_str(), 0755);
    FILE *js = std::fopen((dir + "/scene.json").c_str(), "wb");
    if (!js)
        throw std::runtime_error("cannot write " + dir + "/scene.json");
    std::fprintf(js, "{\n  \"imagesPath\": \"%s\",\n  \"views\": [\n", dir.c_str());
    for (int v = 0; v < cfg.n_views; ++v) {
        std::vector<uint8_t> bgr((size_t)cfg.width * cfg.height * 3);
        if (dp_synth_render_host(&cfg, P.data(), v, bgr.data()) != DP_OK)
            throw std::runtime_error("dp_synth_render_host failed");
        char name[64];
        std::snprintf(name, sizeof name, "view_%03d.ppm", v);
        dpio::write_ppm(dir + "/" + name, cfg.width, cfg.height, bgr);
        std::fprintf(js, "    {\"filename\": \"%s\", \"projectionMatrix\": [", name);
        for (int r = 0; r < 3; ++r)
            std::fprintf(js, "[%.17g, %.17g, %.17g, %.17g]%s", P[12 * v + 4 * r], P[12 * v + 4 * r + 1],
                         P[12 * v + 4 * r + 2], P[12 * v + 4 * r + 3], r < 2 ? ", " : "");
        std::fprintf(js, "]}%s\n", v + 1 < cfg.n_views ? "," : "");
    }
    std::fprintf(js, "  ]\n}\n");
    std::fclose(js);
    const int64_t n = dp_synth_seeds(&cfg, P.data(), nullptr, 0);
    std::vector<double> xyz(3 * (size_t)n);
    dp_synth_seeds(&cfg, P.data(), xyz.data(), n);
    FILE *sf = std::fopen((dir + "/seeds.xyz").c_str(), "wb");
    if (!sf)
        throw std::runtime_error("cannot write seeds.xyz");
    for (int64_t i = 0; i < n; ++i)
        std::fprintf(sf, "%.17g %.17g %.17g\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    std::fclose(sf);
    std::printf("{\"scene\": \"%s/scene.json\", \"views\": %d, \"seeds\": %lld}\n", dir.c_str(), cfg.n_views,
                (long long)n);
    return 0;
}

struct SceneData {
    dp_options opt;
    std::vector<dpio::Image> imgs;
    std::vector<double> P;     // 12 per view
    std::vector<double> seeds; // xyz triples: of --seeds, else generate_or_read_seeds fills them
    std::vector<double> truth; // xyz triples of --evaluate
};

SceneData load_scene(const Args &args)
{
    SceneData sc;
    dp_default_options(&sc.opt);
    if (!args.settings.empty())
        apply_settings(dpio::parse_json(dpio::read_file(args.settings)), sc.opt);
    if (args.max_pops >= 0)
        sc.opt.max_pops = args.max_pops;
    for (const dpio::SceneView &v : dpio::read_scene(args.input).views) {
        sc.imgs.push_back(dpio::load_image(v.filename)); // PMVS::AddCamera -> View::Load
        sc.P.insert(sc.P.end(), v.P, v.P + 12);
    }
    if (!args.seeds_path.empty())
        sc.seeds = dpio::read_seeds(args.seeds_path);
    if (!args.eval_path.empty()) {
        sc.truth = dpio::read_seeds(args.eval_path);
        if (sc.truth.size() / 3 > 0x7FFFFFFFull)
            throw std::runtime_error("--evaluate: more than 2^31 - 1 points");
    }
    return sc;
}

// parsed scene summary + FNV-1a of each decoded BGR8 image (no GPU)
void print_check_only(const SceneData &sc)
{
    const std::vector<dpio::Image> &imgs = sc.imgs;
    std::printf("{\"views\": %zu, \"width\": %d, \"height\": %d, \"seeds\": %zu, \"image_fnv\": [", imgs.size(),
                imgs.empty() ? 0 : imgs[0].width, imgs.empty() ? 0 : imgs[0].height, sc.seeds.size() / 3);
    for (size_t v = 0; v < imgs.size(); ++v) {
        uint64_t h = 1469598103934665603ull;
        for (uint8_t b : imgs[v].bgr)
            h = (h ^ b) * 1099511628211ull;
        std::printf("%s\"%016llx\"", v ? ", " : "", (unsigned long long)h);
    }
    std::printf("]");
    if (!sc.truth.empty()) // --evaluate
        std::printf(", \"truth\": %zu", sc.truth.size() / 3);
    std::printf("}\n");
}

struct CtxDestroy {
    void operator()(dp_ctx *c) const { dp_ctx_destroy(c); }
};
using CtxPtr = std::unique_ptr<dp_ctx, CtxDestroy>;

// a library call on the first context
void check(dp_ctx *ctx, int rc, const char *what)
{
    if (rc != DP_OK)
        throw CliError(what, rc, dp_last_error(ctx));
}

// A context on `device` with the scene's views, the fast options and, for
// level > 0, the pyramid up to that level (cv::pyrDown^L on the device, P rows
// 0-1 / 2^L).  `existing` is the number of contexts made before this one: a
// failure on a later context says so, with the count of contexts that exist.
CtxPtr make_context(const SceneData &sc, int device, const dp_fast_options &fo, int level, size_t existing)
{
    dp_ctx *raw = nullptr;
    const int crc = dp_ctx_create(&sc.opt, device, &raw);
    CtxPtr ctx(raw);
    if (crc != DP_OK && existing == 0)
        throw CliError("dp_ctx_create failed (" + std::to_string(crc) + ")");
    auto ok = [&](int rc, const char *what, size_t count) {
        if (rc != DP_OK)
            throw CliError(what, rc, raw ? dp_last_error(raw) : "context not created",
                           existing ? "on context " + std::to_string(count) : "");
    };
    ok(crc, "dp_ctx_create", existing);
    std::vector<dp_image> dimg(sc.imgs.size());
    for (size_t v = 0; v < dimg.size(); ++v)
        dimg[v] = dp_image{sc.imgs[v].width, sc.imgs[v].height, 3 * sc.imgs[v].width, 0, sc.imgs[v].bgr.data()};
    ok(dp_set_views(raw, (int)dimg.size(), sc.P.data(), dimg.data()), "dp_set_views", existing + 1);
    ok(dp_set_fast_options(raw, &fo), "dp_set_fast_options", existing + 1);
    if (level > 0) {
        ok(dp_build_pyramid(raw, level + 1), "dp_build_pyramid", existing + 1);
        ok(dp_set_level(raw, level), "dp_set_level", existing + 1);
    }
    return ctx;
}

// PMVS::InsertSeeds (pmvs.cpp:29-34): without --seeds the seeds come from
// Matcher::GenerateSeeds on the device (level-0 views); with it, load_scene
// has read them
dp_seed_stats generate_or_read_seeds(dp_ctx *ctx, const Args &args, SceneData &sc)
{
    dp_seed_stats sst;
    std::memset(&sst, 0, sizeof sst);
    if (args.seeds_path.empty()) {
        const double *xyz = nullptr;
        int64_t n = 0;
        check(ctx, dp_generate_seeds(ctx, &args.matcher, &xyz, &n, &sst), "dp_generate_seeds");
        sc.seeds.assign(xyz, xyz + 3 * n);
    }
    return sst;
}

dp_filter_options default_filter()
{
    dp_filter_options f;
    dp_default_filter_options(&f);
    return f;
}

// --gpus N / --multi: contexts 1..N-1 on the next devices (wrapping: several
// ranks may share a GPU), released when the run is over
DensifyResult run_multi(dp_ctx *ctx, const Args &args, const SceneData &sc)
{
    const int ndev = dp_device_count();
    std::vector<CtxPtr> more;
    MultiInput in{{ctx}, {args.device}, args.exchange_mode, args.replicate_below, args.iterations, default_filter()};
    for (int g = 1; g < args.gpus; ++g) {
        const int dg = (args.device + g) % (ndev > 0 ? ndev : 1);
        more.push_back(make_context(sc, dg, args.fast, args.level, (size_t)g));
        in.ctxs.push_back(more.back().get());
        in.devices.push_back(dg);
    }
    return densify_multi(in, sc.seeds);
}

DensifyResult run_densify(dp_ctx *ctx, const Args &args, const SceneData &sc)
{
    if (args.gpus > 1 || args.force_multi)
        return run_multi(ctx, args, sc);
    DensifyResult res;
    const int n = (int)(sc.seeds.size() / 3);
    if (args.iterations > 1) {
        // expansion and filter alternated on the device (dp_densify_iterate)
        const dp_filter_options filt = default_filter();
        res.rounds.assign((size_t)args.iterations, dp_iterate_stats{});
        check(ctx,
              dp_densify_iterate(ctx, sc.seeds.data(), n, args.iterations, &filt, &res.patches, &res.n, &res.stats,
                                 res.rounds.data()),
              "dp_densify_iterate");
        res.filtered = true;
    } else {
        check(ctx, dp_densify(ctx, sc.seeds.data(), n, &res.patches, &res.n, &res.stats), "dp_densify");
    }
    return res;
}

// PMVS::FilterPatches (pmvs.h:27, undefined in the reference): dp_filter_patches
// spec.  The patches that are written, rendered and fused.
std::vector<dp_patch> filter_survivors(dp_ctx *ctx, const Args &args, const DensifyResult &res)
{
    std::vector<uint8_t> keep((size_t)res.n, 1);
    if (args.do_filter && !res.filtered && res.n > 0) {
        const dp_filter_options filt = default_filter();
        check(ctx, dp_filter_patches(ctx, res.patches, res.n, &filt, keep.data()), "dp_filter_patches");
    }
    std::vector<dp_patch> kept;
    kept.reserve((size_t)res.n);
    for (int64_t i = 0; i < res.n; ++i)
        if (keep[(size_t)i])
            kept.push_back(res.patches[i]);
    return kept;
}

// any record with pos / normal / rgb as a point of the PLY
template <typename T> std::vector<dpio::CloudPoint> to_cloud(const std::vector<T> &recs)
{
    std::vector<dpio::CloudPoint> cloud(recs.size());
    for (size_t i = 0; i < recs.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            cloud[i].pos[k] = recs[i].pos[k];
            cloud[i].normal[k] = recs[i].normal[k];
            cloud[i].rgb[k] = recs[i].rgb[k];
        }
    return cloud;
}

dp_render_options render_options(const Args &args)
{
    dp_render_options ro;
    dp_default_render_options(&ro);
    ro.splat_scale = (float)args.splat_scale;
    return ro;
}

dp_mapref_options mapref_options(const Args &args)
{
    dp_mapref_options mo;
    dp_default_mapref_options(&mo);
    if (args.refine_window > 0)
        mo.window = args.refine_window;
    if (args.refine_min_ncc >= -1.0)
        mo.min_ncc = (float)args.refine_min_ncc;
    return mo;
}

// the report's member of the last --refine-maps pass
std::string refined_report(const char *name, int passes, const dp_mapref_stats &ms, double total_ms)
{
    char buf[320];
    std::snprintf(buf, sizeof buf,
                  ", \"%s\": {\"passes\": %d, \"kept\": %lld, \"filled\": %lld, \"moved\": %lld, \"candidates\": %lld, "
                  "\"refine_ms\": %.3f}",
                  name, passes, (long long)ms.kept, (long long)ms.filled, (long long)ms.moved,
                  (long long)ms.candidates, total_ms);
    return buf;
}

// --depth-maps with --refine-maps N: the refinement reads every view's planes,
// so all views are rendered first (with normals, which it needs), refined N
// times on the host form, then written: depth, score, and normal when asked.
std::string write_refined_depth_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept)
{
    const dp_render_options ro = render_options(args);
    const dp_mapref_options mo = mapref_options(args);
    std::vector<int32_t> vid((size_t)V), ws((size_t)V), hs((size_t)V);
    std::vector<std::vector<float>> depth[2], normal[2];
    std::vector<std::vector<float>> score((size_t)V);
    for (int b = 0; b < 2; ++b) {
        depth[b].resize((size_t)V);
        normal[b].resize((size_t)V);
    }
    std::vector<float *> pd[2], pn[2], ps((size_t)V);
    for (int b = 0; b < 2; ++b) {
        pd[b].resize((size_t)V);
        pn[b].resize((size_t)V);
    }
    for (int32_t v = 0; v < V; ++v) {
        check(ctx, dp_level_info(ctx, args.level, v, &ws[(size_t)v], &hs[(size_t)v], nullptr), "dp_level_info");
        const size_t px = (size_t)ws[(size_t)v] * hs[(size_t)v];
        vid[(size_t)v] = v;
        for (int b = 0; b < 2; ++b) {
            depth[b][(size_t)v].assign(px, 0.0f);
            normal[b][(size_t)v].assign(px * 3, 0.0f);
            pd[b][(size_t)v] = depth[b][(size_t)v].data();
            pn[b][(size_t)v] = normal[b][(size_t)v].data();
        }
        score[(size_t)v].assign(px, 0.0f);
        ps[(size_t)v] = score[(size_t)v].data();
    }
    dp_render_stats rs;
    check(ctx,
          dp_render_maps(ctx, kept.data(), (int64_t)kept.size(), nullptr, vid.data(), V, &ro, pd[0].data(), nullptr,
                         pn[0].data(), nullptr, &rs),
          "dp_render_maps");
    dp_mapref_stats ms{};
    double refine_ms = 0.0;
    int cur = 0;
    for (int pass = 0; pass < args.refine_passes; ++pass, cur ^= 1) {
        check(ctx,
              dp_refine_maps(ctx, vid.data(), V, &mo, nullptr, pd[cur].data(), pn[cur].data(), pd[cur ^ 1].data(),
                             pn[cur ^ 1].data(), ps.data(), nullptr, &ms),
              "dp_refine_maps");
        refine_ms += ms.refine_ms;
    }
    for (int32_t v = 0; v < V; ++v) {
        char name[64];
        std::snprintf(name, sizeof name, "/depth_%04d.pfm", (int)v);
        dpio::write_pfm(args.depth_dir + name, pd[cur][(size_t)v], ws[(size_t)v], hs[(size_t)v], 1);
        std::snprintf(name, sizeof name, "/score_%04d.pfm", (int)v);
        dpio::write_pfm(args.depth_dir + name, ps[(size_t)v], ws[(size_t)v], hs[(size_t)v], 1);
        if (args.depth_normals) {
            std::snprintf(name, sizeof name, "/normal_%04d.pfm", (int)v);
            dpio::write_pfm(args.depth_dir + name, pn[cur][(size_t)v], ws[(size_t)v], hs[(size_t)v], 3);
        }
    }
    char buf[160];
    std::snprintf(buf, sizeof buf, ", \"depth_maps\": {\"views\": %zu, \"covered_pixels\": %lld, \"render_ms\": %.3f}",
                  (size_t)V, (long long)rs.covered_pixels, rs.render_ms);
    return buf + refined_report("refined_maps", args.refine_passes, ms, refine_ms);
}

// --depth-maps: the written patches as per-view depth (and normal) maps of
// the level the densify ran on (dp_render_maps), one view at a time; with
// --gpus N this context (rank 0) renders, the store being replicated.
// Returns the report's "depth_maps" member.
std::string write_depth_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept)
{
    if (mkdir(args.depth_dir.c_str(), 0777) != 0 && errno != EEXIST)
        throw std::runtime_error("cannot create " + args.depth_dir);
    if (args.refine_passes > 0)
        return write_refined_depth_maps(ctx, args, V, kept);
    const dp_render_options ro = render_options(args);
    int64_t covered = 0;
    double render_ms = 0.0;
    std::vector<float> depth, normal;
    for (int32_t v = 0; v < V; ++v) {
        int32_t w = 0, h = 0;
        check(ctx, dp_level_info(ctx, args.level, v, &w, &h, nullptr), "dp_level_info");
        depth.assign((size_t)w * h, 0.0f);
        if (args.depth_normals)
            normal.assign((size_t)w * h * 3, 0.0f);
        float *pd = depth.data(), *pn = args.depth_normals ? normal.data() : nullptr;
        dp_render_stats rs;
        check(ctx,
              dp_render_maps(ctx, kept.data(), (int64_t)kept.size(), nullptr, &v, 1, &ro, &pd, nullptr,
                             args.depth_normals ? &pn : nullptr, nullptr, &rs),
              "dp_render_maps");
        covered += rs.covered_pixels;
        render_ms += rs.render_ms;
        char name[64];
        std::snprintf(name, sizeof name, "/depth_%04d.pfm", (int)v);
        dpio::write_pfm(args.depth_dir + name, pd, w, h, 1);
        if (args.depth_normals) {
            std::snprintf(name, sizeof name, "/normal_%04d.pfm", (int)v);
            dpio::write_pfm(args.depth_dir + name, pn, w, h, 3);
        }
    }
    char buf[160];
    std::snprintf(buf, sizeof buf, ", \"depth_maps\": {\"views\": %zu, \"covered_pixels\": %lld, \"render_ms\": %.3f}",
                  (size_t)V, (long long)covered, render_ms);
    return buf;
}

// The first stage of --fuse and --mesh alike: depth and normal maps of every
// view rendered into device planes (dp_render_maps_device, honouring
// --splat-scale) and, with --refine-maps N, refined there.  DeviceMaps owns the
// planes (and whatever else its user allocates through bytes()); `cap` bounds
// the pixels that hold a depth.
struct DeviceMaps {
    std::vector<dpk::DevMem> mem;
    std::vector<int32_t> vid;
    std::vector<float *> depth, normal;
    int64_t cap = 0;
    std::string refined; // the report's member of --refine-maps, empty without it

    void *bytes(size_t n, const char *who)
    {
        mem.emplace_back();
        if (mem.back().alloc(n ? n : 1) != hipSuccess)
            throw std::runtime_error(std::string(who) + ": out of device memory");
        return mem.back().p;
    }
};

// --evaluate: the ground-truth points on the device and, per evaluated cloud,
// the report's entry.  A cloud is searched where it lies (dp_cloud_nearest_device,
// both directions, radius --eval-max-dist); only index and dist come back, and
// the host sums the matched distances in fp64 in index order.
struct Evaluation {
    dp_ctx *ctx = nullptr;
    double tau = 0.0;
    float max_dist = 0.0f;
    int64_t n_truth = 0;
    DeviceMaps mem;
    float *d_truth = nullptr;
    std::string entries; // "name": {...}, ...
    // --eval-align: the options, the transform once it is estimated, the report's member
    dp_cloud_align_options align_opts{};
    bool align = false, aligned = false;
    double M[12] = {0};
    std::string align_json;
    // --eval-normals: the options and the truth's normals once they are estimated
    dp_cloud_normals_options normals_opts{};
    bool normals = false;
    float *d_truth_normal = nullptr;

    Evaluation(dp_ctx *c, const Args &args, const std::vector<double> &truth)
        : ctx(c), tau(args.eval_tau), max_dist((float)args.eval_max_dist), n_truth((int64_t)(truth.size() / 3)),
          align(args.eval_align)
    {
        align_opts.max_dist = (float)args.eval_align_radius;
        align_opts.iterations = args.eval_align_iterations;
        align_opts.min_pairs = 3;
        align_opts.flags = args.eval_align_scale ? DP_CLOUD_ALIGN_SCALE : 0;
        align_opts.rms_tol = 0.0;
        normals = args.eval_normals;
        normals_opts.max_dist = (float)args.eval_normals_radius;
        normals_opts.k = args.eval_normals_k;
        normals_opts.min_neighbours = 3;
        normals_opts.flags = 0;
        std::vector<float> xyz(truth.begin(), truth.end());
        d_truth = (float *)mem.bytes(xyz.size() * sizeof(float), "--evaluate");
        if (!xyz.empty() && hipMemcpy(d_truth, xyz.data(), xyz.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("--evaluate: copy of the ground truth failed");
    }

    // d[lo] + (d[min(lo + 1, m - 1)] - d[lo]) * (pos - lo), pos = p (m - 1), of ascending values
    static double quantile(const std::vector<double> &d, double p)
    {
        if (d.empty())
            return std::nan("");
        const double pos = p * (double)(d.size() - 1);
        const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, d.size() - 1);
        return d[lo] + (d[hi] - d[lo]) * (pos - (double)lo);
    }

    static std::string number(double v)
    {
        if (!std::isfinite(v))
            return "null"; // no distance matched
        char buf[40];
        std::snprintf(buf, sizeof buf, "%.17g", v);
        return buf;
    }

    // the results of one search: nq indices and distances on the device
    struct Found {
        DeviceMaps out;
        int32_t *d_index = nullptr;
        float *d_dist = nullptr;
        Found(int64_t nq)
        {
            d_index = (int32_t *)out.bytes((size_t)nq * 4, "--evaluate");
            d_dist = (float *)out.bytes((size_t)nq * 4, "--evaluate");
        }
    };

    // the matched distances of a search, ascending, and their sum in index order
    static std::vector<double> matched_distances(const Found &f, int64_t nq, double *sum)
    {
        std::vector<int32_t> index((size_t)nq);
        std::vector<float> dist((size_t)nq);
        if (nq > 0 && (hipMemcpy(index.data(), f.d_index, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(dist.data(), f.d_dist, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess))
            throw std::runtime_error("--evaluate: copy of the distances failed");
        std::vector<double> d;
        *sum = 0.0;
        for (size_t i = 0; i < index.size(); ++i)
            if (index[i] >= 0) {
                d.push_back((double)dist[i]);
                *sum += (double)dist[i];
            }
        std::sort(d.begin(), d.end());
        return d;
    }

    // one direction's entry from its search; *ratio = within_tau / n
    std::string entry(const Found &f, int64_t nq, int64_t queries, int64_t matched, double *ratio) const
    {
        double sum = 0.0;
        const std::vector<double> d = matched_distances(f, nq, &sum);
        const int64_t within = (int64_t)(std::upper_bound(d.begin(), d.end(), tau) - d.begin());
        *ratio = queries > 0 ? (double)within / (double)queries : 0.0;
        char buf[200];
        std::snprintf(buf, sizeof buf, "{\"n\": %lld, \"matched\": %lld, \"within_tau\": %lld, \"ratio\": %.17g, ",
                      (long long)queries, (long long)matched, (long long)within, *ratio);
        return std::string(buf) + "\"mean\": " + number(d.empty() ? std::nan("") : sum / (double)d.size()) +
               ", \"median\": " + number(quantile(d, 0.5)) + ", \"p90\": " + number(quantile(d, 0.9)) + "}";
    }

    // --eval-normals: cloud_normal_error of the Python package over the matches of
    // the accuracy direction.  The records' normals lie normal_offset bytes behind
    // their positions; the truth's are estimated by the first call.
    std::string normals_entry(const Found &f, const void *d_q, int64_t nq, int64_t qs, int64_t normal_offset)
    {
        if (!d_truth_normal) {
            d_truth_normal = (float *)mem.bytes((size_t)std::max<int64_t>(n_truth, 1) * 12, "--eval-normals");
            check(ctx,
                  dp_cloud_normals_device(ctx, n_truth ? d_truth : nullptr, n_truth, 12, &normals_opts, nullptr, 0,
                                          d_truth_normal, nullptr, nullptr, nullptr, nullptr),
                  "dp_cloud_normals_device");
        }
        std::vector<int32_t> index((size_t)nq);
        std::vector<float> dist((size_t)nq), truth((size_t)n_truth * 3);
        std::vector<char> recs((size_t)nq * (size_t)qs);
        const size_t head = nq > 0 ? (size_t)(nq - 1) * (size_t)qs + (size_t)normal_offset + 12 : 0;
        if (hipDeviceSynchronize() != hipSuccess ||
            (nq > 0 && (hipMemcpy(index.data(), f.d_index, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(dist.data(), f.d_dist, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(recs.data(), d_q, head, hipMemcpyDeviceToHost) != hipSuccess)) ||
            (n_truth > 0 && hipMemcpy(truth.data(), d_truth_normal, truth.size() * 4, hipMemcpyDeviceToHost) != hipSuccess))
            throw std::runtime_error("--eval-normals: copy of the normals failed");
        std::vector<double> deg;
        double sum = 0.0;
        for (int64_t i = 0; i < nq; ++i) {
            if (index[(size_t)i] < 0 || !((double)dist[(size_t)i] <= tau))
                continue;
            float af[3];
            std::memcpy(af, recs.data() + (size_t)i * (size_t)qs + (size_t)normal_offset, 12);
            const float *bf = truth.data() + 3 * (size_t)index[(size_t)i];
            const double a[3] = {af[0], af[1], af[2]}, b[3] = {bf[0], bf[1], bf[2]};
            bool ok = true, a_any = false, b_any = false;
            for (int k = 0; k < 3; ++k) {
                ok = ok && std::isfinite(a[k]) && std::isfinite(b[k]);
                a_any = a_any || a[k] != 0.0;
                b_any = b_any || b[k] != 0.0;
            }
            if (!ok || !a_any || !b_any)
                continue;
            const double dot = std::fabs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
            const double la = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
            const double lb = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
            const double angle = std::acos(std::min(1.0, dot / (la * lb))) * (180.0 / 3.14159265358979323846);
            deg.push_back(angle);
            sum += angle;
        }
        std::sort(deg.begin(), deg.end());
        char buf[64];
        std::snprintf(buf, sizeof buf, "{\"n\": %lld, ", (long long)deg.size());
        return std::string(buf) + "\"mean_deg\": " + number(deg.empty() ? std::nan("") : sum / (double)deg.size()) +
               ", \"median_deg\": " + number(quantile(deg, 0.5)) + ", \"p90_deg\": " + number(quantile(deg, 0.9)) + "}";
    }

    // one direction between two clouds; normal_offset >= 0: the entry of the queries' normals into *normals_json
    std::string side(const void *d_q, int64_t nq, int64_t qs, const void *d_t, int64_t nt, int64_t ts, double *ratio,
                     int64_t normal_offset = -1, std::string *normals_json = nullptr)
    {
        Found f(nq);
        const dp_cloud_nearest_options o{max_dist, 0, 0};
        dp_cloud_nearest_stats st;
        check(ctx,
              dp_cloud_nearest_device(ctx, nq ? d_q : nullptr, nq, qs, nt ? d_t : nullptr, nt, ts, &o, f.d_index, f.d_dist,
                                      nullptr, &st, nullptr),
              "dp_cloud_nearest_device");
        if (normal_offset >= 0)
            *normals_json = normals_entry(f, d_q, nq, qs, normal_offset);
        return entry(f, nq, st.queries, st.matched, ratio);
    }

    // points against the surface of a device mesh (dp_mesh_nearest_device)
    dp_mesh_nearest_stats surface(const Found &f, const void *d_q, int64_t nq, int64_t qs, const dp_mesh_vertex *d_v,
                                  int64_t nv, const int32_t *d_t, int64_t nt)
    {
        const dp_mesh_nearest_options o{max_dist, 0, 0};
        dp_mesh_nearest_stats st;
        check(ctx,
              dp_mesh_nearest_device(ctx, nq ? d_q : nullptr, nq, qs, nv ? d_v : nullptr, nv, nt ? d_t : nullptr, nt, &o,
                                     f.d_index, f.d_dist, nullptr, nullptr, &st, nullptr),
              "dp_mesh_nearest_device");
        return st;
    }

    // --eval-mesh-surface: the mesh's vertices against the truth and the truth
    // against the mesh's surface
    void add_mesh_surface(const dp_mesh_vertex *d_v, int64_t nv, const int32_t *d_t, int64_t nt)
    {
        DeviceMaps copy;
        d_v = (const dp_mesh_vertex *)moved(copy, d_v, nv, sizeof(dp_mesh_vertex));
        double p = 0.0, r = 0.0;
        const std::string acc = side(d_v, nv, sizeof(dp_mesh_vertex), d_truth, n_truth, 12, &p);
        Found f(n_truth);
        const dp_mesh_nearest_stats st = surface(f, d_truth, n_truth, 12, d_v, nv, d_t, nt);
        const std::string com = entry(f, n_truth, st.queries, st.matched, &r);
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.17g", p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0);
        entries += std::string(entries.empty() ? "" : ", ") + "\"mesh_surface\": {\"accuracy\": " + acc +
                   ", \"completeness\": " + com + ", \"fscore\": " + buf + "}";
    }

    // the vertices of one mesh against the surface of another: the entry and the largest distance
    std::string deviation_side(const dp_mesh_vertex *d_q, int64_t nq, const dp_mesh_vertex *d_v, int64_t nv,
                               const int32_t *d_t, int64_t nt, double *top)
    {
        Found f(nq);
        const dp_mesh_nearest_stats st = surface(f, d_q, nq, sizeof(dp_mesh_vertex), d_v, nv, d_t, nt);
        double sum = 0.0;
        const std::vector<double> d = matched_distances(f, nq, &sum);
        *top = d.empty() ? std::nan("") : d.back();
        char buf[120];
        std::snprintf(buf, sizeof buf, "{\"n\": %lld, \"matched\": %lld, ", (long long)st.queries, (long long)st.matched);
        return std::string(buf) + "\"mean\": " + number(d.empty() ? std::nan("") : sum / (double)d.size()) +
               ", \"median\": " + number(quantile(d, 0.5)) + ", \"p90\": " + number(quantile(d, 0.9)) +
               ", \"max\": " + number(*top) + "}";
    }

    // --eval-mesh-surface with --mesh-decimate: mesh a (before) and mesh b (after), both ways
    void add_deviation(const char *name, const dp_mesh_vertex *d_va, int64_t nva, const int32_t *d_ta, int64_t nta,
                       const dp_mesh_vertex *d_vb, int64_t nvb, const int32_t *d_tb, int64_t ntb)
    {
        double ta = 0.0, tb = 0.0;
        const std::string ab = deviation_side(d_va, nva, d_vb, nvb, d_tb, ntb, &ta);
        const std::string ba = deviation_side(d_vb, nvb, d_va, nva, d_ta, nta, &tb);
        const double top = std::isnan(ta) ? tb : (std::isnan(tb) ? ta : std::max(ta, tb));
        entries += std::string(entries.empty() ? "" : ", ") + "\"" + name + "\": {\"a_to_b\": " + ab + ", \"b_to_a\": " +
                   ba + ", \"max\": " + number(top) + "}";
    }

    // --eval-align: the transform that moves the cloud onto the truth (dp_cloud_align_device)
    void estimate(const void *d_points, int64_t n, int64_t stride)
    {
        std::vector<dp_cloud_align_step> trace((size_t)align_opts.iterations + 1);
        dp_cloud_align_stats st;
        double scale = 1.0;
        check(ctx,
              dp_cloud_align_device(ctx, n ? d_points : nullptr, n, stride, n_truth ? d_truth : nullptr, n_truth, 12,
                                    &align_opts, nullptr, M, &scale, trace.data(), nullptr, nullptr, &st, nullptr),
              "dp_cloud_align_device");
        aligned = true;
        const dp_cloud_align_step &last = trace[(size_t)st.iterations_run];
        align_json = ", \"align\": {\"matrix\": [";
        for (int k = 0; k < 12; ++k)
            align_json += std::string(k ? ", " : "") + number(M[k]);
        char buf[120];
        std::snprintf(buf, sizeof buf, ", \"iterations\": %lld, \"matched\": %lld, ", (long long)st.iterations_run,
                      (long long)last.matched);
        align_json += "], \"scale\": " + number(scale) + buf + "\"rms_before\": " + number(trace[0].rms) +
                      ", \"rms\": " + number(last.rms) + "}";
    }

    // --eval-align: a copy of n records (the position first) under the transform,
    // their normals with them when normal_offset >= 0; without it the records themselves
    const void *moved(DeviceMaps &copy, const void *d_records, int64_t n, int64_t stride, int64_t normal_offset = -1)
    {
        if (!aligned)
            return d_records;
        void *d = copy.bytes((size_t)n * (size_t)stride, "--eval-align");
        check(ctx, dp_cloud_transform_device(ctx, n ? d_records : nullptr, n, stride, M, normal_offset, d, nullptr),
              "dp_cloud_transform_device");
        return d;
    }

    // the cloud of n points at d_points (device memory, `stride` bytes apart, each the head
    // of its record) against the truth; normal_offset: where a record's normal
    // lies, for --eval-normals (-1: the records have none)
    void add(const char *name, const void *d_points, int64_t n, int64_t stride, int64_t normal_offset = -1)
    {
        static_assert(offsetof(dp_patch, pos) == 0 && offsetof(dp_fused_point, pos) == 0 &&
                          offsetof(dp_mesh_vertex, pos) == 0,
                      "moved() copies records from their positions on");
        if (align && !aligned)
            estimate(d_points, n, stride); // the first cloud added: the written patches
        DeviceMaps copy;
        if (!normals)
            normal_offset = -1;
        d_points = moved(copy, d_points, n, stride, normal_offset);
        double p = 0.0, r = 0.0;
        std::string normals_json;
        const std::string acc = side(d_points, n, stride, d_truth, n_truth, 12, &p, normal_offset, &normals_json);
        const std::string com = side(d_truth, n_truth, 12, d_points, n, stride, &r);
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.17g", p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0);
        entries += std::string(entries.empty() ? "" : ", ") + "\"" + name + "\": {\"accuracy\": " + acc +
                   ", \"completeness\": " + com + ", \"fscore\": " + buf +
                   (normal_offset >= 0 ? ", \"normals\": " + normals_json : std::string()) + "}";
    }

    // host records, uploaded first
    template <typename T>
    void add_host(const char *name, const std::vector<T> &recs, size_t pos_offset, int64_t normal_offset = -1)
    {
        DeviceMaps up;
        char *d = (char *)up.bytes(recs.size() * sizeof(T), "--evaluate");
        if (!recs.empty() && hipMemcpy(d, recs.data(), recs.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("--evaluate: copy of a cloud failed");
        add(name, d + pos_offset, (int64_t)recs.size(), (int64_t)sizeof(T), normal_offset);
    }

    std::string report() const
    {
        return ", \"evaluate\": {" + entries + "}" + align_json;
    }
};

void render_device_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, const char *who,
                        const char *refined_name, DeviceMaps &m)
{
    auto device_bytes = [&m, who](size_t bytes) { return m.bytes(bytes, who); };
    check(ctx, hipSetDevice(args.device) == hipSuccess ? DP_OK : DP_E_HIP, "hipSetDevice");
    std::vector<int32_t> &vid = m.vid;
    std::vector<float *> &dd = m.depth, &dn = m.normal;
    vid.resize((size_t)V);
    dd.resize((size_t)V);
    dn.resize((size_t)V);
    for (int32_t v = 0; v < V; ++v) {
        int32_t w = 0, h = 0;
        check(ctx, dp_level_info(ctx, args.level, v, &w, &h, nullptr), "dp_level_info");
        vid[(size_t)v] = v;
        dd[(size_t)v] = (float *)device_bytes((size_t)w * h * 4);
        dn[(size_t)v] = (float *)device_bytes((size_t)w * h * 12);
    }
    dp_patch *d_pat = (dp_patch *)device_bytes(kept.size() * sizeof(dp_patch));
    if (!kept.empty() &&
        hipMemcpy(d_pat, kept.data(), kept.size() * sizeof(dp_patch), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error(std::string(who) + ": copy of the patches failed");
    const dp_render_options ro = render_options(args);
    dp_render_stats rs;
    check(ctx,
          dp_render_maps_device(ctx, kept.empty() ? nullptr : d_pat, (int64_t)kept.size(), nullptr, vid.data(), V, &ro,
                                dd.data(), nullptr, dn.data(), nullptr, &rs, nullptr),
          "dp_render_maps_device");
    m.cap = rs.covered_pixels;
    // --refine-maps N: N passes between the render and its user, into a
    // second set of planes and back; a pixel that is not kept holds no depth
    if (args.refine_passes > 0) {
        const dp_mapref_options mo = mapref_options(args);
        std::vector<float *> dd2((size_t)V), dn2((size_t)V);
        for (int32_t v = 0; v < V; ++v) {
            int32_t w = 0, h = 0;
            check(ctx, dp_level_info(ctx, args.level, v, &w, &h, nullptr), "dp_level_info");
            dd2[(size_t)v] = (float *)device_bytes((size_t)w * h * 4);
            dn2[(size_t)v] = (float *)device_bytes((size_t)w * h * 12);
        }
        dp_mapref_stats ms{};
        double refine_ms = 0.0;
        for (int pass = 0; pass < args.refine_passes; ++pass) {
            check(ctx,
                  dp_refine_maps_device(ctx, vid.data(), V, &mo, nullptr, dd.data(), dn.data(), dd2.data(), dn2.data(),
                                        nullptr, nullptr, &ms, nullptr),
                  "dp_refine_maps_device");
            refine_ms += ms.refine_ms;
            dd.swap(dd2);
            dn.swap(dn2);
        }
        m.cap = ms.kept;
        m.refined = refined_report(refined_name, args.refine_passes, ms, refine_ms);
    }
}

// --fuse: the device maps fused there (dp_fuse_maps_device); only the points
// come back.  An empty pixel is never emitted, so the pixels that hold a depth
// size the point buffer; should the fusion report more, it is reallocated once
// and re-run.  Returns the report's "fused" member.
std::string write_fused(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev)
{
    DeviceMaps m;
    render_device_maps(ctx, args, V, kept, "--fuse", "refined", m);
    const std::vector<int32_t> &vid = m.vid;
    const std::vector<float *> &dd = m.depth, &dn = m.normal;
    const std::string &refined = m.refined;
    int64_t cap = m.cap, n_fused = 0;
    dp_fuse_stats fs;
    dp_fused_point *d_pts = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        d_pts = (dp_fused_point *)m.bytes((size_t)cap * sizeof(dp_fused_point), "--fuse");
        check(ctx,
              dp_fuse_maps_device(ctx, vid.data(), V, &args.fuse, dd.data(), dn.data(), d_pts, cap, &n_fused, &fs,
                                  nullptr),
              "dp_fuse_maps_device");
        if (n_fused <= cap)
            break;
        cap = n_fused;
    }
    if (n_fused > cap)
        throw std::runtime_error("--fuse: the point count changed between two runs");
    // --fuse-clean-k: the outliers go before anything reads the cloud
    std::string cleaned;
    if (args.fuse_clean()) {
        const int64_t n_all = n_fused;
        uint8_t *d_keep = (uint8_t *)m.bytes((size_t)n_all, "--fuse-clean-k");
        dp_fused_point *d_kept = (dp_fused_point *)m.bytes((size_t)n_all * sizeof(dp_fused_point), "--fuse-clean-k");
        int64_t *d_n = (int64_t *)m.bytes(sizeof(int64_t), "--fuse-clean-k");
        dp_cloud_clean_options co{(float)args.fuse_clean_radius, args.fuse_clean_k, args.fuse_clean_min_neighbours,
                                  (float)args.fuse_clean_std,
                                  args.fuse_clean_radius_only ? DP_CLOUD_CLEAN_RADIUS_ONLY : 0};
        dp_cloud_clean_stats cs;
        check(ctx,
              dp_cloud_clean_device(ctx, d_pts, n_all, sizeof(dp_fused_point), &co, d_keep, nullptr, nullptr, d_kept, d_n,
                                    &cs, nullptr),
              "dp_cloud_clean_device");
        d_pts = d_kept;
        n_fused = cs.kept;
        char cbuf[320];
        std::snprintf(cbuf, sizeof cbuf,
                      ", \"fused_clean\": {\"points\": %lld, \"kept\": %lld, \"removed_sparse\": %lld, "
                      "\"removed_far\": %lld, \"mu\": %.9g, \"sigma\": %.9g, \"knn_ms\": %.3f, \"clean_ms\": %.3f}",
                      (long long)n_all, (long long)cs.kept, (long long)cs.removed_sparse, (long long)cs.removed_far,
                      cs.mu, cs.sigma, cs.knn_ms, cs.clean_ms);
        cleaned = cbuf;
    }
    std::vector<dp_fused_point> pts((size_t)n_fused);
    if (n_fused > 0 &&
        hipMemcpy(pts.data(), d_pts, pts.size() * sizeof(dp_fused_point), hipMemcpyDeviceToHost) != hipSuccess)
        throw std::runtime_error("--fuse: copy of the points failed");
    dpio::write_ply(args.fuse_path, to_cloud(pts), ev != nullptr, args.eval_normals);
    if (ev)
        ev->add("fused", (const char *)d_pts + offsetof(dp_fused_point, pos), n_fused, sizeof(dp_fused_point),
                offsetof(dp_fused_point, normal));
    char buf[240];
    std::snprintf(buf, sizeof buf,
                  ", \"fused\": {\"points\": %lld, \"fusable\": %lld, \"depth_pixels\": %lld, \"fuse_ms\": %.3f}",
                  (long long)n_fused, (long long)fs.fusable, (long long)fs.depth_pixels, fs.fuse_ms);
    return refined + buf + cleaned;
}

// --mesh: the device maps integrated into one TSDF volume around the written
// patches (dp_tsdf_integrate_device) and meshed there (dp_tsdf_mesh_device,
// once for the counts and once into buffers of that size) and, with one of the
// clean-up options, cleaned there (dp_mesh_clean_device); only the mesh comes
// back.  The volume is the patches' bounding box padded by the truncation;
// the voxel defaults to the box's longest side / --mesh-dim, the truncation to
// four voxels.  Returns the report's "mesh" member.
std::string write_mesh(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev)
{
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    for (const dp_patch &p : kept) {
        if (!(std::isfinite(p.pos[0]) && std::isfinite(p.pos[1]) && std::isfinite(p.pos[2])))
            continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = any ? std::min(lo[a], (double)p.pos[a]) : (double)p.pos[a];
            hi[a] = any ? std::max(hi[a], (double)p.pos[a]) : (double)p.pos[a];
        }
        any = true;
    }
    if (!any)
        throw std::runtime_error("--mesh: no patches to bound the volume");
    const double side = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    const double voxel = args.mesh_voxel > 0.0 ? args.mesh_voxel : side / args.mesh_dim;
    if (!(voxel > 0.0))
        throw std::runtime_error("--mesh: the patches have no extent (give --mesh-voxel)");
    const double trunc = args.mesh_trunc > 0.0 ? args.mesh_trunc : 4.0 * voxel;
    dp_tsdf_options to;
    dp_default_tsdf_options(&to);
    to.voxel = (float)voxel;
    to.trunc = (float)trunc;
    to.min_weight = args.mesh_min_weight;
    for (int a = 0; a < 3; ++a) {
        to.origin[a] = (float)(lo[a] - trunc);
        to.dim[a] = (int32_t)std::min(std::max(std::ceil((hi[a] - lo[a] + 2.0 * trunc) / voxel), 2.0), 1024.0);
    }
    DeviceMaps m;
    render_device_maps(ctx, args, V, kept, "--mesh", "mesh_refined", m);
    const size_t points = (size_t)to.dim[0] * to.dim[1] * to.dim[2];
    float *d_tsdf = (float *)m.bytes(points * 4, "--mesh");
    int32_t *d_weight = (int32_t *)m.bytes(points * 4, "--mesh");
    uint32_t *d_rgb = (uint32_t *)m.bytes(points * 4, "--mesh");
    dp_tsdf_stats ts;
    check(ctx,
          dp_tsdf_integrate_device(ctx, m.vid.data(), V, &to, m.depth.data(), d_tsdf, d_weight, d_rgb, &ts, nullptr),
          "dp_tsdf_integrate_device");
    int64_t nv = 0, nt = 0;
    dp_mesh_stats ms;
    check(ctx, dp_tsdf_mesh_device(ctx, &to, d_tsdf, d_weight, d_rgb, nullptr, 0, &nv, nullptr, 0, &nt, &ms, nullptr),
          "dp_tsdf_mesh_device");
    const int64_t vcap = nv, tcap = nt;
    dp_mesh_vertex *d_verts = (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), "--mesh");
    int32_t *d_tris = (int32_t *)m.bytes((size_t)tcap * 3 * sizeof(int32_t), "--mesh");
    check(ctx,
          dp_tsdf_mesh_device(ctx, &to, d_tsdf, d_weight, d_rgb, vcap ? d_verts : nullptr, vcap, &nv,
                              tcap ? d_tris : nullptr, tcap, &nt, &ms, nullptr),
          "dp_tsdf_mesh_device");
    if (nv != vcap || nt != tcap)
        throw std::runtime_error("--mesh: the counts changed between two runs");
    // --mesh-min-component / -frac / --mesh-keep-largest: the small components
    // dropped where the mesh lies (dp_mesh_clean_device; a clean mesh is no
    // larger than its input, so the input's counts size the buffers)
    std::string cleaned;
    if (args.mesh_clean()) {
        dp_mesh_clean_options mco;
        dp_default_mesh_clean_options(&mco);
        if (args.mesh_min_component >= 0)
            mco.min_triangles = args.mesh_min_component;
        if (args.mesh_min_component_frac >= 0.0)
            mco.min_fraction = (float)args.mesh_min_component_frac;
        if (args.mesh_keep_largest >= 0)
            mco.max_components = (int32_t)args.mesh_keep_largest;
        dp_mesh_vertex *d_cverts = (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), "--mesh");
        int32_t *d_ctris = (int32_t *)m.bytes((size_t)tcap * 3 * sizeof(int32_t), "--mesh");
        dp_mesh_clean_stats cs;
        check(ctx,
              dp_mesh_clean_device(ctx, &mco, vcap ? d_verts : nullptr, vcap, tcap ? d_tris : nullptr, tcap,
                                   vcap ? d_cverts : nullptr, vcap, &nv, tcap ? d_ctris : nullptr, tcap, &nt, nullptr,
                                   nullptr, &cs, nullptr),
              "dp_mesh_clean_device");
        if (nv > vcap || nt > tcap)
            throw std::runtime_error("--mesh: the clean-up returned more than it was given");
        d_verts = d_cverts;
        d_tris = d_ctris;
        char cbuf[480];
        std::snprintf(cbuf, sizeof cbuf,
                      ", \"clean\": {\"vertices_in\": %lld, \"triangles_in\": %lld, \"invalid_triangles\": %lld, "
                      "\"unused_vertices\": %lld, \"components\": %lld, \"largest_triangles\": %lld, "
                      "\"components_kept\": %lld, \"vertices_out\": %lld, \"triangles_out\": %lld, \"clean_ms\": %.3f}",
                      (long long)cs.vertices_in, (long long)cs.triangles_in, (long long)cs.invalid_triangles,
                      (long long)cs.unused_vertices, (long long)cs.components, (long long)cs.largest_triangles,
                      (long long)cs.components_kept, (long long)cs.vertices_out, (long long)cs.triangles_out,
                      cs.clean_ms);
        cleaned = cbuf;
    }
    // --mesh-smooth: the vertex positions relaxed where the mesh lies
    // (dp_mesh_smooth_device; the triangles stay); --mesh-normals: the normals
    // of the mesh as it will be written (dp_mesh_normals_device)
    if (args.mesh_smooth >= 0) {
        dp_mesh_smooth_options mso;
        dp_default_mesh_smooth_options(&mso);
        mso.iterations = args.mesh_smooth;
        if (args.mesh_smooth_lambda != 0.0)
            mso.lambda = (float)args.mesh_smooth_lambda;
        if (args.mesh_smooth_mu <= 0.0)
            mso.mu = (float)args.mesh_smooth_mu;
        if (args.mesh_smooth_free_boundary)
            mso.flags |= DP_SMOOTH_FREE_BOUNDARY;
        dp_mesh_vertex *d_sverts = (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), "--mesh");
        dp_mesh_smooth_stats ss;
        check(ctx,
              dp_mesh_smooth_device(ctx, &mso, nv ? d_verts : nullptr, nv, nt ? d_tris : nullptr, nt,
                                    nv ? d_sverts : nullptr, &ss, nullptr),
              "dp_mesh_smooth_device");
        d_verts = d_sverts;
        char sbuf[480];
        std::snprintf(sbuf, sizeof sbuf,
                      ", \"smooth\": {\"steps\": %lld, \"movable_vertices\": %lld, \"pinned_vertices\": %lld, "
                      "\"isolated_vertices\": %lld, \"edges\": %lld, \"boundary_edges\": %lld, "
                      "\"nonmanifold_edges\": %lld, \"max_valence\": %lld, \"adjacency_ms\": %.3f, \"smooth_ms\": %.3f}",
                      (long long)ss.steps, (long long)ss.movable_vertices, (long long)ss.pinned_vertices,
                      (long long)ss.isolated_vertices, (long long)ss.edges, (long long)ss.boundary_edges,
                      (long long)ss.nonmanifold_edges, (long long)ss.max_valence, ss.adjacency_ms, ss.smooth_ms);
        cleaned += sbuf;
    }
    // --mesh-decimate: the vertices of every cell of F voxels merged where the
    // mesh lies (dp_mesh_decimate_device; the result is no larger than its input)
    std::string decimated;
    const dp_mesh_vertex *d_before_verts = d_verts; // what --mesh-decimate was given (--eval-mesh-surface)
    const int32_t *d_before_tris = d_tris;
    const int64_t nv_before = nv, nt_before = nt;
    if (args.mesh_decimate > 0.0) {
        dp_mesh_decimate_options mdo;
        dp_default_mesh_decimate_options(&mdo);
        for (int a = 0; a < 3; ++a)
            mdo.origin[a] = to.origin[a];
        mdo.cell = (float)(args.mesh_decimate * (double)to.voxel);
        mdo.mode = args.mesh_decimate_quadric ? DP_DECIMATE_QUADRIC : DP_DECIMATE_MEAN;
        dp_mesh_vertex *d_dverts = (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), "--mesh");
        int32_t *d_dtris = (int32_t *)m.bytes((size_t)tcap * 3 * sizeof(int32_t), "--mesh");
        dp_mesh_decimate_stats ds;
        int64_t dv = 0, dt = 0;
        check(ctx,
              dp_mesh_decimate_device(ctx, &mdo, nv ? d_verts : nullptr, nv, nt ? d_tris : nullptr, nt,
                                      vcap ? d_dverts : nullptr, vcap, &dv, tcap ? d_dtris : nullptr, tcap, &dt, nullptr,
                                      nullptr, &ds, nullptr),
              "dp_mesh_decimate_device");
        if (dv > nv || dt > nt)
            throw std::runtime_error("--mesh: the simplification returned more than it was given");
        nv = dv;
        nt = dt;
        d_verts = d_dverts;
        d_tris = d_dtris;
        char dbuf[800];
        std::snprintf(dbuf, sizeof dbuf,
                      ", \"mesh_decimate\": {\"cell\": %.9g, \"quadric\": %s, \"vertices_in\": %lld, "
                      "\"triangles_in\": %lld, \"invalid_triangles\": %lld, \"degenerate_triangles\": %lld, "
                      "\"unused_vertices\": %lld, \"clamped_vertices\": %lld, \"clusters\": %lld, "
                      "\"orphan_clusters\": %lld, \"max_cluster\": %lld, \"collapsed_triangles\": %lld, "
                      "\"duplicate_triangles\": %lld, \"quadric_vertices\": %lld, \"mean_vertices\": %lld, "
                      "\"vertices_out\": %lld, \"triangles_out\": %lld, \"decimate_ms\": %.3f}",
                      (double)mdo.cell, args.mesh_decimate_quadric ? "true" : "false", (long long)ds.vertices_in,
                      (long long)ds.triangles_in, (long long)ds.invalid_triangles, (long long)ds.degenerate_triangles,
                      (long long)ds.unused_vertices, (long long)ds.clamped_vertices, (long long)ds.clusters,
                      (long long)ds.orphan_clusters, (long long)ds.max_cluster, (long long)ds.collapsed_triangles,
                      (long long)ds.duplicate_triangles, (long long)ds.quadric_vertices, (long long)ds.mean_vertices,
                      (long long)ds.vertices_out, (long long)ds.triangles_out, ds.decimate_ms);
        decimated = dbuf;
    }
    // (--mesh-colour weights the views by them, so it computes them too; they
    // are written only with --mesh-normals)
    std::vector<float> normals;
    float *d_normals = nullptr;
    if (args.mesh_normals || args.mesh_colour) {
        d_normals = (float *)m.bytes((size_t)vcap * 3 * sizeof(float), "--mesh");
        dp_mesh_normals_stats ns;
        check(ctx,
              dp_mesh_normals_device(ctx, nv ? d_verts : nullptr, nv, nt ? d_tris : nullptr, nt, nv ? d_normals : nullptr,
                                     &ns, nullptr),
              "dp_mesh_normals_device");
        normals.resize(args.mesh_normals ? (size_t)nv * 3 : 0);
        if (!normals.empty() && hipMemcpy(normals.data(), d_normals, normals.size() * sizeof(float), hipMemcpyDeviceToHost) !=
                          hipSuccess)
            throw std::runtime_error("--mesh: copy of the normals failed");
        char nbuf[160];
        std::snprintf(nbuf, sizeof nbuf, ", \"normals\": {\"zero_normals\": %lld, \"normals_ms\": %.3f}",
                      (long long)ns.zero_normals, ns.normals_ms);
        cleaned += nbuf;
    }
    // --mesh-depth-maps: the mesh as it will be written, still on the device,
    // rendered into every view (dp_mesh_render_device) and written as PFM files;
    // --mesh-colour reads the same depth planes, rendered once for both
    std::string rendered;
    std::vector<int32_t> rviews;
    std::vector<float *> rdepth;
    if (!args.mesh_depth_dir.empty() || args.mesh_colour) {
        if (!args.mesh_depth_dir.empty() && mkdir(args.mesh_depth_dir.c_str(), 0777) != 0 && errno != EEXIST)
            throw std::runtime_error("cannot create " + args.mesh_depth_dir);
        dp_mesh_render_options mro;
        dp_default_mesh_render_options(&mro);
        if (args.mesh_cull_back)
            mro.flags |= DP_MESH_RENDER_CULL_BACK;
        std::vector<int32_t> views((size_t)V), ws((size_t)V), hs((size_t)V);
        std::vector<float *> pd((size_t)V), pn((size_t)V, nullptr);
        for (int32_t v = 0; v < V; ++v) {
            views[(size_t)v] = v;
            check(ctx, dp_level_info(ctx, args.level, v, &ws[(size_t)v], &hs[(size_t)v], nullptr), "dp_level_info");
            const size_t px = (size_t)ws[(size_t)v] * (size_t)hs[(size_t)v];
            pd[(size_t)v] = (float *)m.bytes(px * sizeof(float), "--mesh-depth-maps");
            if (args.mesh_depth_normals)
                pn[(size_t)v] = (float *)m.bytes(px * 3 * sizeof(float), "--mesh-depth-maps");
        }
        dp_mesh_render_stats rs;
        check(ctx,
              dp_mesh_render_device(ctx, nv ? d_verts : nullptr, nv, nt ? d_tris : nullptr, nt, views.data(), V, &mro,
                                    pd.data(), nullptr, args.mesh_depth_normals ? pn.data() : nullptr, &rs, nullptr),
              "dp_mesh_render_device");
        rviews = views;
        rdepth = pd;
        std::vector<float> plane;
        for (int32_t v = 0; v < V && !args.mesh_depth_dir.empty(); ++v) {
            const int w = ws[(size_t)v], h = hs[(size_t)v];
            const float *src[2] = {pd[(size_t)v], pn[(size_t)v]};
            const char *fmt[2] = {"/mesh_depth_%04d.pfm", "/mesh_normal_%04d.pfm"};
            for (int j = 0; j < 2; ++j) {
                if (!src[j])
                    continue;
                const int ch = j ? 3 : 1;
                plane.resize((size_t)w * h * ch);
                if (!plane.empty() &&
                    hipMemcpy(plane.data(), src[j], plane.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                    throw std::runtime_error("--mesh-depth-maps: copy of a plane failed");
                char name[64];
                std::snprintf(name, sizeof name, fmt[j], (int)v);
                dpio::write_pfm(args.mesh_depth_dir + name, plane.data(), w, h, ch);
            }
        }
        char rbuf[480];
        std::snprintf(rbuf, sizeof rbuf,
                      ", \"mesh_render\": {\"views\": %d, \"cull_back\": %s, \"triangles\": %lld, "
                      "\"invalid_triangles\": %lld, \"pairs\": %lld, \"clipped_pairs\": %lld, \"culled_pairs\": %lld, "
                      "\"pixel_tests\": %lld, \"covered_pixels\": %lld, \"render_ms\": %.3f}",
                      (int)V, args.mesh_cull_back ? "true" : "false", (long long)rs.triangles,
                      (long long)rs.invalid_triangles, (long long)rs.pairs, (long long)rs.clipped_pairs,
                      (long long)rs.culled_pairs, (long long)rs.pixel_tests, (long long)rs.covered_pixels, rs.render_ms);
        rendered = rbuf;
    }
    // --mesh-colour: the vertices of the mesh as it will be written coloured by
    // the views that see them (dp_mesh_colour_device), the last stage
    if (args.mesh_colour) {
        dp_mesh_colour_options mco;
        dp_default_mesh_colour_options(&mco);
        if (args.mesh_colour_tol >= 0.0)
            mco.depth_tol = (float)args.mesh_colour_tol;
        if (args.mesh_colour_min_cos >= 0.0)
            mco.min_cos = (float)args.mesh_colour_min_cos;
        if (args.mesh_colour_bilinear)
            mco.flags |= DP_MESH_COLOUR_BILINEAR;
        dp_mesh_vertex *d_cverts = (dp_mesh_vertex *)m.bytes((size_t)vcap * sizeof(dp_mesh_vertex), "--mesh-colour");
        dp_mesh_colour_stats cs;
        check(ctx,
              dp_mesh_colour_device(ctx, nv ? d_verts : nullptr, nv, nv ? d_normals : nullptr, rviews.data(), V, &mco,
                                    rdepth.data(), nv ? d_cverts : nullptr, nullptr, nullptr, &cs, nullptr),
              "dp_mesh_colour_device");
        d_verts = d_cverts;
        char cbuf[640];
        std::snprintf(cbuf, sizeof cbuf,
                      ", \"mesh_colour\": {\"views\": %d, \"bilinear\": %s, \"depth_tol\": %.9g, \"min_cos\": %.9g, "
                      "\"vertices\": %lld, \"projected_pairs\": %lld, \"occluded_pairs\": %lld, "
                      "\"grazing_pairs\": %lld, \"visible_pairs\": %lld, \"coloured_vertices\": %lld, "
                      "\"unseen_vertices\": %lld, \"colour_ms\": %.3f}",
                      (int)V, args.mesh_colour_bilinear ? "true" : "false", (double)mco.depth_tol, (double)mco.min_cos,
                      (long long)cs.vertices, (long long)cs.projected_pairs, (long long)cs.occluded_pairs,
                      (long long)cs.grazing_pairs, (long long)cs.visible_pairs, (long long)cs.coloured_vertices,
                      (long long)cs.unseen_vertices, cs.colour_ms);
        rendered += cbuf;
    }
    std::vector<dp_mesh_vertex> verts((size_t)nv);
    std::vector<int32_t> tris((size_t)nt * 3);
    if ((nv > 0 && hipMemcpy(verts.data(), d_verts, verts.size() * sizeof(dp_mesh_vertex), hipMemcpyDeviceToHost) !=
                       hipSuccess) ||
        (nt > 0 && hipMemcpy(tris.data(), d_tris, tris.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
        throw std::runtime_error("--mesh: copy of the mesh failed");
    std::vector<dpio::MeshPoint> out(verts.size());
    for (size_t i = 0; i < verts.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            out[i].pos[k] = verts[i].pos[k];
            out[i].rgb[k] = verts[i].rgb[k];
        }
    dpio::write_mesh_ply(args.mesh_path, out, tris, args.mesh_normals ? &normals : nullptr);
    if (ev)
        ev->add("mesh_vertices", d_verts, nv, sizeof(dp_mesh_vertex));
    if (ev && args.eval_mesh_surface) {
        ev->add_mesh_surface(d_verts, nv, d_tris, nt);
        if (args.mesh_decimate > 0.0)
            ev->add_deviation("decimate_deviation", d_before_verts, nv_before, d_before_tris, nt_before, d_verts, nv,
                              d_tris, nt);
    }
    char buf[400];
    std::snprintf(buf, sizeof buf,
                  ", \"mesh\": {\"vertices\": %lld, \"triangles\": %lld, \"ms\": %.3f, \"dim\": [%d, %d, %d], "
                  "\"voxel\": %.9g, \"trunc\": %.9g, \"observed_voxels\": %lld, \"active_cells\": %lld, "
                  "\"integrate_ms\": %.3f, \"mesh_ms\": %.3f",
                  (long long)nv, (long long)nt, ts.integrate_ms + ms.mesh_ms, to.dim[0], to.dim[1], to.dim[2],
                  (double)to.voxel, (double)to.trunc, (long long)ts.observed_voxels, (long long)ms.active_cells,
                  ts.integrate_ms, ms.mesh_ms);
    return m.refined + buf + cleaned + "}" + decimated + rendered;
}

using Clock = std::chrono::steady_clock;

// The JSON line.  `extra`: the members the optional stages add.
void print_report(const Args &args, DensifyResult &res, size_t written, size_t n_seeds, const dp_seed_stats &sst,
                  Clock::time_point t0, const std::string &extra)
{
    dp_densify_stats &st = res.stats;
    std::vector<dp_iterate_stats> &iters = res.rounds;
    // the per-round counts (one round: the densify and the optional filter)
    if (iters.empty()) {
        dp_iterate_stats one{};
        one.offered = st.seeds_in;
        one.reinserted = st.seed_patches;
        one.patches = st.patches;
        one.candidates = st.candidates;
        one.evals = st.evals;
        one.generations = st.generations;
        iters.push_back(one);
    }
    if (!res.filtered) {
        iters.back().filtered_out = res.n - (int64_t)written;
        if (args.iterations > 1)
            st.patches = (int64_t)written; // as dp_densify_iterate reports: the survivors
    }
    std::string iters_json = "[";
    for (size_t k = 0; k < iters.size(); ++k) {
        char buf[320];
        std::snprintf(buf, sizeof buf,
                      "%s{\"offered\": %lld, \"reinserted\": %lld, \"patches\": %lld, \"filtered_out\": %lld, "
                      "\"candidates\": %lld, \"evals\": %lld, \"generations\": %d}",
                      k ? ", " : "", (long long)iters[k].offered, (long long)iters[k].reinserted,
                      (long long)iters[k].patches, (long long)iters[k].filtered_out, (long long)iters[k].candidates,
                      (long long)iters[k].evals, iters[k].generations);
        iters_json += buf;
    }
    iters_json += "]";
    const double wall = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    std::printf("{\"output\": \"%s\", \"patches\": %lld, \"written\": %zu, \"seeds\": %zu, \"generated_seeds\": %s, "
                "\"keypoints\": %lld, \"matches\": %lld, \"seed_ms\": %.3f, \"seed_patches\": %lld, "
                "\"pops\": %lld, \"candidates\": %lld, \"evals\": %lld, \"generations\": %d, \"refine_ms\": %.3f, "
                "\"densify_ms\": %.3f, \"wall_ms\": %.3f, \"gpus\": %d, \"mode\": \"%s\", \"exchanged\": %lld, "
                "\"iterations\": %s%s}\n",
                args.output.c_str(), (long long)st.patches, written, n_seeds,
                args.seeds_path.empty() ? "true" : "false", (long long)sst.keypoints, (long long)sst.matches,
                sst.total_ms, (long long)st.seed_patches, (long long)st.pops, (long long)st.candidates,
                (long long)st.evals, st.generations, st.refine_ms, st.total_ms, wall, args.gpus,
                args.fast.densify ? "fast" : "parity", (long long)res.exchanged, iters_json.c_str(), extra.c_str());
}

} // namespace

int main(int argc, char **argv)
{
    Args args;
    std::string error;
    switch (parse_args(argc, argv, args, error)) {
    case Parse::Run:
        break;
    case Parse::Help:
        usage();
        return 0;
    case Parse::UsageError:
        if (error.empty())
            usage();
        else
            std::fprintf(stderr, "densify: %s\n", error.c_str());
        return 2;
    }
    try {
        if (!args.synth.empty()) {
            if (args.scene_dir.empty())
                throw std::runtime_error("--synthetic needs --write-scene DIR");
            return write_synthetic(args.synth, args.scene_dir);
        }
        const Clock::time_point t0 = Clock::now();
        SceneData sc = load_scene(args);
        if (args.check_only) {
            print_check_only(sc);
            return 0;
        }
        const int32_t V = (int32_t)sc.imgs.size();
        CtxPtr ctx = make_context(sc, args.device, args.fast, args.level, 0);
        const dp_seed_stats sst = generate_or_read_seeds(ctx.get(), args, sc);
        DensifyResult res = run_densify(ctx.get(), args, sc);
        const std::vector<dp_patch> kept = filter_survivors(ctx.get(), args, res);
        // with --evaluate the clouds' PLYs carry every digit of their positions
        // (with --eval-normals of their normals too): the report describes the
        // files as written
        std::unique_ptr<Evaluation> ev;
        if (!args.eval_path.empty())
            ev.reset(new Evaluation(ctx.get(), args, sc.truth));
        dpio::write_ply(args.output, to_cloud(kept), ev != nullptr, args.eval_normals);
        std::string extra;
        if (!args.depth_dir.empty())
            extra += write_depth_maps(ctx.get(), args, V, kept);
        if (ev)
            ev->add_host("patches", kept, offsetof(dp_patch, pos), offsetof(dp_patch, normal));
        if (!args.fuse_path.empty())
            extra += write_fused(ctx.get(), args, V, kept, ev.get());
        if (!args.mesh_path.empty())
            extra += write_mesh(ctx.get(), args, V, kept, ev.get());
        if (ev) {
            extra += ev->report();
            ev.reset(); // its device memory goes before the context
        }
        ctx.reset(); // wall_ms includes the context's teardown
        print_report(args, res, kept.size(), sc.seeds.size() / 3, sst, t0, extra);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "densify: %s\n", e.what());
        return 1;
    }
}
