// densify -- command-line front end of the MI355X patch loop.
//
// Mirrors the reference's programs/densify/main.cpp (-i scene.json, -s
// settings.json; PMVS::AddCamera per view, then PMVS::Run) and adds what
// SURVEY 8b asks of the build: -o out.ply (PMVS::PrintCloud format), --seeds
// (seed points from a file instead of Matcher::GenerateSeeds), --device,
// option overrides.  All compute goes through the C ABI of libdensepoints.so
// (include/densepoints.h): dp_set_views, dp_generate_seeds, dp_densify.
// The options: usage() in cli_args.cpp.  main() runs the stages in order: here
// are the settings, the scene, the context, the seeds, the densify, the filter
// and the report; the optional stages behind them are those of stages.h, the
// evaluation is evaluate.h, and report_json.h writes the report's text.
#include "multi_gpu.h"
#include "stages.h"

#include <chrono>
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
    JsonObject report;
    report.string("scene", dir + "/scene.json").integer("views", cfg.n_views).integer("seeds", n);
    std::printf("%s\n", report.str().c_str());
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
    std::vector<std::string> fnv;
    for (const dpio::Image &img : imgs) {
        uint64_t h = 1469598103934665603ull;
        for (uint8_t b : img.bgr)
            h = (h ^ b) * 1099511628211ull;
        std::string hex(16, '0'); // sixteen lower-case hex digits
        for (int i = 15; i >= 0; --i, h >>= 4)
            hex[(size_t)i] = "0123456789abcdef"[h & 15];
        fnv.push_back("\"" + hex + "\"");
    }
    JsonObject report;
    report.integer("views", imgs.size()).integer("width", imgs.empty() ? 0 : imgs[0].width);
    report.integer("height", imgs.empty() ? 0 : imgs[0].height).integer("seeds", sc.seeds.size() / 3);
    report.raw("image_fnv", json_array(fnv));
    if (!sc.truth.empty()) // --evaluate
        report.integer("truth", sc.truth.size() / 3);
    std::printf("%s\n", report.str().c_str());
}

struct CtxDestroy {
    void operator()(dp_ctx *c) const { dp_ctx_destroy(c); }
};
using CtxPtr = std::unique_ptr<dp_ctx, CtxDestroy>;

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

using Clock = std::chrono::steady_clock;

// The JSON line.  `extra`: the members the optional stages add.
void print_report(const Args &args, DensifyResult &res, size_t written, size_t n_seeds, const dp_seed_stats &sst,
                  Clock::time_point t0, const JsonObject &extra)
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
    std::vector<std::string> rounds;
    for (const dp_iterate_stats &it : iters) {
        JsonObject o;
        o.integer("offered", it.offered).integer("reinserted", it.reinserted).integer("patches", it.patches);
        o.integer("filtered_out", it.filtered_out).integer("candidates", it.candidates).integer("evals", it.evals);
        rounds.push_back(o.integer("generations", it.generations).str());
    }
    const double wall = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    JsonObject o;
    o.string("output", args.output).integer("patches", st.patches).integer("written", written);
    o.integer("seeds", n_seeds).boolean("generated_seeds", args.seeds_path.empty());
    o.integer("keypoints", sst.keypoints).integer("matches", sst.matches).ms("seed_ms", sst.total_ms);
    o.integer("seed_patches", st.seed_patches).integer("pops", st.pops).integer("candidates", st.candidates);
    o.integer("evals", st.evals).integer("generations", st.generations).ms("refine_ms", st.refine_ms);
    o.ms("densify_ms", st.total_ms).ms("wall_ms", wall).integer("gpus", args.gpus);
    o.string("mode", args.fast.densify ? "fast" : "parity").integer("exchanged", res.exchanged);
    o.raw("iterations", json_array(rounds)).members(extra);
    std::printf("%s\n", o.str().c_str());
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
        JsonObject extra;
        if (!args.depth_dir.empty())
            write_depth_maps(ctx.get(), args, V, kept, extra);
        if (ev)
            ev->add_host("patches", kept, offsetof(dp_patch, pos), offsetof(dp_patch, normal));
        if (!args.fuse_path.empty())
            write_fused(ctx.get(), args, V, kept, ev.get(), extra);
        if (!args.mesh_path.empty())
            write_mesh(ctx.get(), args, V, kept, ev.get(), extra);
        if (ev) {
            ev->report(extra);
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
