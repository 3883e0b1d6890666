// map_stages.cpp -- the --depth-maps and --fuse stages of the densify CLI (stages.h).
#include "stages.h"

#include <cerrno>
#include <cstddef>
#include <sys/stat.h>

namespace {

JsonObject depth_maps_report(int32_t V, int64_t covered_pixels, double render_ms)
{
    JsonObject o;
    return o.integer("views", V).integer("covered_pixels", covered_pixels).ms("render_ms", render_ms);
}

// one zeroed host plane of `channels` floats a pixel per view, and the planes' addresses
struct HostPlanes {
    std::vector<std::vector<float>> store;
    std::vector<float *> p;
    HostPlanes(const std::vector<int32_t> &w, const std::vector<int32_t> &h, int channels)
    {
        for (size_t v = 0; v < w.size(); ++v) {
            store.emplace_back((size_t)w[v] * h[v] * channels, 0.0f);
            p.push_back(store.back().data());
        }
    }
};

// --depth-maps with --refine-maps N: the refinement reads every view's planes,
// so all views are rendered first (with normals, which it needs), refined N
// times on the host form, then written: depth, score, and normal when asked.
void write_refined_depth_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept,
                              JsonObject &report)
{
    const dp_render_options ro = render_options(args);
    const dp_mapref_options mo = mapref_options(args);
    std::vector<int32_t> vid((size_t)V), ws((size_t)V), hs((size_t)V);
    for (int32_t v = 0; v < V; ++v) {
        check(ctx, dp_level_info(ctx, args.level, v, &ws[(size_t)v], &hs[(size_t)v], nullptr), "dp_level_info");
        vid[(size_t)v] = v;
    }
    HostPlanes depth[2] = {{ws, hs, 1}, {ws, hs, 1}}, normal[2] = {{ws, hs, 3}, {ws, hs, 3}}, score(ws, hs, 1);
    dp_render_stats rs;
    check(ctx,
          dp_render_maps(ctx, kept.data(), (int64_t)kept.size(), nullptr, vid.data(), V, &ro, depth[0].p.data(),
                         nullptr, normal[0].p.data(), nullptr, &rs),
          "dp_render_maps");
    dp_mapref_stats ms{};
    double refine_ms = 0.0;
    int cur = 0;
    for (int pass = 0; pass < args.refine_passes; ++pass, cur ^= 1) {
        check(ctx,
              dp_refine_maps(ctx, vid.data(), V, &mo, nullptr, depth[cur].p.data(), normal[cur].p.data(),
                             depth[cur ^ 1].p.data(), normal[cur ^ 1].p.data(), score.p.data(), nullptr, &ms),
              "dp_refine_maps");
        refine_ms += ms.refine_ms;
    }
    for (int32_t v = 0; v < V; ++v) {
        const int w = ws[(size_t)v], h = hs[(size_t)v];
        dpio::write_pfm(view_pfm(args.depth_dir, "depth", v), depth[cur].p[(size_t)v], w, h, 1);
        dpio::write_pfm(view_pfm(args.depth_dir, "score", v), score.p[(size_t)v], w, h, 1);
        if (args.depth_normals)
            dpio::write_pfm(view_pfm(args.depth_dir, "normal", v), normal[cur].p[(size_t)v], w, h, 3);
    }
    report.object("depth_maps", depth_maps_report(V, rs.covered_pixels, rs.render_ms))
        .object("refined_maps", refined_report(args.refine_passes, ms, refine_ms));
}

struct FusedCloud {
    dp_fused_point *d_pts = nullptr;
    int64_t n = 0;
};

// An empty pixel is never emitted, so the pixels that hold a depth size the
// point buffer; should the fusion report more, it is reallocated once and re-run.
dp_fuse_stats fuse(dp_ctx *ctx, const Args &args, int32_t V, DeviceMaps &m, FusedCloud &cloud)
{
    dp_fuse_stats fs;
    int64_t cap = m.cap;
    for (int attempt = 0; attempt < 2; ++attempt) {
        cloud.d_pts = (dp_fused_point *)m.bytes((size_t)cap * sizeof(dp_fused_point), "--fuse");
        check(ctx,
              dp_fuse_maps_device(ctx, m.vid.data(), V, &args.fuse, m.depth.data(), m.normal.data(), cloud.d_pts, cap,
                                  &cloud.n, &fs, nullptr),
              "dp_fuse_maps_device");
        if (cloud.n <= cap)
            break;
        cap = cloud.n;
    }
    if (cloud.n > cap)
        throw std::runtime_error("--fuse: the point count changed between two runs");
    return fs;
}

dp_cloud_clean_options clean_options(const Args &args)
{
    return dp_cloud_clean_options{(float)args.fuse_clean_radius, args.fuse_clean_k, args.fuse_clean_min_neighbours,
                                  (float)args.fuse_clean_std,
                                  args.fuse_clean_radius_only ? DP_CLOUD_CLEAN_RADIUS_ONLY : 0};
}

// --fuse-clean-k: the outliers go before anything reads the cloud
JsonObject clean(dp_ctx *ctx, const Args &args, DeviceMaps &m, FusedCloud &cloud)
{
    const int64_t n_all = cloud.n;
    uint8_t *d_keep = (uint8_t *)m.bytes((size_t)n_all, "--fuse-clean-k");
    dp_fused_point *d_kept = (dp_fused_point *)m.bytes((size_t)n_all * sizeof(dp_fused_point), "--fuse-clean-k");
    int64_t *d_n = (int64_t *)m.bytes(sizeof(int64_t), "--fuse-clean-k");
    const dp_cloud_clean_options co = clean_options(args);
    dp_cloud_clean_stats cs;
    check(ctx,
          dp_cloud_clean_device(ctx, cloud.d_pts, n_all, sizeof(dp_fused_point), &co, d_keep, nullptr, nullptr, d_kept,
                                d_n, &cs, nullptr),
          "dp_cloud_clean_device");
    cloud.d_pts = d_kept;
    cloud.n = cs.kept;
    JsonObject o;
    o.integer("points", n_all).integer("kept", cs.kept).integer("removed_sparse", cs.removed_sparse);
    o.integer("removed_far", cs.removed_far).g9("mu", cs.mu).g9("sigma", cs.sigma);
    return o.ms("knn_ms", cs.knn_ms).ms("clean_ms", cs.clean_ms);
}

void write_and_evaluate(const Args &args, const FusedCloud &cloud, Evaluation *ev)
{
    std::vector<dp_fused_point> pts((size_t)cloud.n);
    download(pts, cloud.d_pts, "--fuse: copy of the points failed");
    dpio::write_ply(args.fuse_path, to_cloud(pts), ev != nullptr, args.eval_normals);
    if (ev)
        ev->add("fused", (const char *)cloud.d_pts + offsetof(dp_fused_point, pos), cloud.n, sizeof(dp_fused_point),
                offsetof(dp_fused_point, normal));
}

} // namespace

void write_depth_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, JsonObject &report)
{
    if (mkdir(args.depth_dir.c_str(), 0777) != 0 && errno != EEXIST)
        throw std::runtime_error("cannot create " + args.depth_dir);
    if (args.refine_passes > 0)
        return write_refined_depth_maps(ctx, args, V, kept, report);
    // one view at a time
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
        dpio::write_pfm(view_pfm(args.depth_dir, "depth", v), pd, w, h, 1);
        if (args.depth_normals)
            dpio::write_pfm(view_pfm(args.depth_dir, "normal", v), pn, w, h, 3);
    }
    report.object("depth_maps", depth_maps_report(V, covered, render_ms));
}

void write_fused(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev,
                 JsonObject &report)
{
    DeviceMaps m;
    render_device_maps(ctx, args, V, kept, "--fuse", m);
    FusedCloud cloud;
    const dp_fuse_stats fs = fuse(ctx, args, V, m, cloud);
    JsonObject cleaned;
    if (args.fuse_clean())
        cleaned = clean(ctx, args, m, cloud);
    write_and_evaluate(args, cloud, ev);
    if (!m.refined.empty())
        report.object("refined", m.refined);
    JsonObject fused;
    fused.integer("points", cloud.n).integer("fusable", fs.fusable).integer("depth_pixels", fs.depth_pixels);
    report.object("fused", fused.ms("fuse_ms", fs.fuse_ms));
    if (args.fuse_clean())
        report.object("fused_clean", cleaned);
}
