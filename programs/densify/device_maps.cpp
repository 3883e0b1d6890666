// device_maps.cpp -- see device_maps.h.
#include "device_maps.h"

Planes device_planes(dp_ctx *ctx, int level, int32_t V, bool normals, DeviceMaps &m, const char *who)
{
    Planes p;
    p.w.resize((size_t)V);
    p.h.resize((size_t)V);
    p.depth.resize((size_t)V);
    p.normal.assign((size_t)V, nullptr);
    for (int32_t v = 0; v < V; ++v) {
        check(ctx, dp_level_info(ctx, level, v, &p.w[(size_t)v], &p.h[(size_t)v], nullptr), "dp_level_info");
        const size_t px = (size_t)p.w[(size_t)v] * (size_t)p.h[(size_t)v];
        p.depth[(size_t)v] = (float *)m.bytes(px * sizeof(float), who);
        if (normals)
            p.normal[(size_t)v] = (float *)m.bytes(px * 3 * sizeof(float), who);
    }
    return p;
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

JsonObject refined_report(int passes, const dp_mapref_stats &ms, double total_ms)
{
    JsonObject o;
    o.integer("passes", passes).integer("kept", ms.kept).integer("filled", ms.filled).integer("moved", ms.moved);
    return o.integer("candidates", ms.candidates).ms("refine_ms", total_ms);
}

std::string view_pfm(const std::string &dir, const char *stem, int32_t view)
{
    const std::string n = std::to_string(view);
    return dir + "/" + stem + "_" + std::string(n.size() < 4 ? 4 - n.size() : 0, '0') + n + ".pfm";
}

void render_device_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, const char *who,
                        DeviceMaps &m)
{
    check(ctx, hipSetDevice(args.device) == hipSuccess ? DP_OK : DP_E_HIP, "hipSetDevice");
    Planes maps = device_planes(ctx, args.level, V, true, m, who);
    m.vid.resize((size_t)V);
    for (int32_t v = 0; v < V; ++v)
        m.vid[(size_t)v] = v;
    m.depth = maps.depth;
    m.normal = maps.normal;
    dp_patch *d_pat = (dp_patch *)m.bytes(kept.size() * sizeof(dp_patch), who);
    upload(d_pat, kept, std::string(who) + ": copy of the patches failed");
    const dp_render_options ro = render_options(args);
    dp_render_stats rs;
    check(ctx,
          dp_render_maps_device(ctx, kept.empty() ? nullptr : d_pat, (int64_t)kept.size(), nullptr, m.vid.data(), V,
                                &ro, m.depth.data(), nullptr, m.normal.data(), nullptr, &rs, nullptr),
          "dp_render_maps_device");
    m.cap = rs.covered_pixels;
    if (args.refine_passes == 0)
        return;
    // --refine-maps N: N passes between the render and its user, into a
    // second set of planes and back; a pixel that is not kept holds no depth
    const dp_mapref_options mo = mapref_options(args);
    Planes other = device_planes(ctx, args.level, V, true, m, who);
    dp_mapref_stats ms{};
    double refine_ms = 0.0;
    for (int pass = 0; pass < args.refine_passes; ++pass) {
        check(ctx,
              dp_refine_maps_device(ctx, m.vid.data(), V, &mo, nullptr, m.depth.data(), m.normal.data(),
                                    other.depth.data(), other.normal.data(), nullptr, nullptr, &ms, nullptr),
              "dp_refine_maps_device");
        refine_ms += ms.refine_ms;
        m.depth.swap(other.depth);
        m.normal.swap(other.normal);
    }
    m.cap = ms.kept;
    m.refined = refined_report(args.refine_passes, ms, refine_ms);
}
