// device_maps.h -- what the densify CLI's device stages share: the check of a
// library call, device memory that frees itself, copies that throw, the
// per-view planes of a level, and the first stage of --fuse and --mesh alike
// (render_device_maps).
#pragma once

#include "cli_args.h"
#include "cli_error.h"
#include "dp_buf.h"
#include "report_json.h"

#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

// a library call on the first context
inline void check(dp_ctx *ctx, int rc, const char *what)
{
    if (rc != DP_OK)
        throw CliError(what, rc, dp_last_error(ctx));
}

// DeviceMaps owns the planes of render_device_maps (and whatever else its user
// allocates through bytes()); `cap` bounds the pixels that hold a depth.
struct DeviceMaps {
    std::vector<dpk::DevMem> mem;
    std::vector<int32_t> vid;
    std::vector<float *> depth, normal;
    int64_t cap = 0;
    JsonObject refined; // the report's member of --refine-maps, empty without it

    void *bytes(size_t n, const char *who)
    {
        mem.emplace_back();
        if (mem.back().alloc(n ? n : 1) != hipSuccess)
            throw std::runtime_error(std::string(who) + ": out of device memory");
        return mem.back().p;
    }
};

// host to device and back, the whole vector; a failed copy throws `message`
template <typename T> void upload(void *dst, const std::vector<T> &src, const std::string &message)
{
    if (!src.empty() && hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error(message);
}
template <typename T> void download(std::vector<T> &dst, const void *src, const std::string &message)
{
    if (!dst.empty() && hipMemcpy(dst.data(), src, dst.size() * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)
        throw std::runtime_error(message);
}

// One float plane per view of the level for the depths and, with normals, one
// of three floats a pixel, allocated from `m` (dp_level_info gives the sizes).
struct Planes {
    std::vector<int32_t> w, h;
    std::vector<float *> depth, normal; // normal[v] is null without normals
};
Planes device_planes(dp_ctx *ctx, int level, int32_t V, bool normals, DeviceMaps &m, const char *who);

dp_render_options render_options(const Args &args);
dp_mapref_options mapref_options(const Args &args);

// the report's member of the last --refine-maps pass
JsonObject refined_report(int passes, const dp_mapref_stats &ms, double total_ms);

// "<dir>/<stem>_<view, four digits>.pfm"
std::string view_pfm(const std::string &dir, const char *stem, int32_t view);

// Depth and normal maps of every view rendered into device planes of `m`
// (dp_render_maps_device, honouring --splat-scale) and, with --refine-maps N,
// refined there.
void render_device_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, const char *who,
                        DeviceMaps &m);
