// stages.h -- the optional stages of the densify CLI that follow the densify
// itself: --depth-maps (map_stages.cpp), --fuse (map_stages.cpp) and --mesh
// (mesh_stages.cpp).  Each writes its files and adds its members to the report.
#pragma once

#include "device_maps.h"
#include "evaluate.h"
#include "scene_io.h"

#include <vector>

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

// --depth-maps: the written patches as per-view depth (and normal) maps of
// the level the densify ran on (dp_render_maps), with --refine-maps N refined;
// with --gpus N this context (rank 0) renders, the store being replicated.
// Adds "depth_maps" and, refined, "refined_maps".
void write_depth_maps(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, JsonObject &report);

// --fuse: the device maps fused there (dp_fuse_maps_device) and, with
// --fuse-clean-k, cleaned there; only the points come back.  Adds "refined"
// (with --refine-maps), "fused" and "fused_clean".
void write_fused(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev,
                 JsonObject &report);

// --mesh: the device maps integrated into one TSDF volume around the written
// patches and meshed there, the mesh cleaned, smoothed, simplified, rendered
// and coloured there as the options ask; only the mesh comes back.  Adds
// "mesh_refined" (with --refine-maps), "mesh", "mesh_decimate", "mesh_render"
// and "mesh_colour".
void write_mesh(dp_ctx *ctx, const Args &args, int32_t V, const std::vector<dp_patch> &kept, Evaluation *ev,
                JsonObject &report);
