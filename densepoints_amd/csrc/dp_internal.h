// dp_internal.h -- shared between the C-ABI host code and the gfx950 kernels.
#pragma once

#include "../../include/densepoints.h"
#include "dp_geom.h"
#include "dp_devmath.h"
#include <hip/hip_runtime.h>

namespace dpk {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;

struct GenDev;

// ---- the organizer's per-record work, shared by the organizer kernels
// (dp_bfs.hip) and the refine kernels' densify epilogue ------------------------

// PatchGrid cell of a record centre in one view (patch_organizer.cpp:42-65):
// false when it projects outside the view's grid
__device__ __forceinline__ bool org_cell(const dpg::ViewDev &v, const float *pos, double gs, int64_t &cell)
{
    double u, w;
    dpg::project(v.P, pos[0], pos[1], pos[2], u, w);
    const int64_t row = dpg::grid_coord(w, gs), col = dpg::grid_coord(u, gs);
    if (col < 0 || col >= v.gw || row < 0 || row >= v.gh)
        return false;
    cell = v.grid_off + row * (int64_t)v.gw + col;
    return true;
}

// Patch::ComputeColor (patch.cpp:51-73) by one wave: lane l projects the centre
// into views l, l + 64; the BGR sums are exact integers in any order, so the
// wave sum is the reference's fp64 sum.  Returns R | G << 8 | B << 16 (the
// record's rgb bytes) in every lane.
__device__ __forceinline__ uint32_t wave_color(const dpg::ViewDev *views, int V, const float *pos, int lane)
{
    const float p0 = pos[0], p1 = pos[1], p2 = pos[2];
    uint32_t s0 = 0, s1 = 0, s2 = 0, nin = 0;
    for (int v = lane; v < V; v += 64) {
        const dpg::ViewDev &vw = views[v];
        double u, w;
        dpg::project(vw.P, p0, p1, p2, u, w);
        if (dpg::inside(u, w, vw.W, vw.H)) {
            const uint32_t px = vw.img[(size_t)(int)w * (size_t)vw.pitch + (size_t)(int)u];
            s0 += px & 255u;
            s1 += (px >> 8) & 255u;
            s2 += (px >> 16) & 255u;
            ++nin;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        nin += __shfl_xor(nin, o);
    }
    if (!nin)
        return 0u;
    const uint32_t c0 = (uint8_t)((double)s2 / (double)nin), c1 = (uint8_t)((double)s1 / (double)nin),
                   c2 = (uint8_t)((double)s0 / (double)nin);
    return c0 | c1 << 8 | c2 << 16;
}

// capacity-1 claims of one record by one wave (PatchGrid::TryInsert's first
// come, first served as atomicMin(seq)): lane l claims its cell in views l and
// 64 + l when they are visible
__device__ __forceinline__ void wave_claims(const dpg::ViewDev *views, const float *pos, uint64_t vis0, uint64_t vis1,
                                            double gs, uint32_t *grid, uint32_t seq, int lane)
{
    int64_t cell;
    if (((vis0 >> lane) & 1ull) && org_cell(views[lane], pos, gs, cell))
        atomicMin(&grid[cell], seq);
    if (((vis1 >> lane) & 1ull) && org_cell(views[64 + lane], pos, gs, cell))
        atomicMin(&grid[cell], seq);
}

// densify epilogue of a refine launch (RefineArgs::epi, FastArgs::epi): the
// organizer work a refined candidate that passed the filter can do at once,
// by the wave that refined it
constexpr int kEpiColor = 1;  // Patch::ComputeColor into the record's rgb
constexpr int kEpiClaims = 2; // capacity-1 claims at seq0 + index (the organizer skips its claims pass)

// The epilogue as a call, not inlined: its fp64 projections would otherwise
// join the refine kernels' register allocation (the parity kernel's spills
// grew 4 -> 20 VGPRs inlined); as a call only the values live across it are
// saved, once per candidate.  Returns the colour (wave_color) or 0.
[[maybe_unused]] static __device__ __noinline__ uint32_t refine_epilogue(const dpg::ViewDev *views, int V, float p0,
                                                                        float p1, float p2, uint64_t vis0,
                                                                        uint64_t vis1, int epi, double gs,
                                                                        uint32_t *grid, uint32_t seq, int lane)
{
    const float pf[3] = {p0, p1, p2};
    if (epi & kEpiClaims)
        wave_claims(views, pf, vis0, vis1, gs, grid, seq, lane);
    return (epi & kEpiColor) ? wave_color(views, V, pf, lane) : 0u;
}

// Arguments of the fused refine kernel (one wavefront per patch).
struct RefineArgs {
    const dpg::ViewDev *views;
    int32_t V;
    int32_t cell;
    int32_t mode;
    int32_t n;
    dp_options opt;
    dp_patch *patches;       // in/out (EVAL..EXPAND on existing patches)
    uint8_t *accept;         // optional
    uint32_t *work;          // the launch's dequeue counter (one word, zeroed per launch)
    unsigned long long *evals; // optional: total objective evaluations
    // expansion-generation fields (mode DP_MODE_EXPAND with parents != null)
    const dp_patch *parents; // queue; child c expands parents[parent0 + c/4] direction c%4
    int64_t parent0;
    int64_t max_pops;
    // narrow addressing: every view plane lies within 4 GiB above img_base, so
    // a window tap is img_base (SGPR) + a 32-bit byte offset (ViewDev::img_off)
    const char *img_base;
    int32_t narrow;
    // optional longest-first dequeue order, filled by launch_refine: groups
    // (one parent's 4 children, or one patch) by descending visible-view count
    // (a candidate costs ~E |V| texel passes), so the longest run first and
    // the launch does not end on a few long stragglers.  Scheduling only:
    // every candidate's output is independent of the order.
    uint32_t *order;         // >= ceil(n / group size) entries, or null
    uint32_t *order_scratch; // kLptBuckets * 2 counters
    // optional item list of a partitioned generation: child c
    // expands queue entry parent0 + items[c / 4] instead of parent0 + c / 4
    const int64_t *items;
    // device-resident BFS generation (dp_bfs.hip): n = gen->ncand and parent0 =
    // gen->head are read on the device (the refine_kernel<.., kGen = true>
    // instances), so a generation is queued before its size is known
    const GenDev *gen;
    // densify epilogue (kEpi* bits): colour and/or claims of the candidates that
    // pass the filter; a claim's seq is (gen ? gen->seq0 : seq0) + index
    int32_t epi;
    uint32_t seq0;
    uint32_t *claim_grid;
    double grid_scale;
};
constexpr int kLptBuckets = 129; // visible-view counts 0..128

// The device-resident BFS state of one generation (dp_bfs.hip).  Generation g
// reads state[g & 1] and its organizer writes generation g + 1's into
// state[(g + 1) & 1], so the host queues K generations behind one wait; every
// kernel of a generation sizes itself from here (ncand = 0: nothing runs).
struct GenDev {
    int64_t np;         // patches in the store before this generation's append
    int64_t head;       // queue index of the first parent (0 for the seed generation)
    int64_t items;      // parents (or seed patches) of this generation; 0 = finished
    int64_t ncand;      // candidates refined/organized: items * per_item, 0 when stalled
    int64_t cand_total; // running statistic: 4 x the expandable parents so far
    int64_t gens;       // expansion generations organized so far
    int64_t accepted;   // the previous generation's organizer accepts
    int64_t nseeds;     // seed points of the densify (sequence base of generation 1)
    int64_t seed_patches; // the seed generation's accepts (statistic)
    uint32_t seq0;      // sequence number of candidate 0
    int32_t per_item;   // 1 (seed generation) or 4 (expansion)
    int32_t stall;      // 1: ncand exceeded the candidate buffers, the host regrows them;
                        // 2: items >= the run's yield bound, the host hands the generation back
    int32_t err;        // 1: the 32-bit sequence space is exhausted
};
static_assert(sizeof(GenDev) % 8 == 0, "GenDev is copied as 64-bit words");

// organizer of one generation on the device (dp_bfs.hip)
struct BfsArgs {
    const dpg::ViewDev *views;
    int32_t V;
    int32_t k;                 // max_patches_per_cell (1: claims/resolve; > 1: k rounds)
    const GenDev *cur;
    GenDev *nxt;
    const dp_patch *cand;      // the generation's candidates in sequence order
    const uint8_t *ok;         // the refine's filter flags
    uint8_t *acc;              // organizer accepts
    uint32_t *bsum;            // kBfsBlocks per-chunk accept counts -> offsets
    uint32_t *grid;
    double grid_scale;
    uint32_t *cellmin;         // k > 1 scratch (ClaimArgs)
    uint64_t *pend;
    uint8_t *granted;
    dp_patch *store;
    int64_t store_cap;
    int64_t cand_cap;          // candidate buffer capacity (stall above it)
    int64_t max_pops;
    unsigned long long *mbox;  // status words (see dp_ctx::mbox); [7] append overflow
    uint32_t *work;            // the refine's dequeue counters, zeroed for the next generation
    uint32_t *lpt_scratch;     // the LPT order's counters, zeroed for the next generation
    int32_t fused;             // kEpi* bits the generation's refine already did (claims: k = 1 only)
    int64_t yield_items;       // > 0: a next generation of this many items or more is not run (stall 2)
};
constexpr int kBfsBlocks = 1024; // chunks of the generation's scan (one block each)

// device-resident organizer (dp_bfs.hip): claims, resolve + chunk counts, the
// chunk scan that also writes the next generation's state, and the append
// (ComputeColor) in sequence order -- four launches, every size read from
// a.cur, no host wait
hipError_t launch_bfs_organize(const BfsArgs &a, hipStream_t s);
// *dst = v on stream s (a state written by the host without a staging copy)
hipError_t launch_bfs_set_state(GenDev *dst, const GenDev &v, hipStream_t s);
// survivors of a filtered store (dp_densify_iterate): launch_keep_count leaves
// the exclusive offsets of the kBfsBlocks chunks of keep[0..n) in bsum and the
// number of nonzero flags in *total_out; launch_keep_gather then copies the
// kept records, unchanged and in index order, to dst (at most dst_cap)
hipError_t launch_keep_count(const uint8_t *keep, int64_t n, uint32_t *bsum, unsigned long long *total_out,
                             hipStream_t s);
hipError_t launch_keep_gather(const dp_patch *src, const uint8_t *keep, int64_t n, const uint32_t *bsum, dp_patch *dst,
                              int64_t dst_cap, hipStream_t s);
// per-rank accepted records of one refined share, compacted (any order) into
// a rank slot: slot[0].seq..: count header (int64 in the first 8 B of record
// 0), records from slot + 1, each with seq = its generation position
hipError_t launch_compact_slot(const dp_patch *cand, const uint8_t *acc, const int64_t *items, int64_t n, int per,
                               dp_patch *slot, hipStream_t s);
// the gathered rank slots (world of them, stride records + header each) to
// their generation positions; ok must be zeroed first.  grid != null: each
// record also claims its cells (capacity 1) at gen->seq0 + its position
struct ScatterClaims {
    const dpg::ViewDev *views;
    uint32_t *grid;
    double grid_scale;
    const GenDev *gen;
};
hipError_t launch_scatter_slots(const dp_patch *recs, int64_t stride, int world, int64_t nc, dp_patch *cand,
                                uint8_t *ok, unsigned long long *exchanged, const ScatterClaims &sc, hipStream_t s);

// one image plane of a pyramid level (BGRA8, B in the low byte)
struct PyrPlane {
    uint32_t *img;
    int32_t w, h, pitch, pad;
};

// PMVS-style filter (dp_filter.hip)
struct FilterArgs {
    const dpg::ViewDev *views;
    int32_t V;
    int32_t pad;
    const dp_patch *patches;
    int64_t n;
    const uint8_t *alive;          // patches taking part in this pass
    unsigned long long *front;     // per (view, cell): f32 depth bits << 32 | index, ~0 = empty
    double *rho;                   // per patch: grid_scale / dx in its reference view
    double grid_scale;
    double min_neighbor_frac;
};

hipError_t launch_filter_rho(const FilterArgs &a, hipStream_t s);
hipError_t launch_filter_front(const FilterArgs &a, hipStream_t s);
hipError_t launch_filter_visibility(const FilterArgs &a, uint8_t *keep, hipStream_t s);
hipError_t launch_filter_neighbors(const FilterArgs &a, uint8_t *keep, hipStream_t s);

// ---- the map stages: render, fuse, mapref, tsdf + mesh (the mesh clean-up
// keeps its arguments in dp_meshclean.hip).  Their shared device helpers are
// in dp_mapdev.h; a striped counter block (k...Stripes x k...Counters words) is
// written by its wave_count and owned by a dpk::StripedCounters (dp_buf.h). ----

// A view's projection with the adjugate and the determinant of its left 3x3
// (filled by view_inverse, dp_ctx.h): the leading member of the fuse and
// mapref view table rows
struct ViewInv {
    double P[12];
    double A[9], det;
};

// depth / index / normal / score maps (dp_render.hip; spec in
// include/densepoints.h, dp_render_maps)
struct RenderSlot { // one requested view
    int32_t view, W, H, pad;
    int64_t zoff; // first z-buffer word of the view
    float *depth; // output planes, any may be null
    int32_t *index;
    float *normal;
    float *score;
};
struct RenderPair { // one (patch, view) pair, its uniform fp64 done once
    double A[9], D, s, RR; // adj(H), det(H), |e1|^2, R^2
    int32_t x0, x1, y0, y1; // clipped candidate box, inclusive
    int32_t slot, index;
};
constexpr int kRenderCounters = 4; // patches, pairs, pixel tests, covered pixels
struct RenderArgs {
    const dpg::ViewDev *views;
    int32_t V;
    int32_t n_slots;
    const dp_patch *patches;
    const uint8_t *keep; // optional
    const double *rho;
    int64_t n;
    const RenderSlot *slots;
    const int32_t *slot_of; // DP_MAX_VIEWS entries: slot of a view, -1 = not requested
    uint64_t req[2];        // requested views as a mask
    double splat_scale, max_radius;
    int32_t all_facing, pad;
    RenderPair *pairs;
    int64_t pair_cap;
    unsigned long long *zbuf;  // per pixel: f32 depth bits << 32 | index, ~0 = empty
    unsigned long long *count; // kRenderCounters, then one pair count per chunk
};
// pairs of patches [i0, i1) into a.pairs, counted in a.count[kRenderCounters + chunk];
// (i1 - i0) * n_slots <= pair_cap
hipError_t launch_render_pairs(const RenderArgs &a, int64_t i0, int64_t i1, int chunk, hipStream_t s);
// the chunk's pairs into the z-buffer (sized from the device-held count)
hipError_t launch_render_raster(const RenderArgs &a, int chunk, hipStream_t s);
hipError_t launch_render_resolve(const RenderArgs &a, int max_pixels, hipStream_t s);

// depth / triangle-index / normal maps of a mesh (dp_meshrender.hip; spec in
// include/densepoints.h, dp_mesh_render; its arguments stay in that file)
struct MeshRenderSlot { // one requested view
    int32_t view, W, H, pad;
    int64_t zoff; // first z-buffer word of the view
    double m;     // determinant of the left 3x3 of its projection
    float *depth; // output planes, any may be null
    int32_t *index;
    float *normal;
};
struct MeshRenderPair { // one (triangle, view) pair, its uniform fp64 done once
    double r[9], D;         // the three edge rows, det [h_0 h_1 h_2]
    int64_t first;          // number of its first band within the chunk
    int32_t x0, x1, y0, y1; // clipped box, inclusive
    int32_t slot, index;
};

// vertex colours of a mesh (dp_meshcolour.hip; spec in include/densepoints.h,
// dp_mesh_colour; its arguments stay in that file)
struct MeshColourView { // one requested view; indexed wave-uniformly (scalar loads)
    double P[12], C[3];  // the level's projection, the camera centre
    const float *depth;  // W x H, the mesh as the view sees it
    const uint32_t *img; // BGRA8 plane of the current level
    int32_t W, H, pitch, view;
};

// depth-map fusion (dp_fuse.hip; spec in include/densepoints.h, dp_fuse_maps)
struct FuseView { // one requested view; indexed wave-uniformly (scalar loads)
    ViewInv inv;
    const float *depth;   // W x H
    const float *normal;  // W x H x 3, or null
    const uint32_t *img;  // BGRA8 plane of the current level
    int64_t poff;         // first pixel of the view in the mask and flag buffers
    int32_t W, H, pitch, view;
};
constexpr int kFuseBlock = 256;    // pixels per block, consecutive in one plane
constexpr int kFuseCounters = 4;   // depth pixels, matched pairs, consistent pairs, fusable
constexpr int kFuseStripes = 64;   // each counter kept kFuseStripes times (summed by the host)
struct FuseArgs {
    const FuseView *tab;
    int32_t K, min_views, no_suppress, has_normals;
    double tol, cos2;               // (double)depth_tol, cs*cs
    unsigned long long *mask;       // per pixel of the requested views
    uint8_t *flag;                  // per pixel: emitted
    unsigned long long *bcount;     // per block: emitted pixels; [blocks] = 0
    const unsigned long long *boff; // their exclusive scan; [blocks] = the total
    unsigned long long *count;      // kFuseStripes x kFuseCounters
    dp_fused_point *out;
    int64_t cap;
};
// gx blocks per view (the largest plane's), K views: block (x, k) is scan entry k * gx + x
hipError_t launch_fuse_mask(const FuseArgs &a, unsigned gx, hipStream_t s);
hipError_t launch_fuse_count(const FuseArgs &a, unsigned gx, hipStream_t s);
hipError_t launch_fuse_emit(const FuseArgs &a, unsigned gx, hipStream_t s);

// depth-map refinement (dp_mapref.hip; spec in include/densepoints.h, dp_refine_maps)
constexpr int kMaprefMaxSources = 8;
constexpr int kMaprefCounters = 6; // depth pixels in, candidates, source scores, kept, filled, moved
constexpr int kMaprefStripes = 64; // each counter kept kMaprefStripes times (summed by the host)
struct MaprefView { // one requested view; indexed wave-uniformly (scalar loads)
    ViewInv inv;
    double C[3], xr[3];     // camera centre, unit x-axis
    const float *depth;     // inputs: W x H, W x H x 3
    const float *normal;
    float *odepth;          // outputs, any may be null
    float *onormal;
    float *oscore;
    int32_t *ochoice;
    const uint16_t *gray;   // biased fp16 gray plane (0x6400 | gray), rows of gpitch
    int32_t W, H, gpitch, nsrc;
    int32_t src[kMaprefMaxSources]; // the source views as ranks into the table
};
struct MaprefArgs {
    const MaprefView *tab;
    int32_t K, window, sweep, nreach; // nreach: the non-zero reaches, compacted into reach[]
    int32_t reach[2], top_k, keep_unscored;
    double step, min_ncc, dmin; // (double)step_px, (double)min_ncc, the NCC denominator floor
    unsigned long long *count;  // kMaprefStripes x kMaprefCounters
};
// gx 16 x 16 tiles per view (the largest plane's), K views
hipError_t launch_mapref(const MaprefArgs &a, unsigned gx, hipStream_t s);

// TSDF volume and mesh (dp_tsdf.hip; spec in include/densepoints.h, dp_tsdf_integrate / dp_tsdf_mesh)
struct TsdfView { // one requested view; indexed wave-uniformly (scalar loads)
    double P[12];
    double g;             // sqrt(dot(m2, m2)), m2 = P[8..10]
    const float *depth;   // W x H
    const uint32_t *img;  // BGRA8 plane of the current level
    int32_t W, H, pitch, view;
};
constexpr int kTsdfRows = 4;       // an integrate block: 64 consecutive x of kTsdfRows rows j (one wave each)
constexpr int kTsdfCounters = 4;   // voxels, observations, observed voxels, near voxels
constexpr int kTsdfStripes = 64;   // each counter kept kTsdfStripes times (summed by the host)
constexpr int kMeshBlock = 256;    // lattice points per block, consecutive in (k, j, i) order
struct TsdfVolume {
    double origin[3], voxel; // widened from the options' floats
    int32_t nx, ny, nz;
};
struct TsdfArgs {
    const TsdfView *tab;
    int32_t K;
    TsdfVolume vol;
    double trunc;
    float *tsdf;                // outputs, any may be null
    int32_t *weight;
    uint32_t *rgb;
    unsigned long long *count;  // kTsdfStripes x kTsdfCounters
};
hipError_t launch_tsdf_integrate(const TsdfArgs &a, hipStream_t s);
struct MeshArgs {
    TsdfVolume vol;
    int32_t min_weight;
    int64_t points;                    // nx * ny * nz; cell (i, j, k) is indexed by its corner p
    const float *tsdf;
    const int32_t *weight;
    const uint32_t *rgb;               // may be null
    uint32_t *flags;                   // one byte per lattice point (7 edge bits), set by 32-bit atomicOr
    uint8_t *tcount;                   // per cell: its triangles (0 where inactive or no cell)
    uint32_t *vbase;                   // per lattice point: the number of its first vertex
    unsigned long long *bcount;        // [0, blocks]: vertices per block, then 0;
    const unsigned long long *boff;    //   [blocks + 1, 2 blocks + 1]: triangles per block, then 0; boff their scans
    unsigned long long *active;        // active cells
    int64_t blocks;
    dp_mesh_vertex *verts;
    int32_t *tris;
    int64_t vcap, tcap;
};
// the flags must be zero before launch_mesh_count; launch_mesh_vertices needs
// the vertex scan, launch_mesh_triangles the triangle scan and the vbase of
// launch_mesh_vertices
hipError_t launch_mesh_count(const MeshArgs &a, hipStream_t s);
hipError_t launch_mesh_vcount(const MeshArgs &a, hipStream_t s);
hipError_t launch_mesh_vertices(const MeshArgs &a, hipStream_t s);
hipError_t launch_mesh_triangles(const MeshArgs &a, hipStream_t s);

hipError_t launch_refine(const RefineArgs &a, hipStream_t s);
hipError_t launch_pyr_down(const PyrPlane *d_src, const PyrPlane *d_dst, int V, int max_dw, int max_dh,
                           hipStream_t s);
int read_stamps(unsigned long long *out);
hipError_t launch_probe_texel(const unsigned long long *ta, const unsigned long long *tb, const uint32_t *fxy, int n,
                              int32_t *gray);
hipError_t launch_render(const dp_synth_config &cfg, const double *P, uint32_t *out, int v,
                         hipStream_t s);
// Seed::CreatePatchesFromPoints: seed patches of n points (xyz device, 3n f64)
hipError_t launch_seed_patches(const dpg::ViewDev *views, int V, const double *xyz, int64_t n, double vis_angle,
                               double cand_angle, dp_patch *out, hipStream_t s);
// multi-GPU partition of a generation's items: super-tile keys
// (ref, tile row, tile column) of the items' centres, and the statistics of a
// cut of the key-sorted order at lo[1..world-1] (stats[2], zeroed here)
hipError_t launch_tile_keys(const dpg::ViewDev *views, const dp_patch *items, int64_t n, double tile, int64_t tx_max,
                            int64_t ty_max, uint64_t *key, int64_t *iota, unsigned long long *stats, hipStream_t s);
hipError_t launch_partition_stats(const uint64_t *key, int64_t n, int world, unsigned long long *stats, hipStream_t s);
hipError_t launch_gather_patches(const dp_patch *src, const int64_t *idx, int64_t n, dp_patch *dst, hipStream_t s);
} // namespace dpk
