// dp_ctx.h -- the context object behind the C ABI and the description of a
// refine launch, shared by the C-ABI translation units (dp_capi.hip: contexts,
// views, pyramid, filter, batch refine/expand; dp_densify.hip: the densify
// engine; dp_fast.hip: performance mode; dp_synth.hip: synthetic scenes and
// probes; dp_seeds_capi.hip, dp_seeds_orb.hip, dp_seeds_akaze.hip: seed
// generation (their own state is dp_seedgen.h); the map stages --
// dp_render.hip: maps; dp_fuse.hip: their fusion; dp_mapref.hip: their
// refinement; dp_tsdf.hip: their volume and mesh; dp_meshclean.hip: the mesh's
// components; dp_meshsmooth.hip: its adjacency, smoothing and normals;
// dp_meshdecimate.hip: its simplification; dp_meshrender.hip: its maps;
// dp_meshcolour.hip: its colours; dp_cloudnearest.hip: nearest points between
// two clouds; dp_meshnearest.hip: nearest triangles of a mesh -- each
// with its scratch as one named member of the context and
// the host helpers they share at the end of this file).  Every member that
// owns a device or pinned allocation or an event has an owning type
// (dp_buf.h), so deleting the context frees them; only the views and the
// pyramid (free_views) and the stream, which must outlive them all, are
// released by hand.
#pragma once

#include "dp_buf.h"
#include "dp_internal.h"

#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <thread>
#include <vector>

struct dp_seedgen; // seed-generation state (dp_seedgen.h)
void dp_seedgen_free(dp_seedgen *s); // delete s (dp_seeds_capi.hip)

namespace dpk {

// host-side parallel loop (the product library carries no OpenMP runtime)
template <typename F> inline void parallel_for(int64_t n, F f)
{
    unsigned hw = std::thread::hardware_concurrency();
    int64_t nt = hw ? (int64_t)(hw > 32 ? 32 : hw) : 4;
    if (nt > n)
        nt = n;
    if (nt <= 1) {
        for (int64_t i = 0; i < n; ++i)
            f(i);
        return;
    }
    std::vector<std::thread> th;
    for (int64_t t = 0; t < nt; ++t)
        th.emplace_back([=, &f]() {
            for (int64_t i = t; i < n; i += nt)
                f(i);
        });
    for (auto &x : th)
        x.join();
}

} // namespace dpk

using dpk::DevBuf;
using dpk::DevMem;
using dpk::Event;
using dpk::HostBuf;
using dpk::parallel_for;

using dpk::StripedCounters;
using dpk::Timer;

namespace dpk {

// ---- the map stages' scratch, one struct per stage (dp_ctx::render, fuse,
// mapref, tsdf, clean); `time` is the section behind the stage's *_ms, `in`,
// `out` and `io` stage the host forms' planes ----------------------------------

// dp_render_maps: the pair list, the counters (kRenderCounters, then one per
// chunk), the slot tables
struct RenderScratch {
    DevBuf<unsigned long long> count;
    DevBuf<RenderPair> pairs;
    DevBuf<RenderSlot> slots;
    DevBuf<int32_t> slot_of;
    DevBuf<unsigned char> out;
    Timer time;
};

// dp_fuse_maps: emitted flags, per-block counts and their scan, the view table,
// the host form's device and pinned points
struct FuseScratch {
    DevBuf<uint8_t> flag;
    DevBuf<unsigned long long> bcount, boff;
    StripedCounters count; // + the scan's total
    DevBuf<FuseView> tab;
    DevBuf<unsigned char> in;
    DevBuf<dp_fused_point> pts;
    HostBuf<dp_fused_point> res;
    Timer time;
};

// dp_refine_maps
struct MaprefScratch {
    DevBuf<MaprefView> tab;
    StripedCounters count;
    DevBuf<unsigned char> io;
    Timer time;
};

// dp_tsdf_integrate / dp_tsdf_mesh: the view table, the host forms' staged
// inputs and volume; the mesh's edge flags (one byte per lattice point, in
// 32-bit words), per-cell triangle counts, per-point first vertex numbers,
// per-block counts and their scans, the host form's device and pinned results
// (it times its two phases apart)
struct TsdfScratch {
    DevBuf<TsdfView> tab;
    StripedCounters count; // the mesh: the active cells' stripes + the vertex and triangle totals
    DevBuf<unsigned long long> bcount, boff;
    DevBuf<unsigned char> in, vol;
    DevBuf<uint32_t> flags, vbase;
    DevBuf<uint8_t> tcount;
    DevBuf<dp_mesh_vertex> verts;
    DevBuf<int32_t> tris;
    HostBuf<dp_mesh_vertex> hverts;
    HostBuf<int32_t> htris;
    Timer time[2];
};

// dp_mesh_components / dp_mesh_clean: the union-find parents (the labels after
// the flatten), used flags, per-root triangle and vertex counts, component
// numbers (at roots), kept flags (by component number), the rank sort's keys,
// the new vertex numbers, per-block counts and their scans, Tmax; the host
// forms' staged inputs, device results and pinned results (they time their
// phases apart)
struct CleanScratch {
    DevBuf<int32_t> parent, tcnt, vcnt, cnum, vmap, tmax;
    DevBuf<uint8_t> used, keptc;
    DevBuf<unsigned long long> keys, keys_sorted, bcount, boff;
    StripedCounters count; // + C, the kept vertex and triangle totals, Tmax
    DevBuf<unsigned char> in;
    DevBuf<int32_t> maps, tris;
    DevBuf<dp_mesh_vertex> verts;
    DevBuf<dp_mesh_component> comps;
    HostBuf<int32_t> htris;
    HostBuf<dp_mesh_vertex> hverts;
    HostBuf<dp_mesh_component> hcomps;
    Timer time[3];
};

// dp_mesh_adjacency / dp_mesh_smooth / dp_mesh_normals.  The adjacency: the
// 6T edge keys and their sorted copy (the unsorted keys' memory holds the rows'
// neighbours and counts after the sort), every sorted key's entry number, the
// offsets and flags (the outputs may be NULL or capped; the smoothing reads
// these), per-block head counts and their scan, the largest valence.  The
// smoothing: two compact position arrays (3 floats per vertex).  The normals:
// the 3T (vertex, triangle) pairs and their sorted copies.  The host forms'
// staged inputs, device results and pinned results.
struct MeshSmoothScratch {
    DevBuf<unsigned long long> keys, keys_sorted, bcount, boff;
    DevBuf<int32_t> hpos, off, maxval;
    DevBuf<uint8_t> vflags;
    StripedCounters count; // + the entry total, the largest valence
    DevBuf<float> pos[2];
    DevBuf<uint32_t> ikeys, ikeys_sorted;
    DevBuf<int32_t> itris, itris_sorted;
    DevBuf<unsigned char> in;
    DevBuf<int32_t> csr;
    DevBuf<dp_mesh_vertex> verts;
    DevBuf<float> normals;
    HostBuf<int32_t> hcsr;
    HostBuf<uint8_t> hflags;
    HostBuf<dp_mesh_vertex> hverts;
    HostBuf<float> hnormals;
    Timer time[2]; // the adjacency; the steps or the normals
};

// dp_mesh_decimate.  The vertices: used flags, the cell keys with the vertex
// numbers and their sorted copies (a cluster is a run of equal keys, its
// members ascending), the cluster of every vertex, the first sorted position of
// every cluster (K + 1 entries).  The triangles: the canonical-triple keys with
// the triangle numbers, their sorted copies and the kept flags.  The clusters:
// survivor flags and output numbers.  QUADRIC: the 3T (cluster, triangle) pairs
// and their sorted copies.  Per-block counts and their scans (cluster heads,
// survivors, kept triangles), the largest cluster; the host form's staged
// inputs, device results and pinned results.
struct MeshDecimateScratch {
    DevBuf<uint8_t> used, tkeep, surv;
    DevBuf<unsigned long long> vkeys, vkeys_sorted, tkeys, tkeys_sorted, bcount, boff;
    DevBuf<int32_t> vidx, vidx_sorted, cid, cstart, tval[2], cout, maxval;
    DevBuf<uint32_t> pkeys, pkeys_sorted;
    DevBuf<int32_t> ptris, ptris_sorted;
    StripedCounters count; // + K, the output vertex and triangle totals, the largest cluster
    DevBuf<unsigned char> in;
    DevBuf<int32_t> maps, tris;
    DevBuf<dp_mesh_vertex> verts;
    HostBuf<int32_t> htris;
    HostBuf<dp_mesh_vertex> hverts;
    Timer time;
};

// dp_mesh_render: the pair list, the counters (the statistics, then one packed
// pair / band counter per chunk), the slot table; the host form's staged mesh
// and planes.  The z-buffer is the context's pix64.
struct MeshRenderScratch {
    DevBuf<unsigned long long> count;
    DevBuf<MeshRenderPair> pairs;
    DevBuf<MeshRenderSlot> slots;
    DevBuf<unsigned char> in, out;
    Timer time;
};

// dp_mesh_colour: the view table, the counters; the host form's staged vertices,
// normals and planes, its device results (vertices, seen, best) and the pinned
// vertices it returns
struct MeshColourScratch {
    DevBuf<MeshColourView> tab;
    StripedCounters count;
    DevBuf<unsigned char> in, out;
    HostBuf<dp_mesh_vertex> hverts;
    Timer time;
};

// dp_cloud_nearest's search grid, made on the device from the targets' bounding
// box (cloud_plan_kernel): cell (x, y, z) has the key (z * n[1] + y) * n[0] + x
struct CloudGrid {
    double origin[3], cell[3];
    int32_t n[3];
    int32_t maxcell; // the most targets in one cell
    int64_t cells;
};

// dp_cloud_nearest.  The targets: the per-block bounding boxes, the grid, the
// cell keys with the target numbers and their sorted copies, the sorted targets'
// coordinates, the first sorted position of every cell (cap + 1 entries).  The
// queries: their cell keys and numbers and the sorted copies.  The host form's
// staged clouds, device results (index, dist, hist) and pinned results.
struct CloudNearestScratch {
    DevBuf<float> boxes, tx, ty, tz;
    DevBuf<CloudGrid> grid;
    DevBuf<uint32_t> tkeys, tkeys_sorted, qkeys, qkeys_sorted;
    DevBuf<int32_t> tidx, tidx_sorted, qidx, qidx_sorted, begin;
    StripedCounters count; // + the grid
    DevBuf<unsigned char> in, out;
    HostBuf<int32_t> hindex;
    HostBuf<float> hdist;
    HostBuf<uint64_t> hhist;
    Timer time[2]; // the grid; the queries
};

// what dp_cloud_clean's one-lane statistics kernel keeps on the device between
// its kernels: the eligible points, mu, sigma and the threshold T, the kept count
struct CloudCleanDev {
    double mu, sigma, threshold;
    int64_t eligible, kept;
};

// dp_cloud_knn and dp_cloud_clean (dp_cloudknn.hip).  The grid, the sorted
// targets and the queries' order are CloudNearestScratch's: the two searches
// never overlap on a context.  Here: the host forms' staged inputs, device
// results and pinned results (one buffer each, laid out by a PlanePacker); the
// filter's self-search rows and counts, the points' mean distances, the two
// buffers the pairwise-sum passes alternate between, the statistics block, the
// keep flags as int32 with their exclusive scan (n + 1 entries each).
struct CloudKnnScratch {
    DevBuf<unsigned char> in, out;
    HostBuf<unsigned char> hout;
    DevBuf<int32_t> rows, rowcount, flag, pos;
    DevBuf<double> mean, sum[2];
    DevBuf<CloudCleanDev> dev;
    StripedCounters count; // dp_cloud_clean's; + the grid and the statistics block
    Timer time[2];         // dp_cloud_clean: the search; the filter
};

// dp_cloud_normals (dp_cloudnormals.hip).  The search is dp_cloud_knn's and the
// self-search rows and counts, the host form's staged input, device results and
// pinned results are CloudKnnScratch's (a call of one ends the validity of the
// other's host results).  Here: the counters and the two times.
struct CloudNormalsScratch {
    StripedCounters count; // + the grid
    Timer time[2];         // the search; everything after it
};

// what dp_cloud_align keeps on the device between its kernels: the current M and
// its scale, the means of the last pass, the rms of the step before, the
// targets taking part (the grid's counter, which every pass zeroes again), and
// the 24 bytes the host reads after every pass: the record and the verdict
// (-1 = M was updated, else the DP_CLOUD_ALIGN_STOP_* reason)
struct CloudAlignDev {
    double M[12], scale, mux[3], muq[3], rms_prev;
    int64_t targets;
    int64_t matched;
    double rms;
    int64_t verdict;
};

// dp_cloud_align and dp_cloud_transform (dp_cloudalign.hip).  The search is
// CloudNearestScratch's.  Here: the transformed source (packed xyz), the last
// pass's index and dist when the caller wants none, the two buffers the
// multi-channel sum levels alternate between, the state block and its pinned
// copy (the record, then the whole block at the end); the host forms' staged
// inputs, device results and pinned results.
struct CloudAlignScratch {
    DevBuf<float> y, dist;
    DevBuf<int32_t> index;
    DevBuf<double> sum[2];
    DevBuf<CloudAlignDev> dev;
    HostBuf<CloudAlignDev> hdev;
    DevBuf<unsigned char> in, out;
    HostBuf<unsigned char> hout;
    Timer time; // everything after the grid
};

// dp_mesh_nearest's search grid, made on the device (meshnear_plan_kernel,
// meshnear_pick_kernel): isotropic cells of side0 * 2^level from one origin,
// cell (x, y, z) with the key (z * n[1] + y) * n[0] + x
struct MeshNearGrid {
    double origin[3], ext[3], side0, side;
    int32_t n[3];
    int32_t level_min; // the first level whose cells fit the cap
    int32_t level;     // the chosen one
    int32_t maxcell;   // the most registrations in one cell
    int64_t cells, entries;
};

// dp_mesh_nearest.  The triangles: the per-block bounding boxes, the grid, the
// per-level registration counts, the cells' counts and first entries (cap + 1
// each), the registrations (triangle and first-cell bits).  The queries: their
// cell keys and numbers and the sorted copies.  The host form's staged inputs,
// device results (index, dist, closest, hist) and pinned results.
struct MeshNearestScratch {
    DevBuf<float> boxes;
    DevBuf<MeshNearGrid> grid;
    DevBuf<unsigned long long> levels;
    DevBuf<int32_t> cellcount, begin, entries;
    DevBuf<uint8_t> first;
    DevBuf<uint32_t> qkeys, qkeys_sorted;
    DevBuf<int32_t> qidx, qidx_sorted;
    StripedCounters count; // + the grid
    DevBuf<unsigned char> in, out;
    HostBuf<int32_t> hindex;
    HostBuf<float> hdist, hclosest;
    HostBuf<uint64_t> hhist;
    Timer time[2]; // the grid; the queries
};

} // namespace dpk

struct SeedgenFree {
    void operator()(dp_seedgen *s) const { dp_seedgen_free(s); }
};

struct dp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    dp_options opt{};
    std::string err;
    int V = 0;
    std::vector<dpg::ViewDev> hv;
    dpg::ViewDev *d_views = nullptr;
    std::vector<uint32_t *> own_img;
    const char *img_base = nullptr; // lowest view plane address
    // image pyramid: planes[l][v] (level 0 = the views as set), pools of levels >= 1
    std::vector<double> P0;                          // V x 12 level-0 projections
    std::vector<std::vector<dpk::PyrPlane>> planes;
    std::vector<uint32_t *> pyr_pool;
    int level = 0;
    bool narrow = false;            // all planes within 4 GiB of img_base (32-bit tap offsets)
    DevBuf<uint32_t> d_work;
    DevBuf<unsigned long long> d_evals;
    Event e0, e1;
    bool timed = false;
    int64_t grid_cells = 0;
    DevBuf<uint32_t> grid;
    DevBuf<uint32_t> cellmin; // organizer with cell capacity > 1: per-round minima
    DevBuf<uint64_t> pend;    // ... and per-candidate undecided claims
    DevBuf<uint8_t> granted;
    DevBuf<uint32_t> lpt;    // refine dequeue order + its counters
    bool lpt_off = false;    // DP_NO_LPT=1 at dp_ctx_create: index-order dequeue
    int64_t gen_cap_test = 0; // DP_GEN_CAP at dp_ctx_create: the device BFS's first candidate capacity (tests)
    DevBuf<dp_patch> pat, store, cand;
    DevBuf<uint8_t> ok, acc;
    DevBuf<unsigned char> scan_tmp;
    // patch filter scratch
    DevBuf<unsigned long long> front;
    DevBuf<uint8_t> f_alive, f_keep;
    DevBuf<double> f_rho;
    DevBuf<dp_patch> f_pat;
    // Buffers shared on purpose by stages whose calls never overlap on a context:
    //   pix64          8 B per pixel of the requested views: dp_render_maps'
    //                  and dp_mesh_render's z-buffer and dp_fuse_maps' masks
    //   f_rho          the filter's rho, which is also dp_render_maps' splat radius
    //   f_pat, f_keep  the filter's staging of host patches and flags, which the
    //                  host form of dp_render_maps stages its own in
    DevBuf<unsigned long long> pix64;
    dpk::RenderScratch render;
    dpk::FuseScratch fuse;
    dpk::MaprefScratch mapref;
    dpk::TsdfScratch tsdf;
    dpk::CleanScratch clean;
    dpk::MeshSmoothScratch smooth;
    dpk::MeshDecimateScratch decimate;
    dpk::MeshRenderScratch meshrender;
    dpk::MeshColourScratch meshcolour;
    dpk::CloudNearestScratch cloudnearest;
    dpk::CloudKnnScratch cloudknn;
    dpk::CloudNormalsScratch cloudnormals;
    dpk::CloudAlignScratch cloudalign;
    dpk::MeshNearestScratch meshnearest;
    HostBuf<dp_patch> result; // dp_densify / dp_densify_result output (pinned)
    // dp_densify_iterate: per iteration {evaluations, filter survivors} on the
    // device (read once, at the end) and the filters' timing events
    DevBuf<unsigned long long> itw;
    std::vector<Event> fev;
    // generation-at-a-time densify (dp_densify_begin/refine/commit/result)
    DevBuf<dp_patch> seedp;  // seed patches of generation 0
    DevBuf<double> seedx;    // seed points (3 f64 each) on the device
    DevBuf<dp_patch> sconv;  // dp_seeds_to_patches output staging
    DevBuf<int64_t> items;   // item list of a partitioned refine / commit
    // partitioned generations: super-tile keys, key-sorted keys and item order
    // (the rank-major order), the cut positions, partition statistics
    DevBuf<uint64_t> tkeys, okeys;
    DevBuf<int64_t> oiota, porder, olo;
    int64_t part_stats[4] = {0, 0, 0, 0}; // items, world, tiles, items in split tiles
    bool part_pending = false;            // a partition's tiles/split counts wait in mbox[2..3]
    // status words read back with the generation's state (one wait per
    // generation or batch): [0] organizer accepts, [2] tiles, [3] items in
    // split tiles (the partition), [4] records exchanged (the slot scatter),
    // [7] the append's overflow flag (cleared when read)
    DevBuf<unsigned long long> mbox;
    // device-resident BFS (dp_bfs.hip): the GenDev pair, chunk counts, the slot
    // holding the next generation's state, the LPT counters the organizer
    // zeroes, the timing events of a batch
    DevBuf<dpk::GenDev> gstate;
    DevBuf<uint32_t> bsum;
    int g_slot = 0;
    uint32_t *g_lpt_scratch = nullptr;
    std::vector<Event> gev;
    DevBuf<dp_patch> wcand; // a rank's refined share (partitioned generations)
    DevBuf<uint8_t> wok;
    Event ej;                  // stream joins (no host wait)
    bool g_time_pending = false; // a densify refine's events (e0, e1) not yet read
    int64_t g_np = 0;        // patches in the replicated store
    int64_t g_nseeds = 0;
    int64_t g_expected = -1; // generation index the next commit must carry
    dp_densify_stats g_st{};
    std::chrono::steady_clock::time_point g_t0;
    // seed generation (Features::Matcher, dp_seeds.hip)
    std::unique_ptr<dp_seedgen, SeedgenFree> seeds;
    // performance mode (dp_fast.hip): options and the fp16 gray planes of one level
    dp_fast_options fopt{4, 2, 6656, 8, 0.5f, 1.0f, 0, 0, 32}; // = dp_default_fast_options (tests/test_gpu_fast.py)
    DevMem gray_pool;          // __half planes, pitch = width rounded up to 64
    size_t gray_cap = 0;       // elements
    DevMem d_gray;             // device GrayPlane table
    bool gray_ready = false;
    DevBuf<unsigned long long> d_fstats;    // dp_fast_stats counters of the last launch
    int gray_level = -1, gray_V = 0;
};

namespace dpk {

// One refine launch as its caller describes it, for either engine (the parity
// kernel, dp_refine.hip, or the performance kernel, dp_fast_kernel.hip); everything
// an engine derives from the context stays in refine_args / dp_fast_launch.
// Refine/eval of n patches in device memory, or with parents the 4 (n / 4)
// expansion children of parents[parent0 + (items ? items[k] : k)], k < n / 4.
// Callers brace-initialise the first five members, in this order, and name the rest.
struct RefineJob {
    dp_patch *patches = nullptr; // in/out; with parents, the children (out)
    uint8_t *accept = nullptr;   // optional
    int n = 0;                   // with gen: the candidate buffers' capacity
    int cell = 0;
    int mode = 0;                // DP_MODE_*; >= DP_MODE_FAST_EVAL: the performance kernel
    const dp_patch *parents = nullptr;
    int64_t parent0 = 0;
    const int64_t *items = nullptr;
    // only parents with an index below max_pops expand (dp_densify's pop cap);
    // both kernels read it under `parents` only, so a launch without parents
    // leaves the default
    int64_t max_pops = INT64_MAX;
    const GenDev *gen = nullptr; // a device-resident BFS generation (its size and parent0 read on the device)
    int epi = 0;                 // the densify epilogue (kEpi* bits; claims at seq0 + index into c->grid)
    uint32_t seq0 = 0;
    // The (e0, e1) event pair behind dp_last_kernel_ms.  The performance engine
    // records it on every launch; the parity engine records it (and sets
    // c->timed) unless this is set, which refine_gen does: its batch times
    // each generation with the gev events, and dp_last_kernel_ms keeps naming
    // the last launch outside the batch.
    bool parity_untimed = false;
};

} // namespace dpk

// performance-mode launch of a job (dp_fast.hip)
int dp_fast_launch(dp_ctx *c, const dpk::RefineJob &job, hipStream_t s);

// shared by the batch API (dp_capi.hip, where they live) and the densify
// engine (dp_densify.hip)
dpk::RefineArgs refine_args(dp_ctx *c, const dpk::RefineJob &job);
// the job on the engine job.mode names
int launch_job(dp_ctx *c, const dpk::RefineJob &job, hipStream_t s);
int check_refine(dp_ctx *c, int n, int cell, int mode);
// n host seed points -> seed patches in device memory d_out (async on s)
int seeds_device(dp_ctx *c, const double *xyz, int64_t n, dp_patch *d_out, hipStream_t s);
// the epilogue a densify generation's refine runs: the colours always, the
// claims when the organizer's capacity is 1 (k > 1 claims in rounds)
int densify_epi(const dp_ctx *c);
// View::SetProjectionMatrix: the ViewDev of a W x H view with projection P
int view_from_P(const double *P, int W, int H, int gs, dpg::ViewDev &v);

static inline int fail(dp_ctx *c, int code, const std::string &msg)
{
    if (c)
        c->err = msg;
    return code;
}

// ---- host helpers shared by the map stages' C-ABI halves ----------------------

// The `views` argument of a map stage: set, 1..min(V, cap) ids, each unique and
// < V; `who` is the entry point named in the message.  A stage without a cap
// of its own passes DP_MAX_VIEWS.
static inline int check_view_list(dp_ctx *c, const char *who, const int32_t *views, int n_views, int cap)
{
    const std::string w(who);
    if (c->V <= 0)
        return fail(c, DP_E_STATE, w + ": no views set");
    if (!views || n_views < 1 || n_views > c->V || n_views > cap)
        return fail(c, DP_E_ARG,
                    w + (cap < DP_MAX_VIEWS ? ": n_views must be in 1..min(V, " + std::to_string(cap) + ")"
                                            : ": n_views must be in 1..V"));
    uint64_t seen[2] = {0, 0};
    for (int k = 0; k < n_views; ++k) {
        const int32_t v = views[k];
        if (v < 0 || v >= c->V || ((seen[v >> 6] >> (v & 63)) & 1ull))
            return fail(c, DP_E_ARG, w + ": view ids must be unique and < V");
        seen[v >> 6] |= 1ull << (v & 63);
    }
    return DP_OK;
}

// P of the view with the adjugate and the determinant of its left 3x3 (the
// spec's view table entry); false when the matrix is singular
static inline bool view_inverse(const dpg::ViewDev &v, dpk::ViewInv &t)
{
    const double *P = v.P;
    const double h[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    for (int j = 0; j < 12; ++j)
        t.P[j] = P[j];
    t.det = dpg::adjugate3(h, t.A);
    return t.det != 0.0 && std::isfinite(t.det);
}

// pixels of view v at the current level
static inline size_t view_pixels(const dp_ctx *c, int32_t v) { return (size_t)c->hv[v].W * (size_t)c->hv[v].H; }

// the layout of a host form's planes in one staging buffer: add returns the
// plane's offset, 256-B aligned; total is the buffer's size
struct PlanePacker {
    size_t total = 0;
    size_t add(size_t bytes)
    {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    }
};

#define DP_HIP(c, expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail((c), _e == hipErrorOutOfMemory ? DP_E_OOM : DP_E_HIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                   \
    } while (0)
