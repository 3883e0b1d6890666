// dp_ctx.h -- the context object behind the C ABI and the description of a
// refine launch, shared by the C-ABI translation units (dp_capi.hip: contexts,
// views, pyramid, filter, batch refine/expand; dp_densify.hip: the densify
// engine; dp_fast.hip: performance mode; dp_synth.hip: synthetic scenes and
// probes; dp_seeds_capi.hip, dp_seeds_orb.hip, dp_seeds_akaze.hip: seed
// generation (their own state is dp_seedgen.h); dp_render.hip: maps;
// dp_fuse.hip: their fusion; dp_mapref.hip: their refinement; dp_tsdf.hip:
// their volume and mesh; dp_meshclean.hip: the mesh's components).  Every member that owns a device or pinned
// allocation or an event has an owning type (dp_buf.h), so deleting the
// context frees them; only the views and the pyramid (free_views) and the
// stream, which must outlive them all, are released by hand.
#pragma once

#include "dp_buf.h"
#include "dp_internal.h"

#include <chrono>
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
    // dp_render_maps: z-buffer (8 B per pixel of the requested views), pair list,
    // counters (dpk::kRenderCounters, then one per chunk), slot tables, the host
    // form's output planes, timing events
    DevBuf<unsigned long long> r_z, r_count;
    DevBuf<dpk::RenderPair> r_pairs;
    DevBuf<dpk::RenderSlot> r_slots;
    DevBuf<int32_t> r_slot_of;
    DevBuf<unsigned char> r_out;
    Event r_e0, r_e1;
    // dp_fuse_maps: the per-pixel masks live in r_z (8 B per pixel of the
    // requested views, as the z-buffer; the calls never overlap); emitted flags,
    // per-block counts and their scan, striped counters, the view table, the
    // host form's staged planes and points, the statistics read, timing events
    DevBuf<uint8_t> u_flag;
    DevBuf<unsigned long long> u_bcount, u_boff, u_count;
    DevBuf<dpk::FuseView> u_tab;
    DevBuf<unsigned char> u_in;
    DevBuf<dp_fused_point> u_pts;
    HostBuf<dp_fused_point> u_res;
    HostBuf<unsigned long long> u_hcount;
    Event u_e0, u_e1;
    // dp_refine_maps: the view table, striped counters and their host copy,
    // the host form's staged input and output planes, timing events
    DevBuf<dpk::MaprefView> m_tab;
    DevBuf<unsigned long long> m_count;
    HostBuf<unsigned long long> m_hcount;
    DevBuf<unsigned char> m_io;
    Event m_e0, m_e1;
    // dp_tsdf_integrate / dp_tsdf_mesh: the view table, striped counters and the
    // statistics read, the host forms' staged inputs and volume; the mesh's edge
    // flags (one byte per lattice point, in 32-bit words), per-cell triangle
    // counts, per-point first vertex numbers, per-block counts and their scans,
    // the host form's device and pinned results, timing events (the host form
    // of the mesh times its two phases apart)
    DevBuf<dpk::TsdfView> t_tab;
    DevBuf<unsigned long long> t_count, t_bcount, t_boff;
    HostBuf<unsigned long long> t_hcount;
    DevBuf<unsigned char> t_in, t_vol;
    DevBuf<uint32_t> t_flags, t_vbase;
    DevBuf<uint8_t> t_tcount;
    DevBuf<dp_mesh_vertex> t_verts;
    DevBuf<int32_t> t_tris;
    HostBuf<dp_mesh_vertex> t_hverts;
    HostBuf<int32_t> t_htris;
    Event t_e0, t_e1, t_e2, t_e3;
    // dp_mesh_components / dp_mesh_clean: the union-find parents (the labels
    // after the flatten), used flags, per-root triangle and vertex counts,
    // component numbers (at roots), kept flags (by component number), the rank
    // sort's keys, the new vertex numbers, per-block counts and their scans,
    // striped counters, Tmax, the statistics read; the host forms' staged
    // inputs, device results and pinned results; timing events (the host forms
    // time their phases apart)
    DevBuf<int32_t> c_parent, c_tcnt, c_vcnt, c_cnum, c_vmap, c_tmax;
    DevBuf<uint8_t> c_used, c_keptc;
    DevBuf<unsigned long long> c_keys, c_keys_sorted, c_bcount, c_boff, c_count;
    HostBuf<unsigned long long> c_hcount;
    DevBuf<unsigned char> c_in;
    DevBuf<int32_t> c_maps, c_tris;
    DevBuf<dp_mesh_vertex> c_verts;
    DevBuf<dp_mesh_component> c_comps;
    HostBuf<int32_t> c_htris;
    HostBuf<dp_mesh_vertex> c_hverts;
    HostBuf<dp_mesh_component> c_hcomps;
    Event c_e[6];
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

#define DP_HIP(c, expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail((c), _e == hipErrorOutOfMemory ? DP_E_OOM : DP_E_HIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                   \
    } while (0)
