// dp_densify.hip -- C ABI (include/densepoints.h): the device-side BFS
// densify driver (dp_densify, the generation-at-a-time and one-wait device
// protocols, resume, dp_densify_iterate).
//
// The reference's PMVS driver (methods/pmvs/pmvs.cpp:22-43) runs
//   seeds -> Seed::FilterPatches/OptimizePatches (cell 16) ->
//   PatchOrganizer::SetSeeds -> Expand::ExpandPatches (FIFO, cell 11).
// Here the FIFO runs generation-synchronously on the GPU: generation g+1 is
// every child of the queue slice [head, np) in (parent, direction) order,
// refined by one fused kernel; organizer claims resolve by minimum sequence
// number, which equals the single-thread FIFO's insertion order exactly.
#include "dp_ctx.h"
#include "../../include/densepoints_probe.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------
// densify: seeds -> organizer -> generation-synchronous BFS, device-resident.
// Every expansion generation (refine + the dp_bfs.hip organizer) reads its
// size from the GenDev state on the device, so dp_densify / dp_densify_run
// queue kGenBatch generations behind ONE host wait; the state's stall flag
// stops a batch whose next generation outgrows the candidate buffers (the
// host grows them and resumes there).
// ---------------------------------------------------------------------------

static constexpr int kGenBatch = 8;

// organizer grid of an empty store: capacity 1 keeps the owner seq per cell
// (UINT32_MAX = free), capacity k > 1 the claims made (0) plus the per-round
// minima (UINT32_MAX)
static int reset_grid(dp_ctx *c, hipStream_t s)
{
    const size_t cells = (size_t)c->grid_cells + 1;
    DP_HIP(c, c->grid.reserve(cells));
    if (c->opt.max_patches_per_cell == 1) {
        DP_HIP(c, hipMemsetAsync(c->grid.p, 0xFF, sizeof(uint32_t) * cells, s));
    } else {
        DP_HIP(c, hipMemsetAsync(c->grid.p, 0, sizeof(uint32_t) * cells, s));
        DP_HIP(c, c->cellmin.reserve(cells));
        DP_HIP(c, hipMemsetAsync(c->cellmin.p, 0xFF, sizeof(uint32_t) * cells, s));
    }
    return DP_OK;
}

// patch store capacity, the smaller of two bounds on the accepted patches:
// every accepted patch holds >= 2 claims and a cell takes at most
// max_patches_per_cell of them; and the store holds at most the seed patches
// plus 4 children per pop, pops <= max_pops (expand.cpp:95).  (The first alone
// reserved ~42 GB at config 5 with k = 16.)
static int64_t store_capacity(const dp_ctx *c, int64_t nseeds)
{
    const int64_t by_cells = (int64_t)c->opt.max_patches_per_cell * c->grid_cells / 2;
    const int64_t pops = c->opt.max_pops > 0 ? c->opt.max_pops : 0;
    const int64_t by_pops = nseeds + 4 * pops;
    return (by_cells < by_pops ? by_cells : by_pops) + 16;
}

// the organizer's buffers for generations of up to cap candidates (reserved
// before anything is queued on them: a reserve that grows frees the old buffer)
static int reserve_organizer(dp_ctx *c, int64_t cap)
{
    DP_HIP(c, c->gstate.reserve(2));
    DP_HIP(c, c->bsum.reserve(dpk::kBfsBlocks));
    DP_HIP(c, c->acc.reserve((size_t)cap + 1));
    if (c->opt.max_patches_per_cell > 1) {
        DP_HIP(c, c->pend.reserve(2 * (size_t)cap + 2));
        DP_HIP(c, c->granted.reserve((size_t)cap + 1));
    }
    return DP_OK;
}

// timing events: a pair per generation of a batch, and the seed refine's pair
static int ensure_gen_events(dp_ctx *c)
{
    if (!c->gev.empty())
        return DP_OK;
    c->gev.resize(2 * kGenBatch + 2);
    for (auto &e : c->gev)
        DP_HIP(c, e.create());
    return DP_OK;
}

static int set_state(dp_ctx *c, int slot, const dpk::GenDev &g, hipStream_t s)
{
    DP_HIP(c, dpk::launch_bfs_set_state(c->gstate.p + slot, g, s));
    return DP_OK;
}

// the organizer of the generation in state slot `slot` over cand/okf (in
// sequence order); writes the next generation's state into slot ^ 1.
// cand_cap: the candidate buffers' capacity (the next generation stalls above it)
static int organize_gen(dp_ctx *c, const dp_patch *cand, const uint8_t *okf, int slot, int64_t cand_cap, hipStream_t s,
                        int fused, int64_t yield_items = 0)
{
    dpk::BfsArgs b{};
    b.views = c->d_views;
    b.V = c->V;
    b.k = c->opt.max_patches_per_cell;
    b.cur = c->gstate.p + slot;
    b.nxt = c->gstate.p + (slot ^ 1);
    b.cand = cand;
    b.ok = okf;
    b.acc = c->acc.p;
    b.bsum = c->bsum.p;
    b.grid = c->grid.p;
    b.grid_scale = (double)c->opt.grid_scale;
    b.cellmin = c->cellmin.p;
    b.pend = c->pend.p;
    b.granted = c->granted.p;
    b.store = c->store.p;
    b.store_cap = (int64_t)c->store.cap;
    b.cand_cap = cand_cap;
    b.max_pops = c->opt.max_pops;
    b.mbox = c->mbox.p;
    b.work = c->d_work.p;
    b.lpt_scratch = c->g_lpt_scratch;
    b.fused = fused;
    b.yield_items = yield_items;
    DP_HIP(c, dpk::launch_bfs_organize(b, s));
    return DP_OK;
}

// The generation's status: the state in `slot` (the next generation) and the
// status words (accepts, partition statistics, records exchanged, the
// append's overflow flag, cleared here) -- one wait.
static int read_state(dp_ctx *c, int slot, hipStream_t s, dpk::GenDev *g, unsigned long long mb[8])
{
    DP_HIP(c, hipMemcpyAsync(g, c->gstate.p + slot, sizeof(dpk::GenDev), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(mb, c->mbox.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    if (mb[7]) {
        DP_HIP(c, hipMemsetAsync(c->mbox.p + 7, 0, sizeof(unsigned long long), s));
        return fail(c, DP_E_OOM, "patch store overflow");
    }
    if (g->err)
        return fail(c, DP_E_OOM, "sequence space exhausted");
    if (c->part_pending) {
        c->part_stats[2] = (int64_t)mb[2];
        c->part_stats[3] = (int64_t)mb[3];
        c->part_pending = false;
    }
    return DP_OK;
}

// the refine events of a host-driven generation (recorded by launch_job),
// read after the generation's wait: no extra wait
static int take_refine_ms(dp_ctx *c, double *acc_ms)
{
    if (!c->g_time_pending)
        return DP_OK;
    c->g_time_pending = false;
    DP_HIP(c, hipEventSynchronize(c->e1));
    float f = 0.f;
    DP_HIP(c, hipEventElapsedTime(&f, c->e0, c->e1));
    *acc_ms += f;
    return DP_OK;
}

// make `to` wait for the work queued on `from` so far (device-side, no host wait)
static int join_streams(dp_ctx *c, hipStream_t from, hipStream_t to)
{
    if (from == to)
        return DP_OK;
    DP_HIP(c, hipEventRecord(c->ej, from));
    DP_HIP(c, hipStreamWaitEvent(to, c->ej, 0));
    return DP_OK;
}

// host mirror of the state: the API's generation record and the statistics
static void take_state(dp_ctx *c, const dpk::GenDev &g, dp_generation *gen)
{
    c->g_np = g.np;
    c->g_st.seed_patches = g.seed_patches;
    c->g_st.candidates = g.cand_total;
    c->g_st.generations = (int32_t)g.gens;
    if (gen) {
        gen->index = 1 + (int32_t)g.gens;
        gen->head = g.head;
        gen->items = g.items;
        gen->per_item = 4;
        gen->cell = c->opt.expand_cell_size;
        gen->seq0 = g.seq0;
        c->g_expected = gen->index;
    }
}

// The refine of n candidates of a densify stage (DP_MODE_SEED or
// DP_MODE_EXPAND) into d / okf: the performance refine with
// dp_fast_options.densify, else the stage's parity mode.  An expansion stage
// reads its parents from the store, under the pop cap; the caller adds where
// they start (parent0, items or gen).
static dpk::RefineJob densify_job(const dp_ctx *c, int stage, dp_patch *d, uint8_t *okf, int n, int cell, int epi)
{
    dpk::RefineJob job{d, okf, n, cell, c->fopt.densify ? DP_MODE_FAST_REFINE : stage};
    job.epi = epi;
    if (stage == DP_MODE_EXPAND) {
        job.parents = c->store.p;
        job.max_pops = c->opt.max_pops;
    }
    return job;
}

// The refine of the generation in state slot `slot` (device-sized): Expand::
// ExpandPatch of the queue slice [head, head + items) into c->cand / c->ok.
static int refine_gen(dp_ctx *c, int slot, int64_t cap, hipStream_t s)
{
    dpk::RefineJob job =
        densify_job(c, DP_MODE_EXPAND, c->cand.p, c->ok.p, (int)cap, c->opt.expand_cell_size, densify_epi(c));
    job.gen = c->gstate.p + slot; // size, head and seq0 from the state
    job.parity_untimed = true;    // the batch's gev events time each generation
    return launch_job(c, job, s);
}

// the device-resident loop supports the default refines (the analytic-
// gradient performance refine is host-driven)
static bool device_loop_ok(const dp_ctx *c) { return !(c->fopt.densify && c->fopt.gradient); }

// Up to max_gens expansion generations from the state in c->g_slot, kGenBatch
// per host wait (dp_densify, dp_densify_run).  cap0: the candidate capacity
// to start with.  Leaves the state of the first generation not run in c->g_slot.
static int run_generations(dp_ctx *c, int64_t max_gens, int64_t cap0, hipStream_t s, dpk::GenDev *last,
                           int64_t yield_items = 0)
{
    int64_t cap = std::max<int64_t>(cap0, 1024);
    if (c->gen_cap_test > 0)
        cap = c->gen_cap_test; // DP_GEN_CAP (tests): small buffers, so generations stall and resume
    int64_t done = 0;
    dpk::GenDev g{};
    unsigned long long mb[8];
    int rc0 = ensure_gen_events(c);
    if (rc0 != DP_OK)
        return rc0;
    for (;;) {
        if (cap > INT32_MAX)
            cap = INT32_MAX;
        DP_HIP(c, c->cand.reserve((size_t)cap));
        DP_HIP(c, c->ok.reserve((size_t)cap));
        int rc = reserve_organizer(c, cap);
        if (rc != DP_OK)
            return rc;
        c->g_lpt_scratch = nullptr;
        if (!c->lpt_off && !c->fopt.densify) {
            DP_HIP(c, c->lpt.reserve((size_t)cap + 2 * dpk::kLptBuckets));
            c->g_lpt_scratch = c->lpt.p + cap;
        }
        // the first generation's counters (later ones are zeroed by the previous organizer)
        DP_HIP(c, hipMemsetAsync(c->d_work.p, 0, sizeof(uint32_t), s));
        if (c->fopt.densify) {
            // dp_fast_last_stats: the batch's generations count as one launch
            DP_HIP(c, c->d_fstats.reserve(8));
            DP_HIP(c, hipMemsetAsync(c->d_fstats.p, 0, 8 * sizeof(unsigned long long), s));
        }
        if (c->g_lpt_scratch)
            DP_HIP(c, hipMemsetAsync(c->g_lpt_scratch, 0, 2 * dpk::kLptBuckets * sizeof(uint32_t), s));
        const int k = (int)std::min<int64_t>(kGenBatch, max_gens - done);
        int slot = c->g_slot;
        for (int i = 0; i < k; ++i) {
            DP_HIP(c, hipEventRecord(c->gev[2 * i], s));
            rc = refine_gen(c, slot, cap, s);
            if (rc != DP_OK)
                return rc;
            DP_HIP(c, hipEventRecord(c->gev[2 * i + 1], s));
            rc = organize_gen(c, c->cand.p, c->ok.p, slot, cap, s, densify_epi(c), yield_items);
            if (rc != DP_OK)
                return rc;
            slot ^= 1;
        }
        rc = read_state(c, slot, s, &g, mb);
        if (rc != DP_OK)
            return rc;
        for (int i = 0; i < k; ++i) {
            float f = 0.f;
            DP_HIP(c, hipEventElapsedTime(&f, c->gev[2 * i], c->gev[2 * i + 1]));
            c->g_st.refine_ms += f;
        }
        c->g_slot = slot;
        done += k;
        if (g.stall == 2) {
            // the next generation reached the yield bound: hand it back unrun
            g.stall = 0;
            g.ncand = 4 * g.items;
            rc = set_state(c, slot, g, s);
            if (rc != DP_OK)
                return rc;
            break;
        }
        if (g.stall) {
            // the next generation outgrew the buffers: grow and resume it
            c->g_st.stalls += 1;
            cap = std::max<int64_t>(2 * cap, 4 * g.items + (c->gen_cap_test > 0 ? 0 : 4096));
            g.stall = 0;
            g.ncand = 4 * g.items;
            if (g.ncand > INT32_MAX)
                return fail(c, DP_E_OOM, "generation too large");
            rc = reserve_organizer(c, cap);
            if (rc != DP_OK || (rc = set_state(c, slot, g, s)) != DP_OK)
                return rc;
            if (done >= max_gens)
                break;
            continue;
        }
        if (g.items == 0 || done >= max_gens)
            break;
    }
    *last = g;
    return DP_OK;
}

// the seed state: generation 0 over n seed patches (sequence numbers 0 .. n-1)
static dpk::GenDev seed_state(int64_t n)
{
    dpk::GenDev g{};
    g.items = n;
    g.ncand = n;
    g.nseeds = n;
    g.per_item = 1;
    return g;
}

static int begin_impl(dp_ctx *c, int n, hipStream_t s)
{
    c->g_t0 = std::chrono::steady_clock::now();
    c->g_st = dp_densify_stats{};
    c->g_st.seeds_in = n;
    c->g_np = 0;
    c->g_nseeds = n;
    c->g_time_pending = false;
    c->part_pending = false;
    c->g_slot = 0;
    c->result.clear();
    int rc = reset_grid(c, s);
    if (rc != DP_OK || (rc = reserve_organizer(c, std::max<int64_t>(n, 1))) != DP_OK)
        return rc;
    DP_HIP(c, c->store.reserve((size_t)store_capacity(c, n)));
    DP_HIP(c, hipMemsetAsync(c->d_evals.p, 0, sizeof(unsigned long long), s));
    DP_HIP(c, hipMemsetAsync(c->mbox.p, 0, 8 * sizeof(unsigned long long), s));
    return set_state(c, 0, seed_state(n), s);
}

static int result_impl(dp_ctx *c, hipStream_t s, const dp_patch **out, int64_t *n_out, dp_densify_stats *stats)
{
    const int64_t np = c->g_np;
    DP_HIP(c, c->result.resize((size_t)np));
    if (np)
        DP_HIP(c, hipMemcpyAsync(c->result.data(), c->store.p, sizeof(dp_patch) * np, hipMemcpyDeviceToHost, s));
    unsigned long long ev = 0;
    DP_HIP(c, hipMemcpyAsync(&ev, c->d_evals.p, sizeof(ev), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    dp_densify_stats st = c->g_st;
    st.patches = np;
    st.pops = std::min<int64_t>(np, c->opt.max_pops);
    st.evals = (int64_t)ev;
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->g_t0).count();
    if (stats)
        *stats = st;
    *out = c->result.empty() ? nullptr : c->result.data();
    *n_out = np;
    return DP_OK;
}

// every expansion generation from the state in c->g_slot to the end of the
// BFS: device-resident (run_generations), or one host wait per generation for
// the analytic-gradient refine.  known: the state in c->g_slot when the
// caller has just read it (saves that loop's first status read)
static int expand_all(dp_ctx *c, int64_t cap, hipStream_t s, dpk::GenDev *last, const dpk::GenDev *known = nullptr)
{
    if (device_loop_ok(c))
        return run_generations(c, INT64_MAX, cap, s, last);
    const dp_options &o = c->opt;
    dpk::GenDev g{};
    unsigned long long mb[8];
    int rc = DP_OK;
    if (known)
        g = *known;
    else
        rc = read_state(c, c->g_slot, s, &g, mb);
    while (rc == DP_OK && g.items > 0) {
        const int32_t nc = (int32_t)(4 * g.items);
        DP_HIP(c, c->cand.reserve(nc));
        DP_HIP(c, c->ok.reserve(nc));
        if ((rc = reserve_organizer(c, nc)) != DP_OK)
            break;
        rc = take_refine_ms(c, &c->g_st.refine_ms);
        if (rc == DP_OK) {
            dpk::RefineJob job =
                densify_job(c, DP_MODE_EXPAND, c->cand.p, c->ok.p, nc, o.expand_cell_size, densify_epi(c));
            job.parent0 = g.head;
            job.seq0 = g.seq0;
            rc = launch_job(c, job, s);
        }
        c->g_time_pending = true;
        if (rc == DP_OK)
            rc = organize_gen(c, c->cand.p, c->ok.p, c->g_slot, INT64_MAX, s, densify_epi(c));
        if (rc == DP_OK)
            rc = read_state(c, c->g_slot ^ 1, s, &g, mb);
        c->g_slot ^= 1;
    }
    // the last generation's refine events (completed by its status read)
    if (rc == DP_OK)
        rc = take_refine_ms(c, &c->g_st.refine_ms);
    *last = g;
    return rc;
}

// dp_densify up to its result: the finished store stays on the device
static int densify_core(dp_ctx *c, const double *seeds, int n)
{
    hipStream_t s = c->stream;
    const dp_options &o = c->opt;
    // every buffer of the first expansion generation (<= 4 per seed patch)
    // before anything is queued on them
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(4 * (int64_t)n, 1024), INT32_MAX);
    DP_HIP(c, c->cand.reserve((size_t)cap));
    DP_HIP(c, c->ok.reserve((size_t)cap));
    int rc = begin_impl(c, n, s);
    if (rc != DP_OK || (rc = reserve_organizer(c, cap)) != DP_OK || (rc = ensure_gen_events(c)) != DP_OK)
        return rc;
    c->g_expected = -1;
    if (n > 0) {
        rc = seeds_device(c, seeds, n, c->cand.p, s);
        if (rc != DP_OK)
            return rc;
        // seed.cpp:110-144: FilterPatches then OptimizePatches at the seed cell
        // size (performance mode, dp_fast_options.densify: the fast refine),
        // timed by its own event pair (the generations' are re-recorded)
        DP_HIP(c, hipEventRecord(c->gev[2 * kGenBatch], s));
        rc = launch_job(c, densify_job(c, DP_MODE_SEED, c->cand.p, c->ok.p, n, o.seed_cell_size, densify_epi(c)), s);
        if (rc != DP_OK)
            return rc;
        DP_HIP(c, hipEventRecord(c->gev[2 * kGenBatch + 1], s));
        // PatchOrganizer::SetSeeds: TryInsert in seed order (seq = seed index)
        c->g_lpt_scratch = nullptr;
        rc = organize_gen(c, c->cand.p, c->ok.p, 0, cap, s, densify_epi(c));
        if (rc != DP_OK)
            return rc;
        c->g_slot = 1;
        dpk::GenDev g{};
        rc = expand_all(c, cap, s, &g);
        if (rc != DP_OK)
            return rc;
        float f = 0.f;
        DP_HIP(c, hipEventElapsedTime(&f, c->gev[2 * kGenBatch], c->gev[2 * kGenBatch + 1]));
        c->g_st.refine_ms += f;
        take_state(c, g, nullptr);
    }
    return DP_OK;
}

extern "C" int dp_densify(dp_ctx *c, const double *seeds, int n, const dp_patch **out, int64_t *n_out,
                          dp_densify_stats *stats)
{
    if (!c || n < 0 || (n > 0 && !seeds) || !out || !n_out)
        return fail(c, DP_E_ARG, "dp_densify: bad arguments");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_densify: no views");
    hipSetDevice(c->device);
    *out = nullptr;
    *n_out = 0;
    const int rc = densify_core(c, seeds, n);
    if (rc != DP_OK)
        return rc;
    return result_impl(c, c->stream, out, n_out, stats);
}

// ---------------------------------------------------------------------------
// densify one generation at a time (multi-GPU sharding).  Same
// sequence numbering, organizer and pop cap as dp_densify.
// ---------------------------------------------------------------------------

extern "C" int dp_densify_begin(dp_ctx *c, const double *seeds, int n, dp_generation *gen)
{
    if (!c || n < 0 || (n > 0 && !seeds) || !gen)
        return fail(c, DP_E_ARG, "dp_densify_begin: bad arguments");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_densify_begin: no views");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    int rc = begin_impl(c, n, s);
    if (rc != DP_OK)
        return rc;
    if (n > 0) {
        DP_HIP(c, c->seedp.reserve(n));
        rc = seeds_device(c, seeds, n, c->seedp.p, s);
        if (rc != DP_OK)
            return rc;
    }
    DP_HIP(c, hipStreamSynchronize(s));
    *gen = dp_generation{};
    gen->items = n;
    gen->per_item = 1;
    gen->cell = c->opt.seed_cell_size;
    gen->index = 0;
    c->g_expected = 0;
    return DP_OK;
}

static int check_gen(dp_ctx *c, const dp_generation *gen, const char *who)
{
    if (!c || !gen)
        return fail(c, DP_E_ARG, std::string(who) + ": bad arguments");
    if (gen->index != c->g_expected)
        return fail(c, DP_E_STATE, std::string(who) + ": generation out of sequence");
    return DP_OK;
}

// The organizer step of a whole generation on stream s (cp/op: every
// candidate in sequence order, ordered before it on s), ending in the
// generation's one status read; advances *gen.
static int commit_on_stream(dp_ctx *c, dp_generation *gen, const dp_patch *cp, const uint8_t *op, int64_t nc,
                            hipStream_t s, int64_t *exchanged = nullptr, int fused = 0)
{
    int rc = reserve_organizer(c, std::max<int64_t>(nc, 1));
    if (rc != DP_OK)
        return rc;
    c->g_lpt_scratch = nullptr;
    // host-driven generations size their refines on the host: no stall bound
    rc = organize_gen(c, cp, op, c->g_slot, INT64_MAX, s, fused);
    dpk::GenDev g{};
    unsigned long long mb[8];
    if (rc != DP_OK || (rc = read_state(c, c->g_slot ^ 1, s, &g, mb)) != DP_OK ||
        (rc = take_refine_ms(c, &c->g_st.refine_ms)) != DP_OK)
        return rc;
    c->g_slot ^= 1;
    if (exchanged)
        *exchanged = (int64_t)mb[4];
    take_state(c, g, gen);
    return DP_OK;
}

extern "C" int dp_densify_commit(dp_ctx *c, dp_generation *gen, const dp_patch *cand, const uint8_t *accept,
                                 int64_t n_cand)
{
    int rc = check_gen(c, gen, "dp_densify_commit");
    if (rc != DP_OK)
        return rc;
    if (n_cand != gen->items * gen->per_item || (n_cand > 0 && (!cand || !accept)))
        return fail(c, DP_E_ARG, "dp_densify_commit: need all candidates of the generation");
    if (n_cand > INT32_MAX)
        return fail(c, DP_E_OOM, "dp_densify_commit: generation too large");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    if (n_cand > 0) {
        DP_HIP(c, c->cand.reserve((size_t)n_cand));
        DP_HIP(c, c->ok.reserve((size_t)n_cand));
        DP_HIP(c, hipMemcpyAsync(c->cand.p, cand, sizeof(dp_patch) * n_cand, hipMemcpyHostToDevice, s));
        DP_HIP(c, hipMemcpyAsync(c->ok.p, accept, (size_t)n_cand, hipMemcpyHostToDevice, s));
    }
    return commit_on_stream(c, gen, c->cand.p, c->ok.p, n_cand, s);
}

extern "C" int dp_densify_run_until(dp_ctx *c, dp_generation *gen, int32_t max_generations, int64_t yield_items,
                                    int64_t *evals_out)
{
    int rc = check_gen(c, gen, "dp_densify_run");
    if (rc != DP_OK)
        return rc;
    if (gen->index < 1 || max_generations < 1 || yield_items < 0)
        return fail(c, DP_E_ARG,
                    "dp_densify_run: expansion generations only (index >= 1), max_generations >= 1, yield_items >= 0");
    if (evals_out)
        *evals_out = 0;
    if (gen->items == 0)
        return DP_OK;
    if (!device_loop_ok(c))
        return fail(c, DP_E_ARG, "dp_densify_run: the analytic-gradient refine is host-driven");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // the evaluation counter before this call's refines (read after its waits)
    unsigned long long ev[2] = {0, 0};
    if (evals_out)
        DP_HIP(c, hipMemcpyAsync(&ev[0], c->d_evals.p, sizeof(ev[0]), hipMemcpyDeviceToHost, s));
    dpk::GenDev g{};
    rc = run_generations(c, max_generations, std::max<int64_t>(4 * gen->items + 4096, (int64_t)c->cand.cap), s, &g,
                         yield_items);
    if (rc != DP_OK)
        return rc;
    take_state(c, g, gen);
    if (evals_out) {
        DP_HIP(c, hipMemcpyAsync(&ev[1], c->d_evals.p, sizeof(ev[1]), hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipStreamSynchronize(s));
        *evals_out = (int64_t)(ev[1] - ev[0]);
    }
    return DP_OK;
}

extern "C" int dp_densify_run(dp_ctx *c, dp_generation *gen, int32_t max_generations)
{
    return dp_densify_run_until(c, gen, max_generations, 0, nullptr);
}

// ---- partitioned generations (reference-view super-tiles) -------

// The partition of a generation (spec in include/densepoints.h):
// items stable-sorted by super-tile key, the order cut into `world` contiguous
// shares lo[r] = floor(r n / world).  Leaves the order in c->porder, the shares
// in counts (host) and the statistics in the status words (mbox[2..3]; read
// back here when sync, else with the commit's status).
static int partition_impl(dp_ctx *c, const dp_generation *gen, int world, int tile_px, int64_t *counts,
                          hipStream_t s, bool sync)
{
    const int64_t n = gen->items;
    for (int r = 0; r < world; ++r)
        counts[r] = (int64_t)(((__int128)(r + 1) * n) / world - ((__int128)r * n) / world);
    c->part_stats[0] = n;
    c->part_stats[1] = world;
    c->part_stats[2] = c->part_stats[3] = 0;
    if (n == 0)
        return DP_OK;
    if (n > INT32_MAX)
        return fail(c, DP_E_OOM, "partition: generation too large");
    // s is used as given: NULL is the legacy default stream (the async entry
    // point's caller stream), never replaced by the context's stream
    const dp_patch *items = gen->index == 0 ? c->seedp.p : c->store.p + gen->head;
    DP_HIP(c, c->tkeys.reserve((size_t)n));
    DP_HIP(c, c->okeys.reserve((size_t)n));
    DP_HIP(c, c->oiota.reserve((size_t)n));
    DP_HIP(c, c->porder.reserve((size_t)n));
    unsigned long long *stats = c->mbox.p + 2;
    // the dense key's range: tile rows / columns of the largest view, clamped
    // to [-1, TY] x [-1, TX]; the sort covers only the bits that range needs
    int64_t wmax = 1, hmax = 1;
    for (const auto &v : c->hv) {
        wmax = std::max<int64_t>(wmax, v.W);
        hmax = std::max<int64_t>(hmax, v.H);
    }
    const int64_t tx_max = (wmax + tile_px - 1) / tile_px, ty_max = (hmax + tile_px - 1) / tile_px;
    const unsigned __int128 kmax = (unsigned __int128)c->V * (unsigned __int128)(ty_max + 2) * (unsigned __int128)(tx_max + 2);
    int bits = 1;
    while (bits < 64 && ((unsigned __int128)1 << bits) < kmax)
        ++bits;
    DP_HIP(c, dpk::launch_tile_keys(c->d_views, items, n, (double)tile_px, tx_max, ty_max, c->tkeys.p, c->oiota.p, stats,
                                    s));
    size_t tmp = 0;
    DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, c->tkeys.p, c->okeys.p, c->oiota.p, c->porder.p, (int)n,
                                                 0, bits, s));
    DP_HIP(c, c->scan_tmp.reserve(tmp + 16));
    DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, tmp, c->tkeys.p, c->okeys.p, c->oiota.p, c->porder.p,
                                                 (int)n, 0, bits, s));
    DP_HIP(c, dpk::launch_partition_stats(c->okeys.p, n, world, stats, s));
    if (!sync) {
        c->part_pending = true;
        return DP_OK;
    }
    unsigned long long st[2] = {0, 0};
    DP_HIP(c, hipMemcpyAsync(st, stats, sizeof(st), hipMemcpyDeviceToHost, s));
    // the order is read on the caller's stream (refine, compaction): complete it
    DP_HIP(c, hipStreamSynchronize(s));
    c->part_stats[2] = (int64_t)st[0];
    c->part_stats[3] = (int64_t)st[1];
    return DP_OK;
}

extern "C" int dp_densify_owners(dp_ctx *c, const dp_generation *gen, int world, int tile_px, int32_t *owner_out,
                                 int32_t *fallback_out)
{
    if (!c || !gen || world < 1 || world > 64 || tile_px < 1 || (gen->items > 0 && !owner_out))
        return fail(c, DP_E_ARG, "dp_densify_owners: bad arguments (1 <= world <= 64)");
    if (gen->index != c->g_expected)
        return fail(c, DP_E_STATE, "dp_densify_owners: generation out of sequence");
    const int64_t n = gen->items;
    if (fallback_out)
        *fallback_out = 0;
    hipSetDevice(c->device);
    std::vector<int64_t> counts((size_t)world);
    int rc = partition_impl(c, gen, world, tile_px, counts.data(), c->stream, true);
    if (rc != DP_OK || n == 0)
        return rc;
    std::vector<int64_t> order((size_t)n);
    DP_HIP(c, hipMemcpy(order.data(), c->porder.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    int64_t j = 0;
    for (int r = 0; r < world; ++r)
        for (int64_t k = 0; k < counts[r]; ++k, ++j)
            owner_out[order[(size_t)j]] = r;
    return DP_OK;
}

extern "C" int dp_densify_partition_stats(dp_ctx *c, int64_t *stats_out)
{
    if (!c || !stats_out)
        return fail(c, DP_E_ARG, "dp_densify_partition_stats: bad arguments");
    for (int k = 0; k < 4; ++k)
        stats_out[k] = c->part_stats[k];
    return DP_OK;
}

// refine of the items d_items[0..n) of the generation into work / okp on s
// (seed patches by index in generation 0; Expand::ExpandPatch of the queue
// entries head + items[k] otherwise)
static int densify_refine_items_impl(dp_ctx *c, const dp_generation *gen, const int64_t *d_items, int64_t n,
                                     dp_patch *work, uint8_t *okp, hipStream_t s, int epi = 0)
{
    const int64_t nc64 = n * gen->per_item;
    if (nc64 > INT32_MAX)
        return fail(c, DP_E_OOM, "dp_densify_refine_items: shard too large");
    const int32_t nc = (int32_t)nc64;
    int rc = take_refine_ms(c, &c->g_st.refine_ms); // an earlier refine's events, before they are re-recorded
    if (rc != DP_OK)
        return rc;
    if (gen->index == 0) {
        DP_HIP(c, dpk::launch_gather_patches(c->seedp.p, d_items, n, work, s));
        rc = launch_job(c, densify_job(c, DP_MODE_SEED, work, okp, nc, gen->cell, epi), s);
    } else {
        dpk::RefineJob job = densify_job(c, DP_MODE_EXPAND, work, okp, nc, gen->cell, epi);
        job.parent0 = gen->head;
        job.items = d_items;
        rc = launch_job(c, job, s);
    }
    if (rc != DP_OK)
        return rc;
    c->g_time_pending = true; // read at the commit's status sync
    return DP_OK;
}

extern "C" int dp_densify_refine_items(dp_ctx *c, const dp_generation *gen, const int64_t *items, int64_t n,
                                       dp_patch *cand_out, uint8_t *accept_out)
{
    int rc = check_gen(c, gen, "dp_densify_refine_items");
    if (rc != DP_OK)
        return rc;
    if (n < 0 || n > gen->items)
        return fail(c, DP_E_ARG, "dp_densify_refine_items: bad item count");
    if (n == 0)
        return DP_OK;
    if (!items || !cand_out || !accept_out)
        return fail(c, DP_E_ARG, "dp_densify_refine_items: null arrays");
    for (int64_t i = 0; i < n; ++i)
        if (items[i] < 0 || items[i] >= gen->items)
            return fail(c, DP_E_ARG, "dp_densify_refine_items: item out of range");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const size_t nc = (size_t)n * gen->per_item;
    DP_HIP(c, c->items.reserve((size_t)n));
    DP_HIP(c, c->wcand.reserve(nc));
    DP_HIP(c, c->wok.reserve(nc));
    DP_HIP(c, hipMemcpyAsync(c->items.p, items, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    rc = densify_refine_items_impl(c, gen, c->items.p, n, c->wcand.p, c->wok.p, s);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipMemcpyAsync(cand_out, c->wcand.p, sizeof(dp_patch) * nc, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(accept_out, c->wok.p, nc, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}

// ---- the one-wait device protocol (r05, slots r06) ---------------------------
// partition -> refine of the rank's share + compaction into its slot ->
// [all-gather of the slots] -> commit, all queued on the caller's stream; the
// only host wait is the commit's status read.

extern "C" int dp_densify_partition_async(dp_ctx *c, const dp_generation *gen, int world, int tile_px, void *stream,
                                          const int64_t **d_order_out, int64_t *counts_out)
{
    if (!c || !gen || world < 1 || world > 64 || tile_px < 1 || !d_order_out || !counts_out)
        return fail(c, DP_E_ARG, "dp_densify_partition_async: bad arguments (1 <= world <= 64)");
    if (gen->index != c->g_expected)
        return fail(c, DP_E_STATE, "dp_densify_partition_async: generation out of sequence");
    *d_order_out = nullptr;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream; // the caller's stream (NULL: the legacy default stream)
    // the library's own earlier work (begin's seed patches) precedes the keys
    int rc = join_streams(c, c->stream, s);
    if (rc == DP_OK)
        rc = partition_impl(c, gen, world, tile_px, counts_out, s, false);
    if (rc != DP_OK)
        return rc;
    if (gen->items > 0)
        *d_order_out = c->porder.p;
    return DP_OK;
}

extern "C" int dp_densify_refine_share_async(dp_ctx *c, const dp_generation *gen, const int64_t *d_items, int64_t n,
                                             dp_patch *d_slot, int64_t stride, void *stream)
{
    int rc = check_gen(c, gen, "dp_densify_refine_share_async");
    if (rc != DP_OK)
        return rc;
    if (n < 0 || n > gen->items || !d_slot || stride < n * gen->per_item || (n > 0 && !d_items))
        return fail(c, DP_E_ARG, "dp_densify_refine_share_async: bad arguments (stride >= n * per_item)");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream; // the caller's stream (NULL: the legacy default stream)
    const size_t nc = (size_t)n * gen->per_item;
    if (nc > 0) {
        DP_HIP(c, c->wcand.reserve(nc));
        DP_HIP(c, c->wok.reserve(nc));
        // the owner colours its accepted candidates (Patch::ComputeColor off the
        // replicated commit); claims stay with the commit, which sees every rank's
        rc = densify_refine_items_impl(c, gen, d_items, n, c->wcand.p, c->wok.p, s, dpk::kEpiColor);
        if (rc != DP_OK)
            return rc;
    }
    DP_HIP(c, dpk::launch_compact_slot(c->wcand.p, c->wok.p, d_items, n, gen->per_item, d_slot, s));
    return DP_OK;
}

extern "C" int dp_densify_commit_gathered_device(dp_ctx *c, dp_generation *gen, const dp_patch *d_recs, int64_t stride,
                                                 int world, void *stream, int64_t *exchanged_out)
{
    int rc = check_gen(c, gen, "dp_densify_commit_gathered_device");
    if (rc != DP_OK)
        return rc;
    if (world < 1 || world > 64 || stride < 0 || !d_recs)
        return fail(c, DP_E_ARG, "dp_densify_commit_gathered_device: bad arguments");
    const int64_t nc = gen->items * gen->per_item;
    if (nc > INT32_MAX)
        return fail(c, DP_E_OOM, "dp_densify_commit_gathered_device: generation too large");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream; // the caller's stream (NULL: the legacy default stream)
    DP_HIP(c, c->cand.reserve((size_t)std::max<int64_t>(nc, 1)));
    DP_HIP(c, c->ok.reserve((size_t)std::max<int64_t>(nc, 1)));
    if (nc > 0) {
        // every other candidate of the generation failed the refine's filter
        DP_HIP(c, hipMemsetAsync(c->ok.p, 0, (size_t)nc, s));
    }
    // capacity 1: the scatter claims the records' cells as it places them
    const bool claims = c->opt.max_patches_per_cell == 1;
    DP_HIP(c, c->gstate.reserve(2));
    const dpk::ScatterClaims sc{c->d_views, claims ? c->grid.p : nullptr, (double)c->opt.grid_scale,
                                c->gstate.p + c->g_slot};
    DP_HIP(c, dpk::launch_scatter_slots(d_recs, stride, world, nc, c->cand.p, c->ok.p, c->mbox.p + 4, sc, s));
    int64_t ex = 0;
    // the slots' records were coloured by their owners' refines (dp_densify_refine_share_async)
    rc = commit_on_stream(c, gen, c->cand.p, c->ok.p, nc, s, &ex,
                          dpk::kEpiColor | (claims ? dpk::kEpiClaims : 0));
    if (rc == DP_OK && exchanged_out)
        *exchanged_out = ex;
    return rc;
}

extern "C" int dp_densify_result(dp_ctx *c, const dp_patch **out, int64_t *n_out, dp_densify_stats *stats)
{
    if (!c || !out || !n_out)
        return fail(c, DP_E_ARG, "dp_densify_result: bad arguments");
    if (c->g_expected < 0)
        return fail(c, DP_E_STATE, "dp_densify_result: no generation run");
    hipSetDevice(c->device);
    return result_impl(c, c->stream, out, n_out, stats);
}

// ---------------------------------------------------------------------------
// resume: the BFS restarted from an existing patch set (PatchOrganizer::
// SetSeeds, patch_organizer.cpp:70-75, on patches instead of refined seeds),
// and the expand-filter iteration built on it (PMVS alternates expansion and
// filtering; DESIGN.md "Iterated expand-filter").
// ---------------------------------------------------------------------------

// The offered patches are staged in c->cand with the keep flags as the
// organizer's accept flags c->ok (sequence number = index in the input, so the
// kept patches reach TryInsert in index order whatever the launch geometry),
// then a per_item = 1 generation is organized without a refine: claims,
// resolve, append (seq, parent, ACCEPTED, ComputeColor).  d_patches may be the
// context's own store: it is only read by the staging copy, which is ordered
// before the reset and the append on s; d_patches == c->cand.p / d_keep ==
// c->ok.p mean "already staged" (the host form).  One host wait: the status read.
static int resume_impl(dp_ctx *c, const dp_patch *d_patches, const uint8_t *d_keep, int64_t n, hipStream_t s,
                       dp_generation *gen, dpk::GenDev *state = nullptr)
{
    if (n > 0x7fffffffll)
        return fail(c, DP_E_OOM, "dp_densify_resume: too many patches");
    const size_t cap = (size_t)std::max<int64_t>(n, 1);
    // every buffer before anything is queued on it
    if (!d_patches || d_patches != c->cand.p)
        DP_HIP(c, c->cand.reserve(cap));
    if (!d_keep || d_keep != c->ok.p)
        DP_HIP(c, c->ok.reserve(cap));
    int rc = join_streams(c, c->stream, s);
    if (rc != DP_OK)
        return rc;
    if (n > 0) {
        if (d_patches != c->cand.p)
            DP_HIP(c, hipMemcpyAsync(c->cand.p, d_patches, sizeof(dp_patch) * (size_t)n, hipMemcpyDeviceToDevice, s));
        if (!d_keep)
            DP_HIP(c, hipMemsetAsync(c->ok.p, 1, (size_t)n, s));
        else if (d_keep != c->ok.p)
            DP_HIP(c, hipMemcpyAsync(c->ok.p, d_keep, (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    // a store that has to grow is freed by its reserve, and it may be the
    // source: the staging copy completes first (the only case with a second wait)
    if ((size_t)store_capacity(c, n) > c->store.cap)
        DP_HIP(c, hipStreamSynchronize(s));
    rc = begin_impl(c, (int)n, s);
    if (rc != DP_OK)
        return rc;
    c->g_expected = -1;
    c->g_lpt_scratch = nullptr;
    // host-sized follow-up (dp_densify_run reserves for the state it finds): no stall bound
    rc = organize_gen(c, c->cand.p, c->ok.p, 0, INT64_MAX, s, 0);
    dpk::GenDev g{};
    unsigned long long mb[8];
    if (rc != DP_OK || (rc = read_state(c, 1, s, &g, mb)) != DP_OK)
        return rc;
    c->g_slot = 1;
    take_state(c, g, gen);
    gen->seq0 = (uint32_t)n;
    if (state)
        *state = g;
    return DP_OK;
}

extern "C" int dp_densify_resume_device(dp_ctx *c, const dp_patch *d_patches, int64_t n, const uint8_t *d_keep,
                                        dp_generation *gen, void *stream)
{
    if (!c || n < 0 || (n > 0 && !d_patches) || !gen)
        return fail(c, DP_E_ARG, "dp_densify_resume_device: bad arguments");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_densify_resume_device: no views");
    hipSetDevice(c->device);
    return resume_impl(c, d_patches, d_keep, n, stream ? (hipStream_t)stream : c->stream, gen);
}

extern "C" int dp_densify_resume(dp_ctx *c, const dp_patch *patches, int64_t n, const uint8_t *keep, dp_generation *gen)
{
    if (!c || n < 0 || (n > 0 && !patches) || !gen)
        return fail(c, DP_E_ARG, "dp_densify_resume: bad arguments");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_densify_resume: no views");
    if (n > 0x7fffffffll)
        return fail(c, DP_E_OOM, "dp_densify_resume: too many patches");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const size_t cap = (size_t)std::max<int64_t>(n, 1);
    DP_HIP(c, c->cand.reserve(cap));
    DP_HIP(c, c->ok.reserve(cap));
    if (n > 0) {
        DP_HIP(c, hipMemcpyAsync(c->cand.p, patches, sizeof(dp_patch) * (size_t)n, hipMemcpyHostToDevice, s));
        if (keep)
            DP_HIP(c, hipMemcpyAsync(c->ok.p, keep, (size_t)n, hipMemcpyHostToDevice, s));
    }
    return resume_impl(c, c->cand.p, keep ? c->ok.p : nullptr, n, s, gen);
}

// dp_probe_keep_gather (densepoints_probe.h): the survivor compaction of
// dp_densify_iterate on host arrays
extern "C" int dp_probe_keep_gather(dp_ctx *c, const dp_patch *patches, int64_t n, const uint8_t *keep, dp_patch *out,
                                    int64_t *n_out)
{
    if (!c || n < 0 || n > 0x7fffffffll || (n > 0 && (!patches || !keep || !out)) || !n_out)
        return fail(c, DP_E_ARG, "dp_probe_keep_gather: bad arguments");
    *n_out = 0;
    if (n == 0)
        return DP_OK;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    DP_HIP(c, c->f_pat.reserve((size_t)n));
    DP_HIP(c, c->f_keep.reserve((size_t)n));
    DP_HIP(c, c->cand.reserve((size_t)n));
    DP_HIP(c, c->bsum.reserve(dpk::kBfsBlocks));
    DP_HIP(c, c->itw.reserve(2 * 16));
    DP_HIP(c, hipMemcpyAsync(c->f_pat.p, patches, sizeof(dp_patch) * (size_t)n, hipMemcpyHostToDevice, s));
    DP_HIP(c, hipMemcpyAsync(c->f_keep.p, keep, (size_t)n, hipMemcpyHostToDevice, s));
    DP_HIP(c, dpk::launch_keep_count(c->f_keep.p, n, c->bsum.p, c->itw.p, s));
    DP_HIP(c, dpk::launch_keep_gather(c->f_pat.p, c->f_keep.p, n, c->bsum.p, c->cand.p, (int64_t)c->cand.cap, s));
    unsigned long long kept = 0;
    DP_HIP(c, hipMemcpyAsync(&kept, c->itw.p, sizeof(kept), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    if (kept)
        DP_HIP(c, hipMemcpy(out, c->cand.p, sizeof(dp_patch) * (size_t)kept, hipMemcpyDeviceToHost));
    *n_out = (int64_t)kept;
    return DP_OK;
}

extern "C" int dp_densify_store_device(dp_ctx *c, const dp_patch **d_store, int64_t *n)
{
    if (!c || !d_store || !n)
        return fail(c, DP_E_ARG, "dp_densify_store_device: bad arguments");
    *d_store = c->g_np > 0 ? c->store.p : nullptr;
    *n = c->g_np;
    return DP_OK;
}

extern "C" int dp_densify_iterate(dp_ctx *c, const double *seeds, int n, int iterations, const dp_filter_options *fo,
                                  const dp_patch **out, int64_t *n_out, dp_densify_stats *stats,
                                  dp_iterate_stats *per_iter)
{
    if (!c || n < 0 || (n > 0 && !seeds) || !out || !n_out || iterations < 1 || iterations > 16)
        return fail(c, DP_E_ARG, "dp_densify_iterate: bad arguments (1 <= iterations <= 16)");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_densify_iterate: no views");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    *out = nullptr;
    *n_out = 0;
    dp_filter_options o;
    dp_default_filter_options(&o);
    if (fo)
        o = *fo;
    // per iteration two device words read once at the end: [2k] the objective
    // evaluations, [2k + 1] the filter's survivors
    DP_HIP(c, c->itw.reserve(2 * 16));
    if (c->fev.empty()) {
        c->fev.resize(2 * 16);
        for (auto &e : c->fev)
            DP_HIP(c, e.create());
    }
    std::vector<dp_iterate_stats> it((size_t)iterations, dp_iterate_stats{});
    dp_densify_stats tot{};
    tot.seeds_in = n;
    int64_t np = 0;
    auto tk = t0;
    for (int k = 0; k < iterations; ++k) {
        tk = std::chrono::steady_clock::now();
        int rc;
        if (k == 0) {
            rc = densify_core(c, seeds, n);
            it[0].offered = n;
        } else {
            // the previous store and its keep flags, both on the device
            dp_generation g{};
            dpk::GenDev first{};
            rc = resume_impl(c, c->store.p, c->f_keep.p, np, s, &g, &first);
            if (rc == DP_OK && g.items > 0) {
                dpk::GenDev last{};
                rc = expand_all(c, std::max<int64_t>(4 * g.items + 4096, (int64_t)c->cand.cap), s, &last, &first);
                if (rc == DP_OK)
                    take_state(c, last, nullptr);
            }
        }
        if (rc != DP_OK)
            return rc;
        c->g_expected = -1;
        np = c->g_np;
        dp_iterate_stats &st = it[(size_t)k];
        st.reinserted = c->g_st.seed_patches;
        st.patches = np;
        st.candidates = c->g_st.candidates;
        st.generations = c->g_st.generations;
        st.refine_ms = c->g_st.refine_ms;
        tot.pops += std::min<int64_t>(np, std::max<int64_t>(c->opt.max_pops, 0));
        tot.candidates += st.candidates;
        tot.generations += st.generations;
        tot.stalls += c->g_st.stalls;
        tot.refine_ms += st.refine_ms;
        if (k == 0)
            tot.seed_patches = st.reinserted;
        DP_HIP(c, c->f_keep.reserve((size_t)std::max<int64_t>(np, 1)));
        DP_HIP(c, c->bsum.reserve(dpk::kBfsBlocks));
        DP_HIP(c, hipMemcpyAsync(c->itw.p + 2 * k, c->d_evals.p, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
        DP_HIP(c, hipEventRecord(c->fev[2 * k], s));
        rc = dp_filter_patches_device(c, c->store.p, np, &o, c->f_keep.p, s);
        if (rc != DP_OK)
            return rc;
        if (np > 0)
            DP_HIP(c, dpk::launch_keep_count(c->f_keep.p, np, c->bsum.p, c->itw.p + 2 * k + 1, s));
        else
            DP_HIP(c, hipMemsetAsync(c->itw.p + 2 * k + 1, 0, sizeof(unsigned long long), s));
        DP_HIP(c, hipEventRecord(c->fev[2 * k + 1], s));
        st.total_ms = ms_since(tk); // host time: the filter's device time joins the next wait
    }
    // the last store's survivors, unchanged and in store order
    DP_HIP(c, c->cand.reserve((size_t)std::max<int64_t>(np, 1)));
    DP_HIP(c, dpk::launch_keep_gather(c->store.p, c->f_keep.p, np, c->bsum.p, c->cand.p, (int64_t)c->cand.cap, s));
    unsigned long long w[2 * 16];
    DP_HIP(c, hipMemcpyAsync(w, c->itw.p, sizeof(unsigned long long) * 2 * (size_t)iterations, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    const int64_t kept = (int64_t)w[2 * (iterations - 1) + 1];
    DP_HIP(c, c->result.resize((size_t)kept));
    if (kept)
        DP_HIP(c, hipMemcpyAsync(c->result.data(), c->cand.p, sizeof(dp_patch) * (size_t)kept, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    for (int k = 0; k < iterations; ++k) {
        dp_iterate_stats &st = it[(size_t)k];
        st.evals = (int64_t)w[2 * k];
        st.filtered_out = st.patches - (int64_t)w[2 * k + 1];
        if (k > 0)
            st.offered = (int64_t)w[2 * (k - 1) + 1];
        float f = 0.f;
        DP_HIP(c, hipEventElapsedTime(&f, c->fev[2 * k], c->fev[2 * k + 1]));
        st.filter_ms = f;
        tot.evals += st.evals;
    }
    it[(size_t)iterations - 1].total_ms = ms_since(tk); // with the result's copy
    tot.patches = kept;
    tot.total_ms = ms_since(t0);
    if (stats)
        *stats = tot;
    if (per_iter)
        std::copy(it.begin(), it.end(), per_iter);
    *out = c->result.empty() ? nullptr : c->result.data();
    *n_out = kept;
    return DP_OK;
}
