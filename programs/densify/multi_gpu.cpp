#include "multi_gpu.h"

#include "cli_error.h"
#include "dp_buf.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <thread>

namespace {

[[noreturn]] void fail(int rc, const std::string &detail) { throw CliError("multi-GPU densify", rc, detail); }

void hip_ok(hipError_t e, const char *what)
{
    if (e != hipSuccess)
        fail(DP_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

void nccl_ok(ncclResult_t r, const char *what)
{
    if (r != ncclSuccess)
        fail(DP_E_HIP, std::string(what) + ": " + ncclGetErrorString(r));
}

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream()
    {
        if (s)
            (void)hipStreamDestroy(s);
    }
};

struct Comm {
    ncclComm_t c = nullptr;
    Comm() = default;
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    ~Comm()
    {
        if (c)
            ncclCommDestroy(c);
    }
};

// One context's end of the exchange.  Teardown depends on the order of these
// members: ~Rank synchronises the stream, then they go in reverse -- the
// communicator, the buffers, the event, and the stream last.
struct Rank {
    int dev = 0;
    Stream stream;
    dpk::Event ready;                 // this context's slot is complete
    dpk::DevBuf<dp_patch> recv, slot; // slot: stride + 1 records; recv: G slots
    Comm comm;
    ~Rank()
    {
        // errors here have nowhere to go
        (void)hipSetDevice(dev);
        if (stream.s)
            (void)hipStreamSynchronize(stream.s);
    }
};

// The exchange of the device protocol between the contexts of this process:
// RCCL (ncclAllGather of the rank slots in one ncclGroup, over xGMI) when
// every context has its own device, else device-to-device peer copies (the
// contexts share a GPU, as on a one-GPU box).
struct Exchange {
    bool rccl = false;
    std::vector<Rank> ranks;

    Exchange(const std::vector<int> &devices, const std::string &mode) : ranks(devices.size())
    {
        std::vector<int> sorted(devices);
        std::sort(sorted.begin(), sorted.end());
        const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
        rccl = mode == "rccl" || (mode == "auto" && distinct);
        if (rccl && !distinct)
            fail(DP_E_HIP, "--exchange rccl needs one device per context");
        for (size_t g = 0; g < ranks.size(); ++g) {
            Rank &r = ranks[g];
            r.dev = devices[g];
            hip_ok(hipSetDevice(r.dev), "hipSetDevice");
            hip_ok(hipStreamCreateWithFlags(&r.stream.s, hipStreamNonBlocking), "hipStreamCreate");
            hip_ok(r.ready.create(hipEventDisableTiming), "hipEventCreate");
        }
        if (rccl) {
            std::vector<ncclComm_t> comms(ranks.size(), nullptr);
            nccl_ok(ncclCommInitAll(comms.data(), (int)ranks.size(), devices.data()), "ncclCommInitAll");
            for (size_t g = 0; g < ranks.size(); ++g)
                ranks[g].comm.c = comms[g];
        }
    }
    void reserve(int64_t stride)
    {
        const size_t need = (size_t)stride + 1;
        for (Rank &r : ranks) {
            hip_ok(hipSetDevice(r.dev), "hipSetDevice"); // DevBuf allocates on the current device
            hip_ok(r.slot.reserve(need), "hipMalloc");
            hip_ok(r.recv.reserve(need * ranks.size()), "hipMalloc");
        }
    }
    // every context's slot into every context's recv, rank order (queued on
    // the contexts' streams after their compaction: no host wait)
    void all_gather(int64_t stride)
    {
        const size_t bytes = ((size_t)stride + 1) * sizeof(dp_patch);
        if (rccl) {
            ncclGroupStart();
            for (Rank &r : ranks) {
                const ncclResult_t e = ncclAllGather(r.slot.p, r.recv.p, bytes, ncclUint8, r.comm.c, r.stream.s);
                if (e != ncclSuccess) {
                    ncclGroupEnd();
                    nccl_ok(e, "ncclAllGather");
                }
            }
            nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
            return;
        }
        for (Rank &r : ranks) {
            hip_ok(hipSetDevice(r.dev), "hipSetDevice");
            hip_ok(hipEventRecord(r.ready, r.stream.s), "hipEventRecord");
        }
        for (Rank &r : ranks) {
            hip_ok(hipSetDevice(r.dev), "hipSetDevice");
            for (size_t q = 0; q < ranks.size(); ++q) {
                hip_ok(hipStreamWaitEvent(r.stream.s, ranks[q].ready, 0), "hipStreamWaitEvent");
                hip_ok(hipMemcpyPeerAsync((char *)r.recv.p + q * bytes, r.dev, ranks[q].slot.p, ranks[q].dev, bytes,
                                          r.stream.s),
                       "hipMemcpyPeerAsync");
            }
        }
    }
};

// f(g) for every g < G at once, each in its own host thread so the waits
// overlap.  Returns the lowest g whose f returned other than DP_OK, with that
// code in `rc`; -1 when none did.
template <typename F> int on_every_context(int G, F f, int &rc)
{
    std::vector<int> rcs((size_t)G, DP_OK);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g)
        th.emplace_back([&rcs, &f, g]() { rcs[(size_t)g] = f(g); });
    for (auto &t : th)
        t.join();
    for (int g = 0; g < G; ++g)
        if (rcs[(size_t)g] != DP_OK)
            return rc = rcs[(size_t)g], g;
    return -1;
}

struct MultiRun {
    const MultiInput &in;
    const int G;
    Exchange ex;
    std::vector<dpk::DevBuf<uint8_t>> keep; // per-context keep flags of the rounds' filters
    std::vector<dp_generation> gen;
    std::vector<int64_t> repl_evals; // of the round: evaluations of replicated generations
    DensifyResult out;

    explicit MultiRun(const MultiInput &i)
        : in(i), G((int)i.ctxs.size()), ex(i.devices, i.exchange_mode), keep((size_t)G), gen((size_t)G),
          repl_evals((size_t)G, 0)
    {
        out.rounds.assign((size_t)in.iterations, dp_iterate_stats{});
        out.exchanged = 0;
    }
    dp_ctx *ctx(int g) const { return in.ctxs[(size_t)g]; }
    hipStream_t stream(int g) { return ex.ranks[(size_t)g].stream.s; }
    // a library call on context g
    void ok(int g, int rc)
    {
        if (rc != DP_OK)
            fail(rc, dp_last_error(ctx(g)));
    }

    void begin(const std::vector<double> &seeds);
    void filter_and_resume(int round);
    void generations();
    void collect(int round);
};

// round 0 starts from the seeds
void MultiRun::begin(const std::vector<double> &seeds)
{
    const int n = (int)(seeds.size() / 3);
    for (int g = 0; g < G; ++g)
        ok(g, dp_densify_begin(ctx(g), seeds.data(), n, &gen[(size_t)g]));
    out.rounds[0].offered = n;
    out.stats.seeds_in = n;
}

// a later round: every context filters its replicated store and resumes from the survivors
void MultiRun::filter_and_resume(int round)
{
    for (int g = 0; g < G; ++g) {
        const dp_patch *d_store = nullptr;
        int64_t ns = 0;
        ok(g, dp_densify_store_device(ctx(g), &d_store, &ns));
        hip_ok(hipSetDevice(in.devices[(size_t)g]), "hipSetDevice"); // DevBuf allocates on the current device
        hip_ok(keep[(size_t)g].reserve((size_t)std::max<int64_t>(ns, 1)), "hipMalloc");
        uint8_t *d_keep = keep[(size_t)g].p;
        ok(g, dp_filter_patches_device(ctx(g), d_store, ns, &in.filter, d_keep, stream(g)));
        ok(g, dp_densify_resume_device(ctx(g), d_store, ns, d_keep, &gen[(size_t)g], stream(g)));
        if (g == 0) {
            // the flags (not the store) for the round's counts
            std::vector<uint8_t> hk((size_t)ns);
            if (ns > 0)
                hip_ok(hipMemcpy(hk.data(), d_keep, (size_t)ns, hipMemcpyDeviceToHost), "hipMemcpy");
            const int64_t kept = (int64_t)hk.size() - std::count(hk.begin(), hk.end(), 0);
            out.rounds[(size_t)round].offered = kept;
            out.rounds[(size_t)round - 1].filtered_out = ns - kept;
        }
    }
}

// every generation of the round that gen[] starts
void MultiRun::generations()
{
    std::vector<int64_t> counts((size_t)G), ex_g((size_t)G, 0);
    int rc = DP_OK;
    while (gen[0].items > 0) {
        const int per = gen[0].per_item;
        if (gen[0].index >= 1 && gen[0].items < in.replicate_below) {
            // the BFS's small generations (latency-bound refines) on every
            // context at once, device-resident, no exchange, until one reaches
            // the bound; their evaluations count once (context 0)
            const int bad = on_every_context(
                G,
                [&](int g) {
                    int64_t ev = 0;
                    const int r = dp_densify_run_until(ctx(g), &gen[(size_t)g], INT32_MAX, in.replicate_below, &ev);
                    repl_evals[(size_t)g] += ev;
                    return r;
                },
                rc);
            if (bad >= 0)
                ok(bad, rc);
            continue;
        }
        // the partition and each context's share, queued (no host wait)
        int64_t stride = 1;
        for (int g = 0; g < G; ++g) {
            const int64_t *d_order = nullptr;
            ok(g, dp_densify_partition_async(ctx(g), &gen[(size_t)g], G, 64, stream(g), &d_order, counts.data()));
            if (g == 0) {
                stride = std::max<int64_t>(*std::max_element(counts.begin(), counts.end()) * per, 1);
                ex.reserve(stride);
            }
            int64_t off = 0;
            for (int q = 0; q < g; ++q)
                off += counts[(size_t)q];
            ok(g, dp_densify_refine_share_async(ctx(g), &gen[(size_t)g], counts[(size_t)g] ? d_order + off : nullptr,
                                                counts[(size_t)g], ex.ranks[(size_t)g].slot.p, stride, stream(g)));
        }
        ex.all_gather(stride);
        const int bad = on_every_context(
            G,
            [&](int g) {
                return dp_densify_commit_gathered_device(ctx(g), &gen[(size_t)g], ex.ranks[(size_t)g].recv.p, stride, G,
                                                         stream(g), &ex_g[(size_t)g]);
            },
            rc);
        if (bad >= 0)
            ok(bad, rc);
        out.exchanged += ex_g[0];
    }
}

// the round's store read back (context 0's last, so its buffer is the one
// kept), its counts into rounds[round] and the running sums
void MultiRun::collect(int round)
{
    std::vector<dp_densify_stats> sts((size_t)G);
    const dp_patch *res = nullptr;
    int64_t np = 0;
    for (int g = G - 1; g >= 0; --g)
        ok(g, dp_densify_result(ctx(g), &res, &np, &sts[(size_t)g]));
    if (round == in.iterations - 1)
        out.owned.assign(res, res + np);
    dp_densify_stats r = sts[0];
    for (int g = 1; g < G; ++g) {
        r.evals += sts[(size_t)g].evals - repl_evals[(size_t)g];
        r.refine_ms = std::max(r.refine_ms, sts[(size_t)g].refine_ms);
    }
    dp_iterate_stats &is = out.rounds[(size_t)round];
    is.reinserted = r.seed_patches;
    is.patches = r.patches;
    is.candidates = r.candidates;
    is.evals = r.evals;
    is.generations = r.generations;
    is.refine_ms = r.refine_ms;
    is.total_ms = r.total_ms;
    dp_densify_stats &sum = out.stats;
    sum.pops += r.pops;
    sum.candidates += r.candidates;
    sum.evals += r.evals;
    sum.generations += r.generations;
    sum.stalls += r.stalls;
    sum.refine_ms += r.refine_ms;
    sum.total_ms += r.total_ms;
    if (round == 0)
        sum.seed_patches = r.seed_patches;
    sum.patches = r.patches;
}

} // namespace

DensifyResult densify_multi(const MultiInput &in, const std::vector<double> &seeds)
{
    MultiRun run(in);
    for (int round = 0; round < in.iterations; ++round) {
        std::fill(run.repl_evals.begin(), run.repl_evals.end(), 0);
        if (round == 0)
            run.begin(seeds);
        else
            run.filter_and_resume(round);
        run.generations();
        run.collect(round);
    }
    run.out.patches = run.out.owned.data();
    run.out.n = (int64_t)run.out.owned.size();
    return std::move(run.out);
}
