// densify -- command-line front end of the MI355X patch loop.
//
// Mirrors the reference's programs/densify/main.cpp (-i scene.json, -s
// settings.json; PMVS::AddCamera per view, then PMVS::Run) and adds what
// SURVEY 8b asks of the build: -o out.ply (PMVS::PrintCloud format), --seeds
// (seed points from a file instead of Matcher::GenerateSeeds), --device,
// option overrides.  All compute goes through the C ABI of libdensepoints.so
// (include/densepoints.h): dp_set_views, dp_generate_seeds, dp_densify.
//
//   densify -i scene.json [--seeds seeds.xyz] [-s settings.json] [-o points.ply]
//           [--device N] [--max-pops N] [--level L] [--filter] [--iterations N] [--check-only]
//           [--features N] [--fast-threshold T] [--epipolar-matching] [--matcher knn|flann]
//           [--detector orb|akaze] [--akaze-threshold T]
//           [--depth-maps DIR [--splat-scale S] [--depth-normals]]
//           [--fuse FILE.ply [--fuse-min-views K] [--fuse-depth-tol T]]
//   densify --synthetic V,W,H,KIND --write-scene DIR   (deterministic test scene
//           written as scene.json + PPM images + seeds.xyz; no GPU needed)
#include "scene_io.h"

#include "../../include/densepoints.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <chrono>
#include <climits>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <algorithm>
#include <sys/stat.h>
#include <thread>
#include <vector>

namespace {

void usage()
{
    std::fprintf(stderr,
                 "usage: densify -i scene.json [--seeds seeds.xyz] [-s settings.json] [-o points.ply]\n"
                 "               [--device N] [--max-pops N] [--level L] [--filter] [--check-only]\n"
                 "               [--iterations N]  (1..16 rounds of expansion then filter, each round\n"
                 "                             re-expanding from the previous round's survivors with the\n"
                 "                             store resident on the device; N > 1 implies --filter)\n"
                 "               [--features N] [--fast-threshold T] [--epipolar-matching]\n"
                 "               [--matcher knn|flann]  (MatcherType, matcher.h:12)\n"
                 "               [--detector orb|akaze] [--akaze-threshold T]  (DetectorType, matcher.h:11)\n"
                 "               [--gpus N]   (one context per GPU, generations partitioned by\n"
                 "                             reference-view super-tile, accepted candidates\n"
                 "                             all-gathered device to device; output identical to 1 GPU)\n"
                 "               [--exchange auto|rccl|copy]  (auto: RCCL when every context has its\n"
                 "                             own GPU, else peer copies; --multi: that protocol at 1 GPU)\n"
                 "               [--replicate-below N]  (generations of fewer items run on every\n"
                 "                             context, device-resident, no exchange; default 1024 x gpus)\n"
                 "               [--mode parity|fast] [--fast-iters N] [--fast-gradient 0|1]\n"
                 "                            (fast: the performance-mode refine -- LDS-staged gray\n"
                 "                             tiles, fused CG -- for the seed stage and every expansion;\n"
                 "                             gradient 1: analytic, 0: forward differences)\n"
                 "               [--depth-maps DIR [--splat-scale S] [--depth-normals]]  (after the PLY:\n"
                 "                             DIR/depth_%%04d.pfm, and normal_%%04d.pfm, of every view --\n"
                 "                             the written patches as discs of radius S x rho, nearest\n"
                 "                             per pixel: dp_render_maps)\n"
                 "               [--fuse FILE.ply [--fuse-min-views K] [--fuse-depth-tol T]]  (after those:\n"
                 "                             the depth and normal maps of every view, rendered and fused\n"
                 "                             on the device into one cross-view-consistent cloud --\n"
                 "                             dp_fuse_maps; K = 0..63 agreeing other views, default 2;\n"
                 "                             T = relative depth tolerance, default 0.01)\n"
                 "       densify --synthetic V,W,H,KIND --write-scene DIR\n");
}

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

void write_ppm(const std::string &path, int w, int h, const std::vector<uint8_t> &bgr)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f)
        throw std::runtime_error("cannot write " + path);
    std::fprintf(f, "P6\n%d %d\n255\n", w, h);
    std::vector<uint8_t> rgb(bgr.size());
    for (size_t i = 0; i < bgr.size(); i += 3) {
        rgb[i] = bgr[i + 2];
        rgb[i + 1] = bgr[i + 1];
        rgb[i + 2] = bgr[i];
    }
    std::fwrite(rgb.data(), 1, rgb.size(), f);
    std::fclose(f);
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
        write_ppm(dir + "/" + name, cfg.width, cfg.height, bgr);
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
    std::printf("{\"scene\": \"%s/scene.json\", \"views\": %d, \"seeds\": %lld}\n", dir.c_str(), cfg.n_views,
                (long long)n);
    return 0;
}

// The exchange of the device protocol between the contexts of this process:
// RCCL (ncclAllGather of the rank slots in one ncclGroup, over xGMI) when
// every context has its own device, else device-to-device peer copies (the
// contexts share a GPU, as on a one-GPU box).
struct Exchange {
    int G = 0;
    bool rccl = false;
    std::vector<int> dev;
    std::vector<hipStream_t> stream;
    std::vector<hipEvent_t> ready; // each context's slot is complete
    std::vector<ncclComm_t> comm;
    std::vector<dp_patch *> slot, recv;
    std::vector<size_t> slot_cap, recv_cap; // records
    std::string err;

    bool hip(hipError_t e, const char *what)
    {
        if (e == hipSuccess)
            return true;
        err = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    }
    bool init(const std::vector<int> &devices, const char *mode)
    {
        G = (int)devices.size();
        dev = devices;
        std::vector<int> sorted(devices);
        std::sort(sorted.begin(), sorted.end());
        const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
        rccl = std::strcmp(mode, "rccl") == 0 || (std::strcmp(mode, "auto") == 0 && distinct);
        if (rccl && !distinct) {
            err = "--exchange rccl needs one device per context";
            return false;
        }
        stream.assign(G, nullptr);
        ready.assign(G, nullptr);
        slot.assign(G, nullptr);
        recv.assign(G, nullptr);
        slot_cap.assign(G, 0);
        recv_cap.assign(G, 0);
        for (int g = 0; g < G; ++g) {
            if (!hip(hipSetDevice(dev[g]), "hipSetDevice") ||
                !hip(hipStreamCreateWithFlags(&stream[g], hipStreamNonBlocking), "hipStreamCreate") ||
                !hip(hipEventCreateWithFlags(&ready[g], hipEventDisableTiming), "hipEventCreate"))
                return false;
        }
        if (rccl) {
            comm.assign(G, nullptr);
            const ncclResult_t r = ncclCommInitAll(comm.data(), G, dev.data());
            if (r != ncclSuccess) {
                err = std::string("ncclCommInitAll: ") + ncclGetErrorString(r);
                return false;
            }
        }
        return true;
    }
    // slot: stride + 1 records; recv: G slots
    bool reserve(int64_t stride)
    {
        const size_t need = (size_t)stride + 1;
        for (int g = 0; g < G; ++g) {
            if (!hip(hipSetDevice(dev[g]), "hipSetDevice"))
                return false;
            if (slot_cap[g] < need) {
                if (slot[g] && !hip(hipFree(slot[g]), "hipFree"))
                    return false;
                slot_cap[g] = need + need / 4;
                if (!hip(hipMalloc(&slot[g], slot_cap[g] * sizeof(dp_patch)), "hipMalloc"))
                    return false;
            }
            if (recv_cap[g] < need * G) {
                if (recv[g] && !hip(hipFree(recv[g]), "hipFree"))
                    return false;
                recv_cap[g] = (need + need / 4) * G;
                if (!hip(hipMalloc(&recv[g], recv_cap[g] * sizeof(dp_patch)), "hipMalloc"))
                    return false;
            }
        }
        return true;
    }
    // every context's slot into every context's recv, rank order (queued on
    // the contexts' streams after their compaction: no host wait)
    bool all_gather(int64_t stride)
    {
        const size_t bytes = ((size_t)stride + 1) * sizeof(dp_patch);
        if (rccl) {
            ncclGroupStart();
            for (int g = 0; g < G; ++g) {
                const ncclResult_t r = ncclAllGather(slot[g], recv[g], bytes, ncclUint8, comm[g], stream[g]);
                if (r != ncclSuccess) {
                    ncclGroupEnd();
                    err = std::string("ncclAllGather: ") + ncclGetErrorString(r);
                    return false;
                }
            }
            const ncclResult_t r = ncclGroupEnd();
            if (r != ncclSuccess) {
                err = std::string("ncclGroupEnd: ") + ncclGetErrorString(r);
                return false;
            }
            return true;
        }
        for (int g = 0; g < G; ++g)
            if (!hip(hipSetDevice(dev[g]), "hipSetDevice") || !hip(hipEventRecord(ready[g], stream[g]), "hipEventRecord"))
                return false;
        for (int g = 0; g < G; ++g) {
            if (!hip(hipSetDevice(dev[g]), "hipSetDevice"))
                return false;
            for (int q = 0; q < G; ++q) {
                if (!hip(hipStreamWaitEvent(stream[g], ready[q], 0), "hipStreamWaitEvent") ||
                    !hip(hipMemcpyPeerAsync((char *)recv[g] + (size_t)q * bytes, dev[g], slot[q], dev[q], bytes,
                                            stream[g]),
                         "hipMemcpyPeerAsync"))
                    return false;
            }
        }
        return true;
    }
    ~Exchange()
    {
        // teardown: errors here have nowhere to go
        for (int g = 0; g < G; ++g) {
            (void)hipSetDevice(dev[g]);
            if (stream[g])
                (void)hipStreamSynchronize(stream[g]);
            if (rccl && g < (int)comm.size() && comm[g])
                ncclCommDestroy(comm[g]);
            if (slot[g])
                (void)hipFree(slot[g]);
            if (recv[g])
                (void)hipFree(recv[g]);
            if (ready[g])
                (void)hipEventDestroy(ready[g]);
            if (stream[g])
                (void)hipStreamDestroy(stream[g]);
        }
    }
};

// dp_densify over `ctxs.size()` contexts (one per GPU), the device-resident
// protocol of include/densepoints.h with ONE host wait per generation per
// context: every generation's items are partitioned by reference-view
// super-tile on the device (dp_densify_partition_async; the shares are
// host-known floor cuts), each context refines its share and compacts the
// accepted candidates into its slot (dp_densify_refine_share_async), the slots
// are all-gathered device to device (Exchange: RCCL or peer copies), and every
// context commits the whole generation to its replicated organizer
// (dp_densify_commit_gathered_device, in its own host thread so the waits
// overlap) -- no candidate touches host memory, and the store equals
// dp_densify's bit for bit.  Expansion generations of fewer than
// replicate_below items run on every context device-resident instead
// (dp_densify_run_until: no partition, no exchange, eight per host wait).
// Returns the stats of context 0 (evals / refine_ms summed / maxed).
// iterations > 1 (--iterations): after each round but the last, every context
// filters its replicated store on the device (dp_filter_patches_device) and
// restarts the BFS from the survivors (dp_densify_resume_device on its own
// store): no exchange is added.  The caller filters the last round's store.
// The stats then sum over the rounds; iters[k] holds round k's counts (the
// last round's filtered_out is the caller's).  Every round's store is read
// back once for its statistics (dp_densify_result).
struct MultiRun {
    std::vector<dp_ctx *> &ctxs;
    const std::vector<int> &devices;
    Exchange &ex;
    int64_t replicate_below;
    std::string &err;
    std::vector<dp_generation> gen;
    std::vector<int64_t> repl_evals;
    int64_t exchanged = 0;

    int fail_of(int g, int rc)
    {
        err = dp_last_error(ctxs[(size_t)g]);
        return rc;
    }
    // every generation of the round that gen[] starts
    int generations();
};

int MultiRun::generations()
{
    const int G = (int)ctxs.size();
    std::vector<int> rcs((size_t)G, DP_OK);
    std::vector<int64_t> counts((size_t)G), ex_g((size_t)G, 0);
    while (gen[0].items > 0) {
        const int per = gen[0].per_item;
        if (gen[0].index >= 1 && gen[0].items < replicate_below) {
            // the BFS's small generations (latency-bound refines) on every
            // context at once, device-resident, no exchange, until one reaches
            // the bound; their evaluations count once (context 0)
            std::vector<std::thread> th;
            for (int g = 0; g < G; ++g)
                th.emplace_back([&, g]() {
                    int64_t ev = 0;
                    rcs[(size_t)g] = dp_densify_run_until(ctxs[(size_t)g], &gen[(size_t)g], INT32_MAX, replicate_below, &ev);
                    repl_evals[(size_t)g] += ev;
                });
            for (auto &t : th)
                t.join();
            for (int g = 0; g < G; ++g)
                if (rcs[(size_t)g] != DP_OK)
                    return fail_of(g, rcs[(size_t)g]);
            continue;
        }
        // the partition and each context's share, queued (no host wait)
        int64_t stride = 1;
        for (int g = 0; g < G; ++g) {
            const int64_t *d_order = nullptr;
            int rc = dp_densify_partition_async(ctxs[(size_t)g], &gen[(size_t)g], G, 64, ex.stream[(size_t)g], &d_order,
                                                counts.data());
            if (rc != DP_OK)
                return fail_of(g, rc);
            if (g == 0) {
                stride = std::max<int64_t>(*std::max_element(counts.begin(), counts.end()) * per, 1);
                if (!ex.reserve(stride)) {
                    err = ex.err;
                    return DP_E_HIP;
                }
            }
            int64_t off = 0;
            for (int q = 0; q < g; ++q)
                off += counts[(size_t)q];
            rc = dp_densify_refine_share_async(ctxs[(size_t)g], &gen[(size_t)g], counts[(size_t)g] ? d_order + off : nullptr,
                                               counts[(size_t)g], ex.slot[(size_t)g], stride, ex.stream[(size_t)g]);
            if (rc != DP_OK)
                return fail_of(g, rc);
        }
        if (!ex.all_gather(stride)) {
            err = ex.err;
            return DP_E_HIP;
        }
        std::vector<std::thread> th;
        for (int g = 0; g < G; ++g)
            th.emplace_back([&, g]() {
                rcs[(size_t)g] = dp_densify_commit_gathered_device(ctxs[(size_t)g], &gen[(size_t)g], ex.recv[(size_t)g],
                                                                   stride, G, ex.stream[(size_t)g], &ex_g[(size_t)g]);
            });
        for (auto &t : th)
            t.join();
        for (int g = 0; g < G; ++g)
            if (rcs[(size_t)g] != DP_OK)
                return fail_of(g, rcs[(size_t)g]);
        exchanged += ex_g[0];
    }
    return DP_OK;
}

int densify_multi(std::vector<dp_ctx *> &ctxs, const std::vector<int> &devices, const char *exchange_mode,
                  const std::vector<double> &seeds, std::vector<dp_patch> &out, dp_densify_stats &st,
                  std::string &err, int64_t &exchanged, int64_t replicate_below, int iterations,
                  const dp_filter_options &fopt, std::vector<dp_iterate_stats> &iters)
{
    const int G = (int)ctxs.size();
    const int n = (int)(seeds.size() / 3);
    Exchange ex;
    if (!ex.init(devices, exchange_mode)) {
        err = ex.err;
        return DP_E_HIP;
    }
    MultiRun run{ctxs, devices, ex, replicate_below, err, std::vector<dp_generation>((size_t)G),
                 std::vector<int64_t>((size_t)G, 0)};
    // per-context keep flags of the rounds' filters (device), grown as needed
    struct KeepBufs {
        std::vector<uint8_t *> p;
        std::vector<size_t> cap;
        std::vector<int> dev;
        ~KeepBufs()
        {
            for (size_t g = 0; g < p.size(); ++g)
                if (p[g]) {
                    (void)hipSetDevice(dev[g]);
                    (void)hipFree(p[g]);
                }
        }
    } keepb{std::vector<uint8_t *>((size_t)G, nullptr), std::vector<size_t>((size_t)G, 0), devices};
    iters.assign((size_t)iterations, dp_iterate_stats{});
    dp_densify_stats sum;
    std::memset(&sum, 0, sizeof sum);
    sum.seeds_in = n;
    for (int round = 0; round < iterations; ++round) {
        dp_iterate_stats &is = iters[(size_t)round];
        std::fill(run.repl_evals.begin(), run.repl_evals.end(), 0);
        if (round == 0) {
            for (int g = 0; g < G; ++g) {
                const int rc = dp_densify_begin(ctxs[(size_t)g], seeds.data(), n, &run.gen[(size_t)g]);
                if (rc != DP_OK)
                    return run.fail_of(g, rc);
            }
            is.offered = n;
        }
        for (int g = 0; round > 0 && g < G; ++g) {
            // every context filters its replicated store and resumes from the survivors
            const dp_patch *d_store = nullptr;
            int64_t ns = 0;
            int rc = dp_densify_store_device(ctxs[(size_t)g], &d_store, &ns);
            if (rc != DP_OK)
                return run.fail_of(g, rc);
            if (!ex.hip(hipSetDevice(devices[(size_t)g]), "hipSetDevice"))
                return err = ex.err, DP_E_HIP;
            const size_t need = (size_t)std::max<int64_t>(ns, 1);
            if (keepb.cap[(size_t)g] < need) {
                if (keepb.p[(size_t)g])
                    (void)hipFree(keepb.p[(size_t)g]);
                keepb.p[(size_t)g] = nullptr;
                keepb.cap[(size_t)g] = 0;
                if (!ex.hip(hipMalloc(&keepb.p[(size_t)g], need + need / 4), "hipMalloc"))
                    return err = ex.err, DP_E_HIP;
                keepb.cap[(size_t)g] = need + need / 4;
            }
            uint8_t *d_keep = keepb.p[(size_t)g];
            rc = dp_filter_patches_device(ctxs[(size_t)g], d_store, ns, &fopt, d_keep, ex.stream[(size_t)g]);
            if (rc == DP_OK)
                rc = dp_densify_resume_device(ctxs[(size_t)g], d_store, ns, d_keep, &run.gen[(size_t)g],
                                              ex.stream[(size_t)g]);
            if (rc != DP_OK)
                return run.fail_of(g, rc);
            if (g == 0) {
                // the flags (not the store) for the round's counts
                std::vector<uint8_t> hk((size_t)ns);
                if (ns > 0 && !ex.hip(hipMemcpy(hk.data(), d_keep, (size_t)ns, hipMemcpyDeviceToHost), "hipMemcpy"))
                    return err = ex.err, DP_E_HIP;
                int64_t kept = 0;
                for (uint8_t f : hk)
                    kept += f != 0;
                is.offered = kept;
                iters[(size_t)round - 1].filtered_out = ns - kept;
            }
        }
        const int grc = run.generations();
        if (grc != DP_OK)
            return grc;
        std::vector<dp_densify_stats> sts((size_t)G);
        const dp_patch *res = nullptr;
        int64_t np = 0;
        for (int g = G - 1; g >= 0; --g) {
            const int rc = dp_densify_result(ctxs[(size_t)g], &res, &np, &sts[(size_t)g]);
            if (rc != DP_OK)
                return run.fail_of(g, rc);
        }
        if (round == iterations - 1)
            out.assign(res, res + np);
        dp_densify_stats r = sts[0];
        for (int g = 1; g < G; ++g) {
            r.evals += sts[(size_t)g].evals - run.repl_evals[(size_t)g];
            r.refine_ms = std::max(r.refine_ms, sts[(size_t)g].refine_ms);
        }
        is.reinserted = r.seed_patches;
        is.patches = r.patches;
        is.candidates = r.candidates;
        is.evals = r.evals;
        is.generations = r.generations;
        is.refine_ms = r.refine_ms;
        is.total_ms = r.total_ms;
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
    exchanged = run.exchanged;
    st = sum;
    return DP_OK;
}

// little-endian PFM ("Pf" 1 channel, "PF" 3), rows bottom-up as the format requires
void write_pfm(const std::string &path, const float *px, int w, int h, int channels)
{
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f)
        throw std::runtime_error("cannot write " + path);
    std::fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", w, h);
    const size_t row = (size_t)w * (size_t)channels;
    bool ok = true;
    for (int y = h - 1; y >= 0 && ok; --y)
        ok = std::fwrite(px + (size_t)y * row, sizeof(float), row, f) == row;
    if (std::fclose(f) != 0 || !ok)
        throw std::runtime_error("short write to " + path);
}

} // namespace

int main(int argc, char **argv)
{
    std::string input, settings, output = "points.ply", seeds_path, synth, scene_dir, depth_dir, fuse_path;
    dp_fuse_options fuse_opt;
    dp_default_fuse_options(&fuse_opt);
    double splat_scale = 1.0;
    bool depth_normals = false;
    int device = 0, gpus = 1;
    bool force_multi = false;
    std::string exchange_mode = "auto";
    long long replicate_below = -1; // default 1024 x contexts
    long long max_pops = -1;
    int level = 0;
    bool check_only = false, do_filter = false, fast = false;
    int iterations = 1;
    int fast_iters = -1, fast_gradient = -1;
    dp_matcher_options mopt; // MatcherOptions defaults (matcher.h:21-32), ORB::create(40000)
    dp_default_matcher_options(&mopt);
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) {
                usage();
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "-i" || a == "--input") input = next();
        else if (a == "-s" || a == "--settings") settings = next();
        else if (a == "-o" || a == "--output") output = next();
        else if (a == "--seeds") seeds_path = next();
        else if (a == "--device") device = std::atoi(next().c_str());
        else if (a == "--gpus") gpus = std::atoi(next().c_str());
        else if (a == "--multi") force_multi = true;
        else if (a == "--replicate-below") replicate_below = std::atoll(next().c_str());
        else if (a == "--exchange") {
            exchange_mode = next();
            if (exchange_mode != "auto" && exchange_mode != "rccl" && exchange_mode != "copy") {
                std::fprintf(stderr, "densify: --exchange expects auto, rccl or copy\n");
                return 2;
            }
        }
        else if (a == "--max-pops") max_pops = std::atoll(next().c_str());
        else if (a == "--level") level = std::atoi(next().c_str());
        else if (a == "--filter") do_filter = true;
        else if (a == "--iterations") {
            iterations = std::atoi(next().c_str());
            if (iterations < 1 || iterations > 16) {
                std::fprintf(stderr, "densify: --iterations expects 1..16\n");
                return 2;
            }
        }
        else if (a == "--check-only") check_only = true;
        else if (a == "--features") mopt.n_features = std::atoi(next().c_str());
        else if (a == "--fast-threshold") mopt.fast_threshold = std::atoi(next().c_str());
        else if (a == "--epipolar-matching") mopt.epipolar_matching = 1;
        else if (a == "--matcher") {
            const std::string v = next();
            if (v == "knn")
                mopt.matcher_type = DP_MATCHER_KNN;
            else if (v == "flann")
                mopt.matcher_type = DP_MATCHER_FLANN;
            else {
                std::fprintf(stderr, "densify: --matcher expects knn or flann\n");
                return 2;
            }
        }
        else if (a == "--detector") {
            const std::string v = next();
            if (v == "orb")
                mopt.detector_type = DP_DETECTOR_ORB;
            else if (v == "akaze")
                mopt.detector_type = DP_DETECTOR_AKAZE;
            else {
                std::fprintf(stderr, "densify: --detector expects orb or akaze\n");
                return 2;
            }
        } else if (a == "--akaze-threshold") mopt.akaze_threshold = (float)std::atof(next().c_str());
        else if (a == "--mode") {
            const std::string m = next();
            if (m != "parity" && m != "fast") {
                usage();
                return 2;
            }
            fast = m == "fast";
        } else if (a == "--fast-iters") fast_iters = std::atoi(next().c_str());
        else if (a == "--fast-gradient") fast_gradient = std::atoi(next().c_str());
        else if (a == "--synthetic") synth = next();
        else if (a == "--write-scene") scene_dir = next();
        else if (a == "--depth-maps") depth_dir = next();
        else if (a == "--splat-scale") {
            splat_scale = std::atof(next().c_str());
            if (!(splat_scale > 0.0)) {
                std::fprintf(stderr, "densify: --splat-scale expects a positive number\n");
                return 2;
            }
        }
        else if (a == "--depth-normals") depth_normals = true;
        else if (a == "--fuse") fuse_path = next();
        else if (a == "--fuse-min-views") {
            char *end = nullptr;
            const std::string v = next();
            const long k = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || k < 0 || k > 63) {
                std::fprintf(stderr, "densify: --fuse-min-views expects 0..63\n");
                return 2;
            }
            fuse_opt.min_views = (int32_t)k;
        }
        else if (a == "--fuse-depth-tol") {
            char *end = nullptr;
            const std::string v = next();
            const double t = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(t >= 0.0) || !(t <= 3.0e38)) {
                std::fprintf(stderr, "densify: --fuse-depth-tol expects a finite number >= 0\n");
                return 2;
            }
            fuse_opt.depth_tol = (float)t;
        }
        else if (a == "-h" || a == "--help") {
            usage();
            return 0;
        } else {
            usage();
            return 2;
        }
    }
    if (iterations > 1)
        do_filter = true; // the filter is what tells the rounds apart
    try {
        if (!synth.empty()) {
            if (scene_dir.empty())
                throw std::runtime_error("--synthetic needs --write-scene DIR");
            return write_synthetic(synth, scene_dir);
        }
        if (input.empty()) {
            usage();
            return 2;
        }
        const auto t0 = std::chrono::steady_clock::now();
        dp_options opt;
        dp_default_options(&opt);
        if (!settings.empty())
            apply_settings(dpio::parse_json(dpio::read_file(settings)), opt);
        if (max_pops >= 0)
            opt.max_pops = max_pops;
        const dpio::Scene sc = dpio::read_scene(input);
        std::vector<dpio::Image> imgs;
        std::vector<double> P;
        for (const dpio::SceneView &v : sc.views) {
            imgs.push_back(dpio::load_image(v.filename)); // PMVS::AddCamera -> View::Load
            P.insert(P.end(), v.P, v.P + 12);
        }
        const std::vector<double> seeds = seeds_path.empty() ? std::vector<double>() : dpio::read_seeds(seeds_path);
        if (check_only) {
            // parsed scene summary + FNV-1a of each decoded BGR8 image (no GPU)
            std::printf("{\"views\": %zu, \"width\": %d, \"height\": %d, \"seeds\": %zu, \"image_fnv\": [",
                        imgs.size(), imgs.empty() ? 0 : imgs[0].width, imgs.empty() ? 0 : imgs[0].height,
                        seeds.size() / 3);
            for (size_t v = 0; v < imgs.size(); ++v) {
                uint64_t h = 1469598103934665603ull;
                for (uint8_t b : imgs[v].bgr)
                    h = (h ^ b) * 1099511628211ull;
                std::printf("%s\"%016llx\"", v ? ", " : "", (unsigned long long)h);
            }
            std::printf("]}\n");
            return 0;
        }
        std::vector<dp_image> dimg(imgs.size());
        for (size_t v = 0; v < imgs.size(); ++v)
            dimg[v] = dp_image{imgs[v].width, imgs[v].height, 3 * imgs[v].width, 0, imgs[v].bgr.data()};
        dp_ctx *ctx = nullptr;
        int rc = dp_ctx_create(&opt, device, &ctx);
        if (rc != DP_OK) {
            std::fprintf(stderr, "densify: dp_ctx_create failed (%d)\n", rc);
            return 1;
        }
        auto check = [&](int r, const char *what) {
            if (r != DP_OK) {
                std::fprintf(stderr, "densify: %s failed (%d): %s\n", what, r, dp_last_error(ctx));
                dp_ctx_destroy(ctx);
                std::exit(1);
            }
        };
        check(dp_set_views(ctx, (int)imgs.size(), P.data(), dimg.data()), "dp_set_views");
        // --mode fast: dp_fast_options.densify on every context
        dp_fast_options fo;
        dp_default_fast_options(&fo);
        fo.densify = fast ? 1 : 0;
        if (fast_iters >= 0)
            fo.iters = fast_iters;
        if (fast_gradient >= 0)
            fo.gradient = fast_gradient;
        check(dp_set_fast_options(ctx, &fo), "dp_set_fast_options");
        if (level > 0) {
            // run on pyramid level L (cv::pyrDown^L on the device, P rows 0-1 / 2^L)
            check(dp_build_pyramid(ctx, level + 1), "dp_build_pyramid");
            check(dp_set_level(ctx, level), "dp_set_level");
        }
        // PMVS::InsertSeeds (pmvs.cpp:29-34): without --seeds the seeds come from
        // Matcher::GenerateSeeds on the device (level-0 views)
        std::vector<double> gen_seeds;
        dp_seed_stats sst;
        std::memset(&sst, 0, sizeof sst);
        if (seeds_path.empty()) {
            const double *xyz = nullptr;
            int64_t n = 0;
            check(dp_generate_seeds(ctx, &mopt, &xyz, &n, &sst), "dp_generate_seeds");
            gen_seeds.assign(xyz, xyz + 3 * n);
        }
        const std::vector<double> &use = seeds_path.empty() ? gen_seeds : seeds;
        const dp_patch *out = nullptr;
        int64_t n_out = 0;
        dp_densify_stats st;
        std::memset(&st, 0, sizeof st);
        std::vector<dp_patch> multi_out;
        int64_t exchanged = -1;
        std::vector<dp_iterate_stats> iters;
        dp_filter_options filt;
        dp_default_filter_options(&filt);
        bool filtered = false; // `out` holds survivors only
        if (gpus > 1 || force_multi) {
            // contexts 1..N-1 on the next devices (wrapping: several ranks may share a GPU)
            const int ndev = dp_device_count();
            std::vector<dp_ctx *> ctxs{ctx};
            std::vector<int> devices{device};
            // a failure on a secondary context reports THAT context's error and
            // releases every context created so far before exiting
            auto check_g = [&](int rc, dp_ctx *cg, const char *what) {
                if (rc == DP_OK)
                    return;
                std::fprintf(stderr, "densify: %s failed on context %zu (%d): %s\n", what, ctxs.size(), rc,
                             cg ? dp_last_error(cg) : "context not created");
                if (cg && (ctxs.empty() || ctxs.back() != cg))
                    dp_ctx_destroy(cg);
                for (dp_ctx *x : ctxs)
                    dp_ctx_destroy(x);
                std::exit(1);
            };
            for (int g = 1; g < gpus; ++g) {
                dp_ctx *cg = nullptr;
                const int dg = (device + g) % (ndev > 0 ? ndev : 1);
                check_g(dp_ctx_create(&opt, dg, &cg), cg, "dp_ctx_create");
                ctxs.push_back(cg);
                devices.push_back(dg);
                check_g(dp_set_views(cg, (int)imgs.size(), P.data(), dimg.data()), cg, "dp_set_views");
                check_g(dp_set_fast_options(cg, &fo), cg, "dp_set_fast_options");
                if (level > 0) {
                    check_g(dp_build_pyramid(cg, level + 1), cg, "dp_build_pyramid");
                    check_g(dp_set_level(cg, level), cg, "dp_set_level");
                }
            }
            std::string err;
            const int64_t rb = replicate_below >= 0 ? (int64_t)replicate_below : 1024 * (int64_t)gpus;
            const int mrc =
                densify_multi(ctxs, devices, exchange_mode.c_str(), use, multi_out, st, err, exchanged, rb, iterations, filt,
                              iters);
            for (int g = 1; g < gpus; ++g)
                dp_ctx_destroy(ctxs[(size_t)g]);
            if (mrc != DP_OK) {
                std::fprintf(stderr, "densify: multi-GPU densify failed (%d): %s\n", mrc, err.c_str());
                dp_ctx_destroy(ctx);
                return 1;
            }
            out = multi_out.data();
            n_out = (int64_t)multi_out.size();
        } else if (iterations > 1) {
            // expansion and filter alternated on the device (dp_densify_iterate)
            iters.assign((size_t)iterations, dp_iterate_stats{});
            check(dp_densify_iterate(ctx, use.data(), (int)(use.size() / 3), iterations, &filt, &out, &n_out, &st,
                                     iters.data()),
                  "dp_densify_iterate");
            filtered = true;
        } else {
            check(dp_densify(ctx, use.data(), (int)(use.size() / 3), &out, &n_out, &st), "dp_densify");
        }
        // PMVS::FilterPatches (pmvs.h:27, undefined in the reference): dp_filter_patches spec
        std::vector<uint8_t> keep((size_t)n_out, 1);
        if (do_filter && !filtered && n_out > 0)
            check(dp_filter_patches(ctx, out, n_out, &filt, keep.data()), "dp_filter_patches");
        std::vector<dpio::CloudPoint> cloud;
        cloud.reserve((size_t)n_out);
        for (int64_t i = 0; i < n_out; ++i) {
            if (!keep[i])
                continue;
            dpio::CloudPoint cp;
            for (int k = 0; k < 3; ++k) {
                cp.pos[k] = out[i].pos[k];
                cp.normal[k] = out[i].normal[k];
                cp.rgb[k] = out[i].rgb[k];
            }
            cloud.push_back(cp);
        }
        dpio::write_ply(output, cloud);
        // --depth-maps: the written patches as per-view depth (and normal) maps of
        // the level the densify ran on (dp_render_maps), one view at a time; with
        // --gpus N this context (rank 0) renders, the store being replicated
        char depth_json[160] = "";
        if (!depth_dir.empty()) {
            if (mkdir(depth_dir.c_str(), 0777) != 0 && errno != EEXIST)
                throw std::runtime_error("cannot create " + depth_dir);
            std::vector<dp_patch> kept;
            kept.reserve(cloud.size());
            for (int64_t i = 0; i < n_out; ++i)
                if (keep[i])
                    kept.push_back(out[i]);
            dp_render_options ro;
            dp_default_render_options(&ro);
            ro.splat_scale = (float)splat_scale;
            int64_t covered = 0;
            double render_ms = 0.0;
            std::vector<float> depth, normal;
            for (int32_t v = 0; v < (int32_t)imgs.size(); ++v) {
                int32_t w = 0, h = 0;
                check(dp_level_info(ctx, level, v, &w, &h, nullptr), "dp_level_info");
                depth.assign((size_t)w * h, 0.0f);
                if (depth_normals)
                    normal.assign((size_t)w * h * 3, 0.0f);
                float *pd = depth.data(), *pn = depth_normals ? normal.data() : nullptr;
                dp_render_stats rs;
                check(dp_render_maps(ctx, kept.data(), (int64_t)kept.size(), nullptr, &v, 1, &ro, &pd, nullptr,
                                     depth_normals ? &pn : nullptr, nullptr, &rs),
                      "dp_render_maps");
                covered += rs.covered_pixels;
                render_ms += rs.render_ms;
                char name[64];
                std::snprintf(name, sizeof name, "/depth_%04d.pfm", (int)v);
                write_pfm(depth_dir + name, pd, w, h, 1);
                if (depth_normals) {
                    std::snprintf(name, sizeof name, "/normal_%04d.pfm", (int)v);
                    write_pfm(depth_dir + name, pn, w, h, 3);
                }
            }
            std::snprintf(depth_json, sizeof depth_json,
                          ", \"depth_maps\": {\"views\": %zu, \"covered_pixels\": %lld, \"render_ms\": %.3f}",
                          imgs.size(), (long long)covered, render_ms);
        }
        // --fuse: depth and normal maps of every view rendered into device planes
        // (dp_render_maps_device, honouring --splat-scale) and fused there
        // (dp_fuse_maps_device); only the points come back.  An empty pixel is
        // never emitted, so the render's covered pixels size the point buffer;
        // should the fusion report more, it is reallocated once and re-run.
        std::string fused_json;
        if (!fuse_path.empty()) {
            std::vector<dp_patch> kept;
            kept.reserve(cloud.size());
            for (int64_t i = 0; i < n_out; ++i)
                if (keep[i])
                    kept.push_back(out[i]);
            const int V = (int)imgs.size();
            struct DevMem {
                std::vector<void *> p;
                void *get(size_t bytes)
                {
                    void *q = nullptr;
                    if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess)
                        throw std::runtime_error("--fuse: out of device memory");
                    p.push_back(q);
                    return q;
                }
                ~DevMem()
                {
                    for (void *q : p)
                        (void)hipFree(q);
                }
            } mem;
            check(hipSetDevice(device) == hipSuccess ? DP_OK : DP_E_HIP, "hipSetDevice");
            std::vector<int32_t> vid((size_t)V);
            std::vector<float *> dd((size_t)V), dn((size_t)V);
            for (int32_t v = 0; v < V; ++v) {
                int32_t w = 0, h = 0;
                check(dp_level_info(ctx, level, v, &w, &h, nullptr), "dp_level_info");
                vid[(size_t)v] = v;
                dd[(size_t)v] = (float *)mem.get((size_t)w * h * 4);
                dn[(size_t)v] = (float *)mem.get((size_t)w * h * 12);
            }
            dp_patch *d_pat = (dp_patch *)mem.get(kept.size() * sizeof(dp_patch));
            if (!kept.empty() &&
                hipMemcpy(d_pat, kept.data(), kept.size() * sizeof(dp_patch), hipMemcpyHostToDevice) != hipSuccess)
                throw std::runtime_error("--fuse: copy of the patches failed");
            dp_render_options ro;
            dp_default_render_options(&ro);
            ro.splat_scale = (float)splat_scale;
            dp_render_stats rs;
            check(dp_render_maps_device(ctx, kept.empty() ? nullptr : d_pat, (int64_t)kept.size(), nullptr, vid.data(), V,
                                        &ro, dd.data(), nullptr, dn.data(), nullptr, &rs, nullptr),
                  "dp_render_maps_device");
            int64_t cap = rs.covered_pixels, n_fused = 0;
            dp_fuse_stats fs;
            dp_fused_point *d_pts = nullptr;
            for (int attempt = 0; attempt < 2; ++attempt) {
                d_pts = (dp_fused_point *)mem.get((size_t)cap * sizeof(dp_fused_point));
                check(dp_fuse_maps_device(ctx, vid.data(), V, &fuse_opt, dd.data(), dn.data(), d_pts, cap, &n_fused, &fs,
                                          nullptr),
                      "dp_fuse_maps_device");
                if (n_fused <= cap)
                    break;
                cap = n_fused;
            }
            if (n_fused > cap)
                throw std::runtime_error("--fuse: the point count changed between two runs");
            std::vector<dp_fused_point> pts((size_t)n_fused);
            if (n_fused > 0 &&
                hipMemcpy(pts.data(), d_pts, pts.size() * sizeof(dp_fused_point), hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("--fuse: copy of the points failed");
            std::vector<dpio::CloudPoint> fused(pts.size());
            for (size_t i = 0; i < pts.size(); ++i)
                for (int k = 0; k < 3; ++k) {
                    fused[i].pos[k] = pts[i].pos[k];
                    fused[i].normal[k] = pts[i].normal[k];
                    fused[i].rgb[k] = pts[i].rgb[k];
                }
            dpio::write_ply(fuse_path, fused);
            char buf[240];
            std::snprintf(buf, sizeof buf,
                          ", \"fused\": {\"points\": %lld, \"fusable\": %lld, \"depth_pixels\": %lld, \"fuse_ms\": %.3f}",
                          (long long)n_fused, (long long)fs.fusable, (long long)fs.depth_pixels, fs.fuse_ms);
            fused_json = buf;
        }
        dp_ctx_destroy(ctx);
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
        if (!filtered) {
            iters.back().filtered_out = n_out - (int64_t)cloud.size();
            if (iterations > 1)
                st.patches = (int64_t)cloud.size(); // as dp_densify_iterate reports: the survivors
        }
        std::string iters_json = "[";
        for (size_t k = 0; k < iters.size(); ++k) {
            char buf[320];
            std::snprintf(buf, sizeof buf,
                          "%s{\"offered\": %lld, \"reinserted\": %lld, \"patches\": %lld, \"filtered_out\": %lld, "
                          "\"candidates\": %lld, \"evals\": %lld, \"generations\": %d}",
                          k ? ", " : "", (long long)iters[k].offered, (long long)iters[k].reinserted,
                          (long long)iters[k].patches, (long long)iters[k].filtered_out, (long long)iters[k].candidates,
                          (long long)iters[k].evals, iters[k].generations);
            iters_json += buf;
        }
        iters_json += "]";
        const double wall =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("{\"output\": \"%s\", \"patches\": %lld, \"written\": %zu, \"seeds\": %zu, \"generated_seeds\": %s, "
                    "\"keypoints\": %lld, \"matches\": %lld, \"seed_ms\": %.3f, \"seed_patches\": %lld, "
                    "\"pops\": %lld, \"candidates\": %lld, \"evals\": %lld, \"generations\": %d, \"refine_ms\": %.3f, "
                    "\"densify_ms\": %.3f, \"wall_ms\": %.3f, \"gpus\": %d, \"mode\": \"%s\", \"exchanged\": %lld, "
                    "\"iterations\": %s%s%s}\n",
                    output.c_str(), (long long)st.patches, cloud.size(), use.size() / 3,
                    seeds_path.empty() ? "true" : "false", (long long)sst.keypoints, (long long)sst.matches,
                    sst.total_ms, (long long)st.seed_patches, (long long)st.pops, (long long)st.candidates,
                    (long long)st.evals, st.generations, st.refine_ms, st.total_ms, wall, gpus,
                    fast ? "fast" : "parity", (long long)exchanged, iters_json.c_str(), depth_json, fused_json.c_str());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "densify: %s\n", e.what());
        return 1;
    }
}
