// multi_gpu.h -- dp_densify over several contexts of this process (one per
// GPU): the densify CLI's --gpus N / --multi driver.
#pragma once

#include "../../include/densepoints.h"

#include <string>
#include <vector>

// What a densify driver hands to the rest of the CLI, whichever one ran
// (dp_densify, dp_densify_iterate or densify_multi).
struct DensifyResult {
    const dp_patch *patches = nullptr; // the library's buffer (one context), else `owned`
    int64_t n = 0;
    std::vector<dp_patch> owned;
    dp_densify_stats stats{};
    std::vector<dp_iterate_stats> rounds; // empty: one round, described by `stats`
    int64_t exchanged = -1;               // records all-gathered; -1: one context
    bool filtered = false;                // `patches` holds the last filter's survivors only
};

struct MultiInput {
    std::vector<dp_ctx *> ctxs; // views set; context 0's stats are the ones reported
    std::vector<int> devices;   // of each context
    std::string exchange_mode;  // auto | rccl | copy
    int64_t replicate_below;
    int iterations;
    dp_filter_options filter; // of the rounds before the last
};

// The device-resident protocol of include/densepoints.h with ONE host wait per
// generation per context: every generation's items are partitioned by
// reference-view super-tile on the device (dp_densify_partition_async; the
// shares are host-known floor cuts), each context refines its share and
// compacts the accepted candidates into its slot
// (dp_densify_refine_share_async), the slots are all-gathered device to device
// (RCCL or peer copies), and every context commits the whole generation to its
// replicated organizer (dp_densify_commit_gathered_device, in its own host
// thread so the waits overlap) -- no candidate touches host memory, and the
// store equals dp_densify's bit for bit.  Expansion generations of fewer than
// replicate_below items run on every context device-resident instead
// (dp_densify_run_until: no partition, no exchange, eight per host wait).
// The stats are context 0's (evals summed, refine_ms maxed, over the contexts).
// iterations > 1: after each round but the last, every context filters its
// replicated store on the device (dp_filter_patches_device) and restarts the
// BFS from the survivors (dp_densify_resume_device on its own store): no
// exchange is added.  The caller filters the last round's store.  The stats
// then sum over the rounds; rounds[k] holds round k's counts (the last round's
// filtered_out is the caller's).  Every round's store is read back once for
// its statistics (dp_densify_result).
// Throws CliError ("multi-GPU densify failed (<rc>): ...").
DensifyResult densify_multi(const MultiInput &in, const std::vector<double> &seeds);
