// dp_fast.h -- what the performance mode's two translation units share:
// dp_fast_kernel.hip (the device code and its launchers) and dp_fast.hip (the
// host side: options, gray planes, dp_fast_launch, C ABI).
#pragma once

#include "dp_ctx.h"

#include <hip/hip_fp16.h>

namespace dpk {

constexpr int kFastMaxV = 32;     // staged views per patch (per-view records)
constexpr int kFastMaxBbox = 48;  // window bounding-box side cap (grazing views)
constexpr int kFastMaxMargin = 7; // keeps a tile row <= 64 entries (one lane each)
constexpr int kFastSlots = 4;     // at most this many samples per lane per view pass
constexpr int kFastRec = 64;      // LDS record per staged view (bytes), counted in the budget
constexpr int kFastPoses = 4;     // poses per batched evaluation (start + 3 differences)
constexpr int kFastItems = 44;    // (view, pose) records per pass set
constexpr float kRcpMin = 0x1p-20f, kRcpMax = 0x1p+64f; // operand range of recip_rn
constexpr int kFastBudget = 16384; // the kernel's tile arena (dp_fast_options.tile_budget max)

struct GrayPlane {
    const __half *p;
    int32_t w, h, pitch, pad;
};

// fp32 camera of a view (or_fast.c fcam_of): rows 0-1 of P times 32 (1/32-px
// units), row 2, the centre and the unit x-axis, each rounded once on the host
struct FastCam {
    float Q[12];
    float C[3], xr[3];
    int32_t W, H;
};
static_assert(sizeof(FastCam) == 80, "FastCam is read as five 16-byte pieces");

struct FastArgs {
    const dpg::ViewDev *views;
    const GrayPlane *gray;
    const FastCam *cams;
    int32_t V, cell, mode, n;
    dp_options opt;
    dp_fast_options fo;
    dp_patch *patches;
    uint8_t *accept;
    uint32_t *work;
    unsigned long long *evals;
    const dp_patch *parents; // expansion: child c = parents[c / 4], direction c % 4
    int64_t parent0;         // chunk k's parent is parents[parent0 + (items ? items[k] : k)] ...
    const int64_t *items;
    int64_t max_pops;        // ... and expands only below this index (the pop cap)
    float cvis, ccand;       // cos(visible_angle), cos(candidate_angle) from the host libm, rounded
    float cvis2, ccand2;     // their squares (fp32)
    double dmin;             // NCC denominator floor in moment units, ((ncc_denom_min 256) N) N
    float dminf;             // the same, rounded to fp32 (the refine objective's floor)
    float gs;                // gradient per objective unit: (1 / fd_step) 2^-24
    unsigned long long *stats; // dp_fast_stats: patches, evals, view_evals, staged_bytes
    uint32_t chunk;          // candidates per dequeue: 4 (siblings share one parent read), or 1
                             // when the launch has fewer than 4 candidates per resident wave
    uint32_t resident;       // resident waves of the launch (the kGen instances pick chunk on the device)
    const GenDev *gen;       // device-resident BFS generation: n and parent0 read here (kGen)
    // densify epilogue (kEpi* bits, dp_internal.h): colour / claims of the
    // candidates that pass the filter, a claim's seq = (gen ? gen->seq0 : seq0) + index
    int32_t epi;
    uint32_t seq0;
    uint32_t *claim_grid;
    double grid_scale;
};

// the fast_kernel instance of the window (a.cell) and the tile arena that
// holds tile_budget (6656, 8192 or kFastBudget bytes)
hipError_t launch_fast(const FastArgs &a, int tile_budget, hipStream_t s);
// gray planes of V views in one launch; max_pitch / max_h: the largest plane's
hipError_t launch_gray(const PyrPlane *d_src, const GrayPlane *d_dst, int V, int max_pitch, int max_h, hipStream_t s);
// device probes of the kernel's arithmetic (tests/test_gpu_fast.py)
hipError_t launch_lds_probe(uint32_t *out);
hipError_t launch_grad_q24_probe(const double *x, int n, int32_t *out);
hipError_t launch_recip_probe(const float *x, int n, float *out);

} // namespace dpk

// the gray planes of the current level, built on demand exactly as the first
// performance-mode call builds them (dp_fast.hip); used by dp_mapref.hip
int dp_gray_planes(dp_ctx *c, std::vector<dpk::GrayPlane> &out);
