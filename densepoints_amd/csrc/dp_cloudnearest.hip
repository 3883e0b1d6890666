// dp_cloudnearest.hip -- the gfx950 kernels of the nearest-point search between
// two clouds (spec in include/densepoints.h, dp_cloud_nearest) and its C ABI: a
// uniform grid over the targets' bounding box, every query walking the 3 x 3 x 3
// cells around its own.
//
//   cloud_box_kernel     the bounding box of the targets taking part: a fixed
//                        number of blocks stride over the targets, one box per
//                        block (min and max of floats do not depend on order)
//   cloud_plan_kernel    one block: the boxes' box and, from it, the grid (below);
//                        made on the device so that the device form never waits
//   cloud_tkeys_kernel   one lane per target: its cell key, the cap's own value for
//                        one that does not take part (it sorts behind every cell)
//   (one stable hipcub radix sort of (key, target) over the bits of the cap)
//   cloud_gather_kernel  the sorted targets' x, y and z as three arrays
//   cloud_begin_kernel   one lane per key 0..cap: the first sorted position
//                        whose key is not below it (a binary search; no atomics,
//                        no memset, the empty cells included)
//   cloud_maxcell_kernel the most targets in one cell (one atomicMax per wave)
//   cloud_qkeys_kernel   one lane per query: the key of the cell nearest to it
//   (the same sort of (key, query): neighbouring lanes walk the same cells)
//   cloud_query_kernel   one lane per cell-sorted query.  With the key (z * ny +
//                        y) * nx + x the three x-neighbours of a cell are one run
//                        of sorted targets, so a query walks 9 runs; the lanes
//                        of a wave mostly read the same addresses.  The results
//                        are scattered to the queries' own positions.
//
// The grid.  The cell side starts at max_dist * (1 + 2^-20) on every axis; while
// the cells number more than the cap (a power of two, 2 * n_targets within 2^16 ..
// 2^24, known to the host, so the sort's bits are too) the axis with the most
// cells doubles its side.  A larger cell is always correct, only slower, and the
// table stays bounded whatever extent / max_dist is.
//
// Why the margin suffices.  A point's cell on an axis is floor(u), u = ((double)x
// - origin) / cell: two fp64 roundings, so the computed u is the true one times
// (1 + e), |e| < 2^-52.  A candidate has d2 <= R2 in fp64, so on every axis the
// true |q - t| <= max_dist * (1 + 2^-51), and the true u differ by at most (1 +
// 2^-51) / (1 + 2^-20) < 1 - 2^-21.  Near the box |u| <= 2^24 + 1 (an axis has
// at most cap cells), so the computed u differ by less than 1 - 2^-21 + 2^-26 <
// 1 and their floors by at most 1: the candidate is in the 3 x 3 x 3 walk.  The
// clamp of a query's u to [-2, n + 1], done in fp64 before any conversion to an
// integer, is monotonic and leaves the targets' range [0, n - 1] alone, so it
// keeps that; a query more than a cell outside the box finds every run empty.
// The cell only bounds the walk: the fp64 test d2 <= R2 decides.
// The argument block, load_point, cell_coord and the constants are
// dp_clouddev.h's; cloud_targets_queue and cloud_queries_queue below are what
// dp_cloudknn.hip and dp_cloudalign.hip share.
#include "dp_clouddev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

__global__ __launch_bounds__(kMeshLanes) void cloud_box_kernel(CloudArgs a)
{
    __shared__ float part[kMeshLanes / 64][6];
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t i = mesh_item(); i < a.nt; i += (int64_t)gridDim.x * kMeshLanes) {
        float p[3];
        if (load_point(a.targets, a.tstride, i, p))
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], p[k]);
                hi[k] = fmaxf(hi[k], p[k]);
            }
    }
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) {
            part[threadIdx.x >> 6][k] = lo[k];
            part[threadIdx.x >> 6][3 + k] = hi[k];
        }
    __syncthreads();
    if (threadIdx.x < 3) {
        float l = part[0][threadIdx.x], h = part[0][3 + threadIdx.x];
        for (int w = 1; w < kMeshLanes / 64; ++w) {
            l = fminf(l, part[w][threadIdx.x]);
            h = fmaxf(h, part[w][3 + threadIdx.x]);
        }
        a.boxes[6 * blockIdx.x + threadIdx.x] = l;
        a.boxes[6 * blockIdx.x + 3 + threadIdx.x] = h;
    }
}

// one block: the box of the boxes, then the grid
__global__ __launch_bounds__(kMeshLanes) void cloud_plan_kernel(CloudArgs a)
{
    __shared__ float part[kMeshLanes / 64][6];
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int b = threadIdx.x; b < a.nboxes; b += kMeshLanes)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], a.boxes[6 * b + k]);
            hi[k] = fmaxf(hi[k], a.boxes[6 * b + 3 + k]);
        }
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) {
            part[threadIdx.x >> 6][k] = lo[k];
            part[threadIdx.x >> 6][3 + k] = hi[k];
        }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (int w = 1; w < kMeshLanes / 64; ++w)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], part[w][k]);
            hi[k] = fmaxf(hi[k], part[w][3 + k]);
        }
    CloudGrid g{};
    double ext[3], n[3];
    const bool none = !(lo[0] <= hi[0]); // no target takes part: one cell that nothing falls in
    for (int k = 0; k < 3; ++k) {
        g.origin[k] = none ? 0.0 : (double)lo[k];
        ext[k] = none ? 0.0 : (double)hi[k] - (double)lo[k];
        g.cell[k] = a.R * (1.0 + 0x1p-20);
        n[k] = floor(ext[k] / g.cell[k]) + 1.0;
    }
    // every doubling at least halves the axis' excess over one cell, so this ends
    while (n[0] * n[1] * n[2] > (double)a.cap) {
        const int k = n[0] >= n[1] && n[0] >= n[2] ? 0 : (n[1] >= n[2] ? 1 : 2);
        g.cell[k] = g.cell[k] * 2.0;
        n[k] = floor(ext[k] / g.cell[k]) + 1.0;
    }
    for (int k = 0; k < 3; ++k)
        g.n[k] = (int32_t)n[k];
    g.cells = (int64_t)g.n[0] * g.n[1] * g.n[2];
    g.maxcell = 0;
    *a.grid = g;
}

__global__ __launch_bounds__(kMeshLanes) void cloud_tkeys_kernel(CloudArgs a)
{
    const int64_t i = mesh_item();
    bool part = false;
    if (i < a.nt) {
        const CloudGrid &g = *a.grid;
        float p[3];
        part = load_point(a.targets, a.tstride, i, p);
        uint32_t key = (uint32_t)a.cap;
        if (part) {
            const int32_t x = cell_coord(g, 0, p[0], 0.0, -1.0), y = cell_coord(g, 1, p[1], 0.0, -1.0),
                          z = cell_coord(g, 2, p[2], 0.0, -1.0);
            key = (uint32_t)((z * g.n[1] + y) * g.n[0] + x);
        }
        a.tkeys[i] = key;
        a.tidx[i] = (int32_t)i;
    }
    wave_count<kCloudStripes, kCloudCounters>(a.count, 0, part ? 1ull : 0ull, wave_stripe());
}

__global__ __launch_bounds__(kMeshLanes) void cloud_gather_kernel(CloudArgs a)
{
    const int64_t i = mesh_item();
    if (i >= a.nt)
        return;
    float p[3];
    load_point(a.targets, a.tstride, a.tidx_sorted[i], p);
    a.tx[i] = p[0];
    a.ty[i] = p[1];
    a.tz[i] = p[2];
}

__global__ __launch_bounds__(kMeshLanes) void cloud_begin_kernel(CloudArgs a)
{
    const int64_t k = mesh_item();
    if (k > a.cap)
        return;
    int64_t lo = 0, hi = a.nt; // the first position whose key is >= k
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.tkeys_sorted[mid] < (uint32_t)k)
            lo = mid + 1;
        else
            hi = mid;
    }
    a.begin[k] = (int32_t)lo;
}

__global__ __launch_bounds__(kMeshLanes) void cloud_maxcell_kernel(CloudArgs a)
{
    const int64_t k = mesh_item();
    int32_t v = k < a.cap ? a.begin[k + 1] - a.begin[k] : 0;
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0 && v)
        atomicMax(&a.grid->maxcell, v);
}

__global__ __launch_bounds__(kMeshLanes) void cloud_qkeys_kernel(CloudArgs a)
{
    const int64_t i = mesh_item();
    if (i >= a.nq)
        return;
    const CloudGrid &g = *a.grid;
    float p[3];
    uint32_t key = (uint32_t)a.cap;
    if (load_point(a.queries, a.qstride, i, p)) {
        const int32_t x = cell_coord(g, 0, p[0], 0.0, -1.0), y = cell_coord(g, 1, p[1], 0.0, -1.0),
                      z = cell_coord(g, 2, p[2], 0.0, -1.0);
        key = (uint32_t)((z * g.n[1] + y) * g.n[0] + x);
    }
    a.qkeys[i] = key;
    a.qidx[i] = (int32_t)i;
}

__global__ __launch_bounds__(kMeshLanes) void cloud_query_kernel(CloudArgs a)
{
    const int64_t i = mesh_item();
    const bool in = i < a.nq;
    const CloudGrid &g = *a.grid;
    float p[3] = {0.0f, 0.0f, 0.0f};
    int64_t qi = 0;
    bool part = false;
    if (in) {
        qi = a.qidx_sorted[i];
        part = load_point(a.queries, a.qstride, qi, p);
    }
    double best = __builtin_huge_val();
    int32_t who = -1;
    if (part) {
        const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
        const int32_t cx = cell_coord(g, 0, p[0], -2.0, 1.0), cy = cell_coord(g, 1, p[1], -2.0, 1.0),
                      cz = cell_coord(g, 2, p[2], -2.0, 1.0);
        const int32_t x0 = max(cx - 1, 0), x1 = min(cx + 1, g.n[0] - 1);
        for (int32_t z = max(cz - 1, 0); z <= min(cz + 1, g.n[2] - 1) && x0 <= x1; ++z)
            for (int32_t y = max(cy - 1, 0); y <= min(cy + 1, g.n[1] - 1); ++y) {
                const int32_t row = (z * g.n[1] + y) * g.n[0];
                const int32_t e = a.begin[row + x1 + 1];
                for (int32_t j = a.begin[row + x0]; j < e; ++j) {
                    const double dx = q[0] - (double)a.tx[j], dy = q[1] - (double)a.ty[j], dz = q[2] - (double)a.tz[j];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= a.R2 && d2 <= best) {
                        const int32_t t = a.tidx_sorted[j];
                        if (d2 < best || t < who) {
                            best = d2;
                            who = t;
                        }
                    }
                }
            }
    }
    if (in) {
        const float d = who >= 0 ? (float)dpg::dvsqrt(best) : __builtin_huge_valf();
        a.index[qi] = who;
        a.dist[qi] = d;
        if (who >= 0 && a.hist) {
            const double b = floor(dpg::dvdiv((double)d, a.R) * (double)a.bins);
            const int64_t last = (int64_t)a.bins - 1, bin = (int64_t)b < last ? (int64_t)b : last;
            atomicAdd(&a.hist[bin], 1ull);
        }
    }
    const uint32_t stripe = wave_stripe();
    wave_count<kCloudStripes, kCloudCounters>(a.count, 1, part ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 2, part && who >= 0 ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 3, part && who < 0 ? 1ull : 0ull, stripe);
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

// the counts, pointers and strides (dp_clouddev.h)
int cloud_check_clouds(dp_ctx *c, const std::string &w, const void *queries, int64_t nq, int64_t qstride,
                       const void *targets, int64_t nt, int64_t tstride)
{
    if (nq < 0 || nt < 0 || nq > 0x7FFFFFFFll || nt > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n_queries and n_targets must be in 0..2^31 - 1");
    if (nq > 0 && !queries)
        return fail(c, DP_E_ARG, w + ": queries must be given");
    if (nt > 0 && !targets)
        return fail(c, DP_E_ARG, w + ": targets must be given");
    if (qstride < 12 || qstride % 4)
        return fail(c, DP_E_ARG, w + ": query_stride must be a multiple of 4 and at least 12");
    if (tstride < 12 || tstride % 4)
        return fail(c, DP_E_ARG, w + ": target_stride must be a multiple of 4 and at least 12");
    return DP_OK;
}

// argument checks shared by both forms (they need no device)
static int cloud_check(dp_ctx *c, const std::string &w, const void *queries, int64_t nq, int64_t qstride,
                       const void *targets, int64_t nt, int64_t tstride, const dp_cloud_nearest_options *o)
{
    const int rc = cloud_check_clouds(c, w, queries, nq, qstride, targets, nt, tstride);
    if (rc != DP_OK)
        return rc;
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if (!(o->max_dist > 0.0f) || !std::isfinite(o->max_dist))
        return fail(c, DP_E_ARG, w + ": max_dist must be finite and > 0");
    if (o->hist_bins < 0 || o->hist_bins > 65536)
        return fail(c, DP_E_ARG, w + ": hist_bins must be in 0..65536");
    if (o->flags)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    return DP_OK;
}

// the bits of the sort's keys: a point that does not take part has the key cap itself
static int cloud_end_bit(int32_t cap)
{
    int bits = 0;
    while ((1 << bits) < cap)
        ++bits;
    return bits + 1;
}

// the grid over the targets (dp_clouddev.h)
int cloud_targets_queue(dp_ctx *c, dpk::CloudArgs &a, hipStream_t s)
{
    const int64_t nt = a.nt, nq = a.nq;
    dpk::CloudNearestScratch &r = c->cloudnearest;
    // the cap: the power of two at or above 2 * n_targets, within 2^16..2^24
    int cap_bits = dpk::kCloudCapMinBits;
    while (cap_bits < dpk::kCloudCapMaxBits && (1ll << cap_bits) < 2 * nt)
        ++cap_bits;
    const int32_t cap = 1 << cap_bits;
    const int end_bit = cap_bits + 1; // the key of a point that does not take part is cap itself
    const int64_t box_blocks = std::min<int64_t>(dpk::mesh_blocks(nt), dpk::kCloudBoxBlocks);
    const size_t t = (size_t)std::max<int64_t>(nt, 1), q = (size_t)std::max<int64_t>(nq, 1);
    DP_HIP(c, r.boxes.reserve(6 * (size_t)dpk::kCloudBoxBlocks));
    DP_HIP(c, r.grid.reserve(1));
    DP_HIP(c, r.tkeys.reserve(t));
    DP_HIP(c, r.tkeys_sorted.reserve(t));
    DP_HIP(c, r.tidx.reserve(t));
    DP_HIP(c, r.tidx_sorted.reserve(t));
    DP_HIP(c, r.tx.reserve(t));
    DP_HIP(c, r.ty.reserve(t));
    DP_HIP(c, r.tz.reserve(t));
    DP_HIP(c, r.begin.reserve((size_t)cap + 1));
    DP_HIP(c, r.qkeys.reserve(q));
    DP_HIP(c, r.qkeys_sorted.reserve(q));
    DP_HIP(c, r.qidx.reserve(q));
    DP_HIP(c, r.qidx_sorted.reserve(q));
    DP_HIP(c, r.count.reserve(dpk::kCloudStripes, dpk::kCloudCounters, (sizeof(dpk::CloudGrid) + 7) / 8));

    a.cap = cap;
    a.nboxes = (int32_t)box_blocks;
    a.boxes = r.boxes.p;
    a.grid = r.grid.p;
    a.tkeys = r.tkeys.p;
    a.tkeys_sorted = r.tkeys_sorted.p;
    a.qkeys = r.qkeys.p;
    a.qkeys_sorted = r.qkeys_sorted.p;
    a.tidx = r.tidx.p;
    a.tidx_sorted = r.tidx_sorted.p;
    a.qidx = r.qidx.p;
    a.qidx_sorted = r.qidx_sorted.p;
    a.begin = r.begin.p;
    a.tx = r.tx.p;
    a.ty = r.ty.p;
    a.tz = r.tz.p;
    a.count = r.count.dev.p;

    size_t tmp = 0, b = 0;
    if (nt > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.tkeys, a.tkeys_sorted, a.tidx, a.tidx_sorted, (int)nt, 0,
                                                     end_bit, s));
        tmp = std::max(tmp, b);
    }
    if (nq > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.qkeys, a.qkeys_sorted, a.qidx, a.qidx_sorted, (int)nq, 0,
                                                     end_bit, s));
        tmp = std::max(tmp, b);
    }
    DP_HIP(c, c->scan_tmp.reserve(tmp ? tmp : 1));

    DP_HIP(c, r.count.zero(s));
    // the grid
    DP_HIP(c, r.time[0].begin(s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_box_kernel, box_blocks, a, s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_plan_kernel, 1, a, s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_tkeys_kernel, dpk::mesh_blocks(nt), a, s));
    if (nt > 0) {
        b = tmp;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.tkeys, a.tkeys_sorted, a.tidx, a.tidx_sorted,
                                                     (int)nt, 0, end_bit, s));
    }
    DP_HIP(c, dpk::launch_over(dpk::cloud_gather_kernel, dpk::mesh_blocks(nt), a, s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_begin_kernel, dpk::mesh_blocks((int64_t)cap + 1), a, s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_maxcell_kernel, dpk::mesh_blocks(cap), a, s));
    DP_HIP(c, r.time[0].end(s));
    return DP_OK;
}

// the queries' cell order (dp_clouddev.h)
int cloud_queries_queue(dp_ctx *c, const dpk::CloudArgs &a, hipStream_t s)
{
    const int64_t nq = a.nq;
    const int end_bit = cloud_end_bit(a.cap);
    DP_HIP(c, c->cloudnearest.time[1].begin(s));
    DP_HIP(c, dpk::launch_over(dpk::cloud_qkeys_kernel, dpk::mesh_blocks(nq), a, s));
    if (nq > 0) {
        // cloud_targets_queue reserved the larger of the two sorts' needs
        size_t b = c->scan_tmp.cap;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.qkeys, a.qkeys_sorted, a.qidx, a.qidx_sorted,
                                                     (int)nq, 0, end_bit, s));
    }
    return DP_OK;
}

int cloud_nearest_walk_queue(dp_ctx *c, const dpk::CloudArgs &a, hipStream_t s)
{
    DP_HIP(c, dpk::launch_over(dpk::cloud_query_kernel, dpk::mesh_blocks(a.nq), a, s));
    DP_HIP(c, c->cloudnearest.time[1].end(s));
    return DP_OK;
}

// queues the search of device clouds on s
static int cloud_queue(dp_ctx *c, const dp_cloud_nearest_options &o, const void *d_queries, int64_t nq, int64_t qstride,
                       const void *d_targets, int64_t nt, int64_t tstride, int32_t *d_index, float *d_dist,
                       uint64_t *d_hist, hipStream_t s)
{
    dpk::CloudArgs a{};
    a.targets = (const char *)d_targets;
    a.queries = (const char *)d_queries;
    a.nt = nt;
    a.nq = nq;
    a.tstride = tstride;
    a.qstride = qstride;
    a.bins = o.hist_bins;
    a.R = (double)o.max_dist;
    a.R2 = (double)o.max_dist * (double)o.max_dist;
    a.index = d_index;
    a.dist = d_dist;
    a.hist = o.hist_bins > 0 ? (unsigned long long *)d_hist : nullptr;
    if (a.hist)
        DP_HIP(c, hipMemsetAsync(a.hist, 0, sizeof(unsigned long long) * (size_t)o.hist_bins, s));
    int rc = cloud_targets_queue(c, a, s);
    if (rc != DP_OK || (rc = cloud_queries_queue(c, a, s)) != DP_OK)
        return rc;
    return cloud_nearest_walk_queue(c, a, s);
}

// the statistics read and its wait
static int cloud_stats(dp_ctx *c, int64_t nq, int64_t nt, dp_cloud_nearest_stats *stats, hipStream_t s)
{
    dpk::CloudNearestScratch &r = c->cloudnearest;
    DP_HIP(c, r.count.read(s));
    DP_HIP(c, hipMemcpyAsync(r.count.extra(), r.grid.p, sizeof(dpk::CloudGrid), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    const dpk::CloudGrid *g = (const dpk::CloudGrid *)r.count.extra();
    stats->targets = r.count.sum(0);
    stats->queries = r.count.sum(1);
    stats->skipped_queries = nq - stats->queries;
    stats->skipped_targets = nt - stats->targets;
    stats->matched = r.count.sum(2);
    stats->unmatched = r.count.sum(3);
    stats->grid_cells = g->cells;
    stats->max_cell_targets = g->maxcell;
    DP_HIP(c, r.time[0].ms(stats->build_ms));
    DP_HIP(c, r.time[1].ms(stats->query_ms));
    return DP_OK;
}

extern "C" int dp_cloud_nearest_device(dp_ctx *c, const void *d_queries, int64_t n_queries, int64_t query_stride,
                                       const void *d_targets, int64_t n_targets, int64_t target_stride,
                                       const dp_cloud_nearest_options *opts, int32_t *d_index, float *d_dist,
                                       uint64_t *d_hist, dp_cloud_nearest_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_nearest_device";
    int rc = cloud_check(c, w, d_queries, n_queries, query_stride, d_targets, n_targets, target_stride, opts);
    if (rc != DP_OK)
        return rc;
    if (n_queries > 0 && !d_index)
        return fail(c, DP_E_ARG, w + ": d_index must be given");
    if (n_queries > 0 && !d_dist)
        return fail(c, DP_E_ARG, w + ": d_dist must be given");
    if ((rc = mesh_check_alias(c, w, {d_index, d_dist, d_hist}, {d_queries, d_targets})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = cloud_queue(c, *opts, d_queries, n_queries, query_stride, d_targets, n_targets, target_stride, d_index,
                          d_dist, d_hist, s)) != DP_OK)
        return rc;
    return stats ? cloud_stats(c, n_queries, n_targets, stats, s) : DP_OK;
}

extern "C" int dp_cloud_nearest(dp_ctx *c, const void *queries, int64_t n_queries, int64_t query_stride,
                                const void *targets, int64_t n_targets, int64_t target_stride,
                                const dp_cloud_nearest_options *opts, const int32_t **index, const float **dist,
                                const uint64_t **hist, dp_cloud_nearest_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_nearest";
    int rc = cloud_check(c, w, queries, n_queries, query_stride, targets, n_targets, target_stride, opts);
    if (rc != DP_OK)
        return rc;
    if (!index)
        return fail(c, DP_E_ARG, w + ": index must be given");
    if (!dist)
        return fail(c, DP_E_ARG, w + ": dist must be given");
    if ((rc = mesh_check_alias(c, w, {index, dist, hist}, {queries, targets})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudNearestScratch &r = c->cloudnearest;
    const int64_t nq = n_queries, nt = n_targets;
    const size_t bins = hist ? (size_t)opts->hist_bins : 0;
    // an array is staged from its first point to the end of its last
    const size_t qbytes = nq > 0 ? (size_t)(nq - 1) * (size_t)query_stride + 12 : 0;
    const size_t tbytes = nt > 0 ? (size_t)(nt - 1) * (size_t)target_stride + 12 : 0;
    PlanePacker pin, pout;
    const size_t iq = pin.add(qbytes), it = pin.add(tbytes);
    const size_t oi = pout.add(4 * (size_t)nq), od = pout.add(4 * (size_t)nq), oh = pout.add(8 * bins);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hindex.resize((size_t)std::max<int64_t>(nq, 1)));
    DP_HIP(c, r.hdist.resize((size_t)std::max<int64_t>(nq, 1)));
    DP_HIP(c, r.hhist.resize(std::max<size_t>(bins, 1)));
    if (nq > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + iq, queries, qbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + it, targets, tbytes, hipMemcpyHostToDevice, s));
    if ((rc = cloud_queue(c, *opts, r.in.p + iq, nq, query_stride, r.in.p + it, nt, target_stride,
                          (int32_t *)(r.out.p + oi), (float *)(r.out.p + od),
                          bins ? (uint64_t *)(r.out.p + oh) : nullptr, s)) != DP_OK)
        return rc;
    if (nq > 0) {
        DP_HIP(c, hipMemcpyAsync(r.hindex.data(), r.out.p + oi, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipMemcpyAsync(r.hdist.data(), r.out.p + od, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    }
    if (bins)
        DP_HIP(c, hipMemcpyAsync(r.hhist.data(), r.out.p + oh, 8 * bins, hipMemcpyDeviceToHost, s));
    if (stats) {
        if ((rc = cloud_stats(c, nq, nt, stats, s)) != DP_OK)
            return rc;
    } else {
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *index = nq > 0 ? r.hindex.data() : nullptr;
    *dist = nq > 0 ? r.hdist.data() : nullptr;
    if (bins)
        *hist = r.hhist.data();
    return DP_OK;
}
