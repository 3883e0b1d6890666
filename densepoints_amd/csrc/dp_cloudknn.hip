// dp_cloudknn.hip -- the gfx950 kernels of the k-nearest-neighbour search between
// two clouds and of the outlier filter built on it (specs in
// include/densepoints.h, dp_cloud_knn and dp_cloud_clean), and their C ABI.
//
// The grid, the sorted targets and the queries' cell order are dp_cloud_nearest's
// (cloud_targets_queue and cloud_queries_queue, dp_clouddev.h), and so is the proof that the 3 x 3 x 3 walk
// meets every candidate: a candidate has d2 <= R2 whatever k is.
//
//   knn_query_kernel<K>  one lane per cell-sorted query over the same 9 runs.  The
//                        lane keeps the K best (d2, target) pairs sorted in
//                        registers, K = 8, 16 or 32 (the smallest that holds k):
//                        every index into the list is a compile-time constant,
//                        so nothing goes to scratch memory.  A candidate is first
//                        compared with the worst entry -- once the list is full
//                        most are rejected there -- and otherwise inserted by one
//                        unrolled compare-and-shift pass.  The order is (d2, index)
//                        lexicographically, which is total, so the list does not
//                        depend on the order the runs deliver candidates in.
//   clean_mean_kernel    one lane per point: m_i from its row, d2 recomputed from
//                        the two points (the same expression, so the same bits)
//   clean_sum_kernel     one level of 2^8 of the balanced pairwise sum: xor
//                        shuffles 1, 2, .., 32 inside a wave (an add is
//                        commutative, so every lane holds the tree's value), the
//                        four waves' values through LDS, (w0 + w1) + (w2 + w3);
//                        the first level reads x_i or y_i, the others the level
//                        below.  Padding is +0.0, which leaves a sum of
//                        non-negative terms as it is, so blocks of 2^8 over n
//                        compute the tree over the next power of two.
//   clean_stat_kernel    one lane: mu after the first sum; var, sigma and T after
//                        the second.  They stay on the device: nothing waits.
//   clean_keep_kernel    the decision, the flags for the scan, the counters
//   (one hipcub exclusive scan of the flags)
//   clean_map_kernel     map and the kept count
//   clean_copy_kernel    one lane per 4-byte word of a record
#include "dp_clouddev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

constexpr int32_t kKnnNone = 0x7FFFFFFF; // an empty list entry's index: above every target's

struct KnnArgs {
    CloudArgs g;
    int32_t k, exclude_self;
    int32_t *count; // per query
};

// (d2, t) before (e2, u) in the answer's order
__device__ __forceinline__ bool knn_before(double d2, int32_t t, double e2, int32_t u)
{
    return d2 < e2 || (d2 == e2 && t < u);
}

template <int K> __global__ __launch_bounds__(kMeshLanes) void knn_query_kernel(KnnArgs ka)
{
    const CloudArgs &a = ka.g;
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
    double ld[K];
    int32_t li[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        ld[s] = __builtin_huge_val();
        li[s] = kKnnNone;
    }
    if (part) {
        const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
        const int32_t self = ka.exclude_self ? (int32_t)qi : -1;
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
                    if (!(d2 <= a.R2) || d2 > ld[K - 1])
                        continue;
                    const int32_t t = a.tidx_sorted[j];
                    if (t == self || !knn_before(d2, t, ld[K - 1], li[K - 1]))
                        continue;
                    // entry s takes its lower neighbour where the candidate goes before
                    // that, and the candidate where it goes before entry s only
#pragma unroll
                    for (int s = K - 1; s > 0; --s) {
                        const bool shift = knn_before(d2, t, ld[s - 1], li[s - 1]);
                        const bool here = knn_before(d2, t, ld[s], li[s]);
                        ld[s] = shift ? ld[s - 1] : (here ? d2 : ld[s]);
                        li[s] = shift ? li[s - 1] : (here ? t : li[s]);
                    }
                    if (knn_before(d2, t, ld[0], li[0])) {
                        ld[0] = d2;
                        li[0] = t;
                    }
                }
            }
    }
    int32_t n = 0;
    if (in) {
        int32_t *irow = a.index + qi * ka.k;
        float *drow = a.dist ? a.dist + qi * ka.k : nullptr;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < ka.k) {
                const bool real = li[s] != kKnnNone;
                n += real ? 1 : 0;
                irow[s] = real ? li[s] : -1;
                if (drow)
                    drow[s] = real ? (float)dpg::dvsqrt(ld[s]) : __builtin_huge_valf();
            }
        ka.count[qi] = n;
    }
    const uint32_t stripe = wave_stripe();
    wave_count<kCloudStripes, kCloudCounters>(a.count, 1, part ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 2, part && n == ka.k ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 3, part && n > 0 && n < ka.k ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 4, part && n == 0 ? 1ull : 0ull, stripe);
    wave_count<kCloudStripes, kCloudCounters>(a.count, 5, (unsigned long long)n, stripe);
}

// ---- dp_cloud_clean ---------------------------------------------------------------

constexpr int kCleanCounters = 5; // points (taking part), eligible, kept, removed_sparse, removed_far
constexpr int kCleanStripes = 64;
constexpr int64_t kCleanCopyBlocks = 1 << 20; // clean_copy_kernel's blocks, at most

struct CleanArgs {
    const char *points;
    int64_t n, stride;
    int32_t k, min_nb, radius_only, pad;
    double std_mul;
    const int32_t *rows, *rowcount;
    double *mean;
    CloudCleanDev *dev;
    int32_t *flag, *pos;
    uint8_t *keep;
    float *mean_dist; // optional
    int32_t *map;     // optional
    char *out;        // optional
    int64_t *n_out;   // optional
    unsigned long long *count; // kCleanStripes x kCleanCounters
};

__global__ __launch_bounds__(kMeshLanes) void clean_mean_kernel(CleanArgs a)
{
    const int64_t i = mesh_item();
    bool eligible = false;
    if (i < a.n) {
        const int32_t c = a.rowcount[i];
        double m = __builtin_huge_val();
        if (c > 0) {
            float p[3], t[3];
            load_point(a.points, a.stride, i, p);
            const int32_t *row = a.rows + i * a.k;
            double sum = 0.0;
            for (int32_t j = 0; j < c; ++j) {
                load_point(a.points, a.stride, row[j], t);
                const double dx = (double)p[0] - (double)t[0], dy = (double)p[1] - (double)t[1],
                             dz = (double)p[2] - (double)t[2];
                const double d = dpg::dvsqrt((dx * dx + dy * dy) + dz * dz);
                sum = j ? sum + d : d;
            }
            m = dpg::dvdiv(sum, (double)c);
        }
        a.mean[i] = m;
        if (a.mean_dist)
            a.mean_dist[i] = (float)m;
        eligible = c >= a.min_nb;
    }
    wave_count<kCleanStripes, kCleanCounters>(a.count, 1, eligible ? 1ull : 0ull, wave_stripe());
}

// one level of the pairwise sum over n terms: block b's 2^8 terms into dst[b].
// what = 0: the terms are src's; 1: x_i; 2: y_i (mu read from the device)
__global__ __launch_bounds__(kMeshLanes) void clean_sum_kernel(CleanArgs a, int what, const double *src, double *dst,
                                                               int64_t n)
{
    __shared__ double part[kMeshLanes / 64];
    const int64_t i = mesh_item();
    double v = 0.0;
    if (i < n) {
        if (what == 0) {
            v = src[i];
        } else if (a.rowcount[i] >= a.min_nb) {
            const double m = a.mean[i];
            if (what == 1) {
                v = m;
            } else {
                const double d = m - a.dev->mu;
                v = d * d;
            }
        }
    }
    for (int o = 1; o < 64; o <<= 1)
        v = v + __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = v;
    __syncthreads();
    static_assert(kMeshLanes == 256, "four waves: two more levels");
    if (threadIdx.x == 0)
        dst[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one lane.  phase 0: N and mu from S(x); phase 1: sigma and T from S(y).
// sum: the last level's one value, NULL for an empty cloud
__global__ __launch_bounds__(kMeshLanes) void clean_stat_kernel(CleanArgs a, int phase, const double *sum)
{
    if (threadIdx.x != 0)
        return;
    CloudCleanDev &d = *a.dev;
    const double S = sum ? *sum : 0.0;
    if (phase == 0) {
        unsigned long long N = 0;
        for (int st = 0; st < kCleanStripes; ++st)
            N += a.count[st * kCleanCounters + 1];
        d.eligible = (int64_t)N;
        d.mu = N > 0 ? dpg::dvdiv(S, (double)N) : 0.0;
        d.sigma = 0.0;
        d.threshold = 0.0;
    } else {
        const double var = d.eligible >= 2 ? dpg::dvdiv(S, (double)(d.eligible - 1)) : 0.0;
        d.sigma = dpg::dvsqrt(var);
        d.threshold = d.mu + a.std_mul * d.sigma;
    }
}

// over n + 1 items: the last one closes the scan's input
__global__ __launch_bounds__(kMeshLanes) void clean_keep_kernel(CleanArgs a)
{
    const int64_t i = mesh_item();
    bool part = false, eligible = false, keep = false;
    if (i < a.n) {
        float p[3];
        part = load_point(a.points, a.stride, i, p);
        eligible = a.rowcount[i] >= a.min_nb; // a point that does not take part has no row
        keep = eligible && (a.radius_only || a.mean[i] <= a.dev->threshold);
        a.keep[i] = keep ? 1 : 0;
        a.flag[i] = keep ? 1 : 0;
    } else if (i == a.n) {
        a.flag[i] = 0;
    }
    const uint32_t stripe = wave_stripe();
    wave_count<kCleanStripes, kCleanCounters>(a.count, 0, part ? 1ull : 0ull, stripe);
    wave_count<kCleanStripes, kCleanCounters>(a.count, 2, keep ? 1ull : 0ull, stripe);
    wave_count<kCleanStripes, kCleanCounters>(a.count, 3, part && !eligible ? 1ull : 0ull, stripe);
    wave_count<kCleanStripes, kCleanCounters>(a.count, 4, eligible && !keep ? 1ull : 0ull, stripe);
}

// over n + 1 items: the last one has the kept count
__global__ __launch_bounds__(kMeshLanes) void clean_map_kernel(CleanArgs a)
{
    const int64_t i = mesh_item();
    if (i < a.n) {
        if (a.map)
            a.map[i] = a.flag[i] ? a.pos[i] : -1;
    } else if (i == a.n) {
        a.dev->kept = a.pos[i];
        if (a.n_out)
            *a.n_out = a.pos[i];
    }
}

__global__ __launch_bounds__(kMeshLanes) void clean_copy_kernel(CleanArgs a)
{
    const int64_t words = a.stride >> 2, total = a.n * words;
    for (int64_t w = mesh_item(); w < total; w += (int64_t)gridDim.x * kMeshLanes) {
        const int64_t i = w / words, k = w - i * words;
        if (a.flag[i])
            ((uint32_t *)(a.out + (int64_t)a.pos[i] * a.stride))[k] = ((const uint32_t *)(a.points + i * a.stride))[k];
    }
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI: dp_cloud_knn
// ---------------------------------------------------------------------------

// the options both calls carry (they need no device)
static int knn_check_search(dp_ctx *c, const std::string &w, float max_dist, int32_t k)
{
    if (!(max_dist > 0.0f) || !std::isfinite(max_dist))
        return fail(c, DP_E_ARG, w + ": max_dist must be finite and > 0");
    if (k < 1 || k > 32)
        return fail(c, DP_E_ARG, w + ": k must be in 1..32");
    return DP_OK;
}

static int knn_check(dp_ctx *c, const std::string &w, const void *queries, int64_t nq, int64_t qstride,
                     const void *targets, int64_t nt, int64_t tstride, const dp_cloud_knn_options *o)
{
    int rc = cloud_check_clouds(c, w, queries, nq, qstride, targets, nt, tstride);
    if (rc != DP_OK)
        return rc;
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if ((rc = knn_check_search(c, w, o->max_dist, o->k)) != DP_OK)
        return rc;
    if (o->flags & ~DP_CLOUD_KNN_EXCLUDE_SELF)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    if ((o->flags & DP_CLOUD_KNN_EXCLUDE_SELF) && nq != nt)
        return fail(c, DP_E_ARG, w + ": DP_CLOUD_KNN_EXCLUDE_SELF needs n_queries == n_targets");
    return DP_OK;
}

// queues the search of device clouds on s (d_dist may be NULL: dp_cloud_clean's
// and dp_cloud_normals' searches); declared in dp_clouddev.h
int knn_queue(dp_ctx *c, const dp_cloud_knn_options &o, const void *d_queries, int64_t nq, int64_t qstride,
                     const void *d_targets, int64_t nt, int64_t tstride, int32_t *d_index, float *d_dist,
                     int32_t *d_count, hipStream_t s)
{
    dpk::KnnArgs ka{};
    dpk::CloudArgs &a = ka.g;
    a.targets = (const char *)d_targets;
    a.queries = (const char *)d_queries;
    a.nt = nt;
    a.nq = nq;
    a.tstride = tstride;
    a.qstride = qstride;
    a.R = (double)o.max_dist;
    a.R2 = (double)o.max_dist * (double)o.max_dist;
    a.index = d_index;
    a.dist = d_dist;
    int rc = cloud_targets_queue(c, a, s);
    if (rc != DP_OK || (rc = cloud_queries_queue(c, a, s)) != DP_OK)
        return rc;
    ka.k = o.k;
    ka.exclude_self = (o.flags & DP_CLOUD_KNN_EXCLUDE_SELF) ? 1 : 0;
    ka.count = d_count;
    const int64_t blocks = dpk::mesh_blocks(nq);
    if (o.k <= 8)
        DP_HIP(c, dpk::launch_over(dpk::knn_query_kernel<8>, blocks, ka, s));
    else if (o.k <= 16)
        DP_HIP(c, dpk::launch_over(dpk::knn_query_kernel<16>, blocks, ka, s));
    else
        DP_HIP(c, dpk::launch_over(dpk::knn_query_kernel<32>, blocks, ka, s));
    DP_HIP(c, c->cloudnearest.time[1].end(s));
    return DP_OK;
}

// the statistics read and its wait
static int knn_stats(dp_ctx *c, int64_t nq, int64_t nt, dp_cloud_knn_stats *stats, hipStream_t s)
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
    stats->full = r.count.sum(2);
    stats->partial = r.count.sum(3);
    stats->empty = r.count.sum(4);
    stats->neighbours = r.count.sum(5);
    stats->grid_cells = g->cells;
    stats->max_cell_targets = g->maxcell;
    DP_HIP(c, r.time[0].ms(stats->build_ms));
    DP_HIP(c, r.time[1].ms(stats->query_ms));
    return DP_OK;
}

extern "C" int dp_cloud_knn_device(dp_ctx *c, const void *d_queries, int64_t n_queries, int64_t query_stride,
                                   const void *d_targets, int64_t n_targets, int64_t target_stride,
                                   const dp_cloud_knn_options *opts, int32_t *d_index, float *d_dist,
                                   int32_t *d_count, dp_cloud_knn_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_knn_device";
    int rc = knn_check(c, w, d_queries, n_queries, query_stride, d_targets, n_targets, target_stride, opts);
    if (rc != DP_OK)
        return rc;
    if (n_queries > 0 && (!d_index || !d_dist || !d_count))
        return fail(c, DP_E_ARG, w + ": d_index, d_dist and d_count must be given");
    if ((rc = mesh_check_alias(c, w, {d_index, d_dist, d_count}, {d_queries, d_targets})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = knn_queue(c, *opts, d_queries, n_queries, query_stride, d_targets, n_targets, target_stride, d_index,
                        d_dist, d_count, s)) != DP_OK)
        return rc;
    return stats ? knn_stats(c, n_queries, n_targets, stats, s) : DP_OK;
}

extern "C" int dp_cloud_knn(dp_ctx *c, const void *queries, int64_t n_queries, int64_t query_stride,
                            const void *targets, int64_t n_targets, int64_t target_stride,
                            const dp_cloud_knn_options *opts, const int32_t **index, const float **dist,
                            const int32_t **count, dp_cloud_knn_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_knn";
    int rc = knn_check(c, w, queries, n_queries, query_stride, targets, n_targets, target_stride, opts);
    if (rc != DP_OK)
        return rc;
    if (!index || !dist || !count)
        return fail(c, DP_E_ARG, w + ": index, dist and count must be given");
    if ((rc = mesh_check_alias(c, w, {index, dist, count}, {queries, targets})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudKnnScratch &r = c->cloudknn;
    const int64_t nq = n_queries, nt = n_targets;
    const size_t row = 4 * (size_t)nq * (size_t)opts->k;
    // an array is staged from its first point to the end of its last
    const size_t qbytes = nq > 0 ? (size_t)(nq - 1) * (size_t)query_stride + 12 : 0;
    const size_t tbytes = nt > 0 ? (size_t)(nt - 1) * (size_t)target_stride + 12 : 0;
    PlanePacker pin, pout;
    const size_t iq = pin.add(qbytes), it = pin.add(tbytes);
    const size_t oi = pout.add(row), od = pout.add(row), oc = pout.add(4 * (size_t)nq);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hout.resize(std::max<size_t>(pout.total, 1)));
    if (nq > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + iq, queries, qbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + it, targets, tbytes, hipMemcpyHostToDevice, s));
    if ((rc = knn_queue(c, *opts, r.in.p + iq, nq, query_stride, r.in.p + it, nt, target_stride,
                        (int32_t *)(r.out.p + oi), (float *)(r.out.p + od), (int32_t *)(r.out.p + oc), s)) != DP_OK)
        return rc;
    if (nq > 0)
        DP_HIP(c, hipMemcpyAsync(r.hout.data(), r.out.p, pout.total, hipMemcpyDeviceToHost, s));
    if (stats) {
        if ((rc = knn_stats(c, nq, nt, stats, s)) != DP_OK)
            return rc;
    } else {
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *index = nq > 0 ? (const int32_t *)(r.hout.data() + oi) : nullptr;
    *dist = nq > 0 ? (const float *)(r.hout.data() + od) : nullptr;
    *count = nq > 0 ? (const int32_t *)(r.hout.data() + oc) : nullptr;
    return DP_OK;
}

// ---------------------------------------------------------------------------
// C ABI: dp_cloud_clean
// ---------------------------------------------------------------------------

static int clean_check(dp_ctx *c, const std::string &w, const void *points, int64_t n, int64_t stride,
                       const dp_cloud_clean_options *o)
{
    if (n < 0 || n > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n must be in 0..2^31 - 1");
    if (n > 0 && !points)
        return fail(c, DP_E_ARG, w + ": points must be given");
    if (stride < 12 || stride % 4)
        return fail(c, DP_E_ARG, w + ": stride must be a multiple of 4 and at least 12");
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    const int rc = knn_check_search(c, w, o->max_dist, o->k);
    if (rc != DP_OK)
        return rc;
    if (o->min_neighbours < 1 || o->min_neighbours > o->k)
        return fail(c, DP_E_ARG, w + ": min_neighbours must be in 1..k");
    if (!(o->std_mul >= 0.0f) || !std::isfinite(o->std_mul))
        return fail(c, DP_E_ARG, w + ": std_mul must be finite and >= 0");
    if (o->flags & ~DP_CLOUD_CLEAN_RADIUS_ONLY)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    return DP_OK;
}

// an output may be neither the input nor another output
static int clean_check_alias(dp_ctx *c, const std::string &w, const void *points, const void *keep, const void *mean,
                             const void *map, const void *out, const void *n_out)
{
    const void *o[5] = {keep, mean, map, out, n_out};
    for (int i = 0; i < 5; ++i) {
        if (!o[i])
            continue;
        if (o[i] == points)
            return fail(c, DP_E_ARG, w + ": an output pointer equals an input pointer");
        for (int j = 0; j < i; ++j)
            if (o[i] == o[j])
                return fail(c, DP_E_ARG, w + ": two output pointers are equal");
    }
    return DP_OK;
}

// queues the filter of a device cloud on s
static int clean_queue(dp_ctx *c, const dp_cloud_clean_options &o, const void *d_points, int64_t n, int64_t stride,
                       uint8_t *d_keep, float *d_mean_dist, int32_t *d_map, void *d_out, int64_t *d_n_out,
                       hipStream_t s)
{
    dpk::CloudKnnScratch &r = c->cloudknn;
    const size_t n1 = (size_t)n + 1;
    const int64_t b1 = dpk::mesh_blocks(n), b2 = dpk::mesh_blocks(b1);
    DP_HIP(c, r.rows.reserve(std::max<size_t>((size_t)n * (size_t)o.k, 1)));
    DP_HIP(c, r.rowcount.reserve(n1));
    DP_HIP(c, r.flag.reserve(n1));
    DP_HIP(c, r.pos.reserve(n1));
    DP_HIP(c, r.mean.reserve(n1));
    DP_HIP(c, r.sum[0].reserve((size_t)std::max<int64_t>(b1, 1)));
    DP_HIP(c, r.sum[1].reserve((size_t)std::max<int64_t>(b2, 1)));
    DP_HIP(c, r.dev.reserve(1));
    DP_HIP(c, r.count.reserve(dpk::kCleanStripes, dpk::kCleanCounters,
                              (sizeof(dpk::CloudGrid) + sizeof(dpk::CloudCleanDev) + 7) / 8));
    size_t scan_bytes = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, r.flag.p, r.pos.p, (int)n1, s));

    // before the search queues its sorts: cloud_targets_queue then only grows the buffer
    DP_HIP(c, c->scan_tmp.reserve(scan_bytes ? scan_bytes : 1));

    DP_HIP(c, r.time[0].begin(s));
    dp_cloud_knn_options ko{o.max_dist, o.k, DP_CLOUD_KNN_EXCLUDE_SELF};
    const int rc = knn_queue(c, ko, d_points, n, stride, d_points, n, stride, r.rows.p, nullptr, r.rowcount.p, s);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, r.time[0].end(s));

    dpk::CleanArgs a{};
    a.points = (const char *)d_points;
    a.n = n;
    a.stride = stride;
    a.k = o.k;
    a.min_nb = o.min_neighbours;
    a.radius_only = (o.flags & DP_CLOUD_CLEAN_RADIUS_ONLY) ? 1 : 0;
    a.std_mul = (double)o.std_mul;
    a.rows = r.rows.p;
    a.rowcount = r.rowcount.p;
    a.mean = r.mean.p;
    a.dev = r.dev.p;
    a.flag = r.flag.p;
    a.pos = r.pos.p;
    a.keep = d_keep;
    a.mean_dist = d_mean_dist;
    a.map = d_map;
    a.out = (char *)d_out;
    a.n_out = d_n_out;
    a.count = r.count.dev.p;

    DP_HIP(c, r.time[1].begin(s));
    DP_HIP(c, r.count.zero(s));
    DP_HIP(c, hipMemsetAsync(r.dev.p, 0, sizeof(dpk::CloudCleanDev), s));
    DP_HIP(c, dpk::launch_over(dpk::clean_mean_kernel, b1, a, s));
    if (!a.radius_only) {
        for (int what = 1; what <= 2; ++what) {
            // the levels: n terms, then a 2^8-th of them, until one is left
            const double *src = nullptr;
            int64_t terms = n;
            int into = 0;
            for (int first = what; terms > 0; first = 0) {
                const int64_t blocks = dpk::mesh_blocks(terms);
                hipLaunchKernelGGL(dpk::clean_sum_kernel, dim3((unsigned)blocks), dim3(dpk::kMeshLanes), 0, s, a, first, src,
                                   r.sum[into].p, terms);
                DP_HIP(c, hipGetLastError());
                src = r.sum[into].p;
                into ^= 1;
                if (blocks == 1)
                    break;
                terms = blocks;
            }
            hipLaunchKernelGGL(dpk::clean_stat_kernel, dim3(1), dim3(dpk::kMeshLanes), 0, s, a, what - 1, src);
            DP_HIP(c, hipGetLastError());
        }
    }
    DP_HIP(c, dpk::launch_over(dpk::clean_keep_kernel, dpk::mesh_blocks(n + 1), a, s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, scan_bytes, r.flag.p, r.pos.p, (int)n1, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_map_kernel, dpk::mesh_blocks(n + 1), a, s));
    if (a.out)
        DP_HIP(c, dpk::launch_over(dpk::clean_copy_kernel,
                                   std::min(dpk::mesh_blocks(n * (stride >> 2)), dpk::kCleanCopyBlocks), a, s));
    DP_HIP(c, r.time[1].end(s));
    return DP_OK;
}

// queues the read of the counters, the grid and the statistics block
static int clean_read(dp_ctx *c, hipStream_t s)
{
    dpk::CloudKnnScratch &r = c->cloudknn;
    char *extra = (char *)r.count.extra();
    DP_HIP(c, r.count.read(s));
    DP_HIP(c, hipMemcpyAsync(extra, c->cloudnearest.grid.p, sizeof(dpk::CloudGrid), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(extra + sizeof(dpk::CloudGrid), r.dev.p, sizeof(dpk::CloudCleanDev), hipMemcpyDeviceToHost,
                             s));
    return DP_OK;
}

// after the wait
static int clean_stats(dp_ctx *c, int64_t n, dp_cloud_clean_stats *stats)
{
    dpk::CloudKnnScratch &r = c->cloudknn;
    const char *extra = (const char *)r.count.extra();
    const dpk::CloudGrid *g = (const dpk::CloudGrid *)extra;
    const dpk::CloudCleanDev *d = (const dpk::CloudCleanDev *)(extra + sizeof(dpk::CloudGrid));
    stats->points = r.count.sum(0);
    stats->skipped = n - stats->points;
    stats->eligible = r.count.sum(1);
    stats->kept = r.count.sum(2);
    stats->removed_sparse = r.count.sum(3);
    stats->removed_far = r.count.sum(4);
    stats->grid_cells = g->cells;
    stats->max_cell_targets = g->maxcell;
    stats->mu = d->mu;
    stats->sigma = d->sigma;
    stats->threshold = d->threshold;
    DP_HIP(c, r.time[0].ms(stats->knn_ms));
    DP_HIP(c, r.time[1].ms(stats->clean_ms));
    return DP_OK;
}

extern "C" int dp_cloud_clean_device(dp_ctx *c, const void *d_points, int64_t n, int64_t stride,
                                     const dp_cloud_clean_options *opts, uint8_t *d_keep, float *d_mean_dist,
                                     int32_t *d_map, void *d_out, int64_t *d_n_out, dp_cloud_clean_stats *stats,
                                     void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_clean_device";
    int rc = clean_check(c, w, d_points, n, stride, opts);
    if (rc != DP_OK)
        return rc;
    if (n > 0 && !d_keep)
        return fail(c, DP_E_ARG, w + ": d_keep must be given");
    if ((rc = clean_check_alias(c, w, d_points, d_keep, d_mean_dist, d_map, d_out, d_n_out)) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = clean_queue(c, *opts, d_points, n, stride, d_keep, d_mean_dist, d_map, d_out, d_n_out, s)) != DP_OK)
        return rc;
    if (!stats)
        return DP_OK;
    if ((rc = clean_read(c, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    return clean_stats(c, n, stats);
}

extern "C" int dp_cloud_clean(dp_ctx *c, const void *points, int64_t n, int64_t stride,
                              const dp_cloud_clean_options *opts, const uint8_t **keep, const float **mean_dist,
                              const int32_t **map, const void **out, int64_t *n_out, dp_cloud_clean_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_clean";
    int rc = clean_check(c, w, points, n, stride, opts);
    if (rc != DP_OK)
        return rc;
    if (!keep)
        return fail(c, DP_E_ARG, w + ": keep must be given");
    if ((rc = clean_check_alias(c, w, points, keep, mean_dist, map, out, n_out)) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudKnnScratch &r = c->cloudknn;
    const size_t bytes = (size_t)n * (size_t)stride;
    PlanePacker pout;
    const size_t ok = pout.add((size_t)n), om = pout.add(mean_dist ? 4 * (size_t)n : 0),
                 op = pout.add(map ? 4 * (size_t)n : 0), oo = pout.add(out ? bytes : 0);
    DP_HIP(c, r.in.reserve(std::max<size_t>(bytes, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hout.resize(std::max<size_t>(pout.total, 1)));
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p, points, bytes, hipMemcpyHostToDevice, s));
    if ((rc = clean_queue(c, *opts, r.in.p, n, stride, (uint8_t *)(r.out.p + ok),
                          mean_dist ? (float *)(r.out.p + om) : nullptr, map ? (int32_t *)(r.out.p + op) : nullptr,
                          out ? r.out.p + oo : nullptr, nullptr, s)) != DP_OK)
        return rc;
    // the head of the results now; the records once the kept count is known
    const size_t head = out ? oo : pout.total;
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.hout.data(), r.out.p, head, hipMemcpyDeviceToHost, s));
    if ((rc = clean_read(c, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    const dpk::CloudCleanDev *d = (const dpk::CloudCleanDev *)((const char *)r.count.extra() + sizeof(dpk::CloudGrid));
    const int64_t kept = d->kept;
    if (out && kept > 0) {
        DP_HIP(c, hipMemcpyAsync(r.hout.data() + oo, r.out.p + oo, (size_t)kept * (size_t)stride, hipMemcpyDeviceToHost,
                                 s));
        DP_HIP(c, hipStreamSynchronize(s));
    }
    if (stats && (rc = clean_stats(c, n, stats)) != DP_OK)
        return rc;
    *keep = n > 0 ? r.hout.data() + ok : nullptr;
    if (mean_dist)
        *mean_dist = n > 0 ? (const float *)(r.hout.data() + om) : nullptr;
    if (map)
        *map = n > 0 ? (const int32_t *)(r.hout.data() + op) : nullptr;
    if (out)
        *out = kept > 0 ? r.hout.data() + oo : nullptr;
    if (n_out)
        *n_out = kept;
    return DP_OK;
}
