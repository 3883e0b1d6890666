// dp_clouddev.h -- what the searches over a point cloud's uniform grid share
// (dp_cloudnearest.hip: one nearest target; dp_cloudknn.hip: the k nearest and
// the outlier filter on them; dp_cloudnormals.hip: the normals from them): the
// kernels' argument block, the guarded load of a point, the cell expression, the
// Jacobi rotation, and the host entries that queue the grid and the k-nearest
// search.  The grid kernels themselves (box, plan, keys, gather, begin, maxcell, query keys)
// and the margin proof live in dp_cloudnearest.hip, which exports
// cloud_targets_queue and cloud_queries_queue below; the searches (and
// dp_cloudalign.hip, which iterates one) use the scratch of c->cloudnearest,
// since their calls never overlap on a context.
#pragma once

#include "dp_meshdev.h"

namespace dpk {

// targets, queries (taking part); then dp_cloud_nearest: matched, unmatched;
// dp_cloud_knn: full, partial, empty, neighbours
constexpr int kCloudCounters = 6;
constexpr int kCloudStripes = 64;
constexpr int kCloudBoxBlocks = 1024; // cloud_box_kernel's blocks, at most
constexpr int kCloudCapMinBits = 16, kCloudCapMaxBits = 24;

struct CloudArgs {
    const char *targets, *queries;
    int64_t nt, nq, tstride, qstride;
    int32_t cap, nboxes; // the cell cap (a power of two); the boxes cloud_box_kernel wrote
    int32_t bins, pad;
    double R, R2; // (double)max_dist and its square
    float *boxes;
    CloudGrid *grid;
    uint32_t *tkeys, *tkeys_sorted, *qkeys, *qkeys_sorted;
    int32_t *tidx, *tidx_sorted, *qidx, *qidx_sorted, *begin;
    float *tx, *ty, *tz;
    int32_t *index;
    float *dist;
    unsigned long long *hist; // optional
    unsigned long long *count; // kCloudStripes x kCloudCounters
};

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }

// point i of an array; false unless its three floats are finite
__device__ __forceinline__ bool load_point(const char *base, int64_t stride, int64_t i, float p[3])
{
    const float *f = (const float *)(base + i * stride);
    p[0] = f[0];
    p[1] = f[1];
    p[2] = f[2];
    return finite_f32(p[0]) && finite_f32(p[1]) && finite_f32(p[2]);
}

// the cell coordinate of x on axis k, clamped to [lo, n + hi] in fp64 first: a
// coordinate of 1e30 must not reach the conversion
__device__ __forceinline__ int32_t cell_coord(const CloudGrid &g, int k, float x, double lo, double hi)
{
    double u = dpg::dvdiv((double)x - g.origin[k], g.cell[k]);
    u = fmin(fmax(u, lo), (double)g.n[k] + hi);
    return (int32_t)floor(u);
}

__device__ __forceinline__ uint32_t wave_stripe() { return blockIdx.x * (kMeshLanes / 64) + (threadIdx.x >> 6); }

// one rotation of the cyclic Jacobi of a symmetric D x D matrix held in
// registers (dp_cloud_align's 4 x 4 N, dp_cloud_normals' 3 x 3 scatter; the
// expressions are the header's): P, Q and D are compile-time, so every index is
// a constant and neither N nor V goes to scratch memory
template <int P, int Q, int D> __device__ __forceinline__ void jacobi_rotate(double (&N)[D][D], double (&V)[D][D])
{
    const double apq = N[P][Q];
    if (apq == 0.0)
        return;
    const double theta = dpg::dvdiv(N[Q][Q] - N[P][P], 2.0 * apq);
    const double t = dpg::dvdiv(theta >= 0.0 ? 1.0 : -1.0, fabs(theta) + dpg::dvsqrt(theta * theta + 1.0));
    const double c = dpg::dvdiv(1.0, dpg::dvsqrt(t * t + 1.0)), s = t * c;
#pragma unroll
    for (int k = 0; k < D; ++k)
        if (k != P && k != Q) {
            const double u = N[k][P], w = N[k][Q];
            N[k][P] = N[P][k] = c * u - s * w;
            N[k][Q] = N[Q][k] = s * u + c * w;
        }
    const double h = t * apq;
    N[P][P] = N[P][P] - h;
    N[Q][Q] = N[Q][Q] + h;
    N[P][Q] = N[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double u = V[k][P], w = V[k][Q];
        V[k][P] = c * u - s * w;
        V[k][Q] = s * u + c * w;
    }
}

} // namespace dpk

// The search but its walk, in two halves that a caller queues in this order on
// s, into the scratch of c->cloudnearest.  dp_cloud_nearest and dp_cloud_knn
// queue both once; dp_cloud_align queues the targets once and the queries once
// per pass.  (dp_cloudnearest.hip)
//
// cloud_targets_queue: reserves the scratch of both halves, zeroes the
// counters, queues the grid over the targets (timed by time[0]).  In: a's
// clouds, counts, strides, R and R2 (queries may still be NULL, nq is used for
// the sizes); out: its cap and every scratch pointer.  index, dist, hist and bins
// stay the caller's.
int cloud_targets_queue(dp_ctx *c, dpk::CloudArgs &a, hipStream_t s);
// cloud_queries_queue: time[1] begun (the caller ends it after its own query
// kernel), the queries' cell keys and their sort.  a as cloud_targets_queue
// left it, with queries and qstride set.
int cloud_queries_queue(dp_ctx *c, const dpk::CloudArgs &a, hipStream_t s);
// dp_cloud_nearest's walk (cloud_query_kernel) and the end of time[1]
int cloud_nearest_walk_queue(dp_ctx *c, const dpk::CloudArgs &a, hipStream_t s);

// dp_cloud_knn's whole search of device clouds, queued on s: both halves above,
// its walk (knn_query_kernel) and the end of time[1].  d_index: nq * o.k int32,
// d_count: nq int32, d_dist: nq * o.k f32 or NULL.  The options are the
// caller's to check.  (dp_cloudknn.hip; dp_cloud_clean and dp_cloudnormals.hip
// search a cloud against itself with it)
int knn_queue(dp_ctx *c, const dp_cloud_knn_options &o, const void *d_queries, int64_t nq, int64_t qstride,
              const void *d_targets, int64_t nt, int64_t tstride, int32_t *d_index, float *d_dist, int32_t *d_count,
              hipStream_t s);

// the counts, pointers and strides both searches check the same way
int cloud_check_clouds(dp_ctx *c, const std::string &w, const void *queries, int64_t nq, int64_t qstride,
                       const void *targets, int64_t nt, int64_t tstride);
