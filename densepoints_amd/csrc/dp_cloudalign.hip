// dp_cloudalign.hip -- the gfx950 kernels of the registration of one cloud to
// another and of the transform of a cloud's records (specs in
// include/densepoints.h, dp_cloud_align and dp_cloud_transform), and their C ABI.
//
// The search of every pass is dp_cloud_nearest's own: the grid over the targets
// is queued once (cloud_targets_queue), the queries' cell order and the walk once
// per pass (cloud_queries_queue, cloud_nearest_walk_queue; dp_clouddev.h), on the
// transformed source, so that c(i) and dist_i are that call's bit for bit.
//
//   align_transform_kernel  one lane per record: the record copied whole (unless
//                           in place, or into the packed scratch of a pass, which
//                           takes the position alone), the position and, when
//                           asked, the normal replaced.  M comes with the
//                           arguments (dp_cloud_transform) or from the device's
//                           state block (a pass).
//   align_targets_kernel    one lane: the targets taking part, kept aside before
//                           the passes zero the search's counters again
//   align_sum_kernel<C, W>  one level of 2^8 of C balanced pairwise sums at once
//                           (clean_sum_kernel's tree: xor shuffles 1, 2, .., 32
//                           inside a wave, the four waves through LDS, (w0 + w1) +
//                           (w2 + w3), +0.0 padding).  W = 1: the six terms of
//                           step 3; W = 2: the eleven of step 4; W = 0: the level
//                           below.  Channel c of level L is src[c * n + i]: one
//                           block makes all channels of its 2^8 items, reading
//                           the two points once.  Every index into the channel
//                           array is a compile-time constant: no scratch memory.
//   align_mean_kernel       one lane: m from the search's counters, the means
//   align_solve_kernel      one lane: the record, the verdict, Horn's N, the
//                           cyclic Jacobi sweeps with every matrix index a
//                           template argument (N and V stay in registers), the
//                           quaternion's rotation, scale and t, the new M
#include "dp_clouddev.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace dpk {
namespace {

constexpr int kAlignUpdated = -1; // the verdict of a step that replaced M

struct TransformArgs {
    const char *in;
    char *out;
    int64_t n, in_stride, out_stride;
    int64_t words;         // 4-byte words of a record to copy first (0: none)
    int64_t normal_offset; // -1: no normal
    double M[12];
    const double *dM; // the device's M when not NULL
};

struct AlignArgs {
    const char *source, *targets;
    int64_t n, sstride, tstride;
    const float *y;       // the transformed source, packed
    const int32_t *index; // c(i) of this pass
    CloudAlignDev *dev;
    const unsigned long long *count; // the search's counters (kCloudStripes x kCloudCounters)
    double rms_tol;
    int32_t min_pairs, scale_mode, step, final;
};

__device__ __forceinline__ bool finite_f64(double x) { return fabs(x) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(kMeshLanes) void align_transform_kernel(TransformArgs a)
{
    const int64_t i = mesh_item();
    if (i >= a.n)
        return;
    const char *rec = a.in + i * a.in_stride;
    char *dst = a.out + i * a.out_stride;
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k)
        M[k] = a.dM ? a.dM[k] : a.M[k];
    float p[3], nrm[3] = {0.0f, 0.0f, 0.0f};
    const bool part = load_point(rec, 0, 0, p);
    if (a.normal_offset >= 0)
        load_point(rec + a.normal_offset, 0, 0, nrm);
    for (int64_t w = 0; w < a.words; ++w)
        ((uint32_t *)dst)[w] = ((const uint32_t *)rec)[w];
    float *o = (float *)dst;
    if (part) {
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            o[r] = (float)(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3]);
    } else {
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
    }
    if (a.normal_offset >= 0) {
        const double x = (double)nrm[0], y = (double)nrm[1], z = (double)nrm[2];
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            v[r] = (M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z;
        const double len = dpg::dvsqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        if (finite_f64(len) && len > 0.0) {
            float *on = (float *)(dst + a.normal_offset);
#pragma unroll
            for (int r = 0; r < 3; ++r)
                on[r] = (float)dpg::dvdiv(v[r], len);
        }
    }
}

__global__ void align_targets_kernel(AlignArgs a)
{
    if (threadIdx.x != 0)
        return;
    unsigned long long t = 0;
    for (int st = 0; st < kCloudStripes; ++st)
        t += a.count[st * kCloudCounters + 0];
    a.dev->targets = (int64_t)t;
}

// one level of C pairwise sums over n terms: block b's 2^8 terms of channel c
// into dst[c * blocks + b]
template <int C, int WHAT>
__global__ __launch_bounds__(kMeshLanes) void align_sum_kernel(AlignArgs a, const double *src, double *dst, int64_t n)
{
    __shared__ double part[kMeshLanes / 64][C];
    const int64_t i = mesh_item();
    double v[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        v[ch] = 0.0;
    if (i < n) {
        if constexpr (WHAT == 0) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch)
                v[ch] = src[ch * n + i];
        } else {
            const int32_t who = a.index[i];
            if (who >= 0) {
                float xf[3], qf[3];
                load_point(a.source, a.sstride, i, xf);
                load_point(a.targets, a.tstride, who, qf);
                if constexpr (WHAT == 1) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        v[k] = (double)xf[k] + 0.0;
                        v[3 + k] = (double)qf[k] + 0.0;
                    }
                } else {
                    const CloudAlignDev &d = *a.dev;
                    double dx[3], dq[3], e[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        dx[k] = (double)xf[k] - d.mux[k];
                        dq[k] = (double)qf[k] - d.muq[k];
                        e[k] = (double)a.y[3 * i + k] - (double)qf[k];
                    }
#pragma unroll
                    for (int k = 0; k < 9; ++k)
                        v[k] = dx[k / 3] * dq[k % 3] + 0.0;
                    v[9] = ((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]) + 0.0;
                    v[10] = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        for (int o = 1; o < 64; o <<= 1)
            v[ch] = v[ch] + __shfl_xor(v[ch], o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
            part[threadIdx.x >> 6][ch] = v[ch];
    }
    __syncthreads();
    static_assert(kMeshLanes == 256, "four waves: two more levels");
    if (threadIdx.x < C) {
        const int ch = threadIdx.x;
        dst[(int64_t)ch * gridDim.x + blockIdx.x] = (part[0][ch] + part[1][ch]) + (part[2][ch] + part[3][ch]);
    }
}

// sum: the six sums of step 3, NULL for an empty source
__global__ void align_mean_kernel(AlignArgs a, const double *sum)
{
    if (threadIdx.x != 0)
        return;
    CloudAlignDev &d = *a.dev;
    unsigned long long m = 0;
    for (int st = 0; st < kCloudStripes; ++st)
        m += a.count[st * kCloudCounters + 2];
    d.matched = (int64_t)m;
    for (int k = 0; k < 3; ++k) {
        d.mux[k] = m > 0 && sum ? dpg::dvdiv(sum[k], (double)m) : 0.0;
        d.muq[k] = m > 0 && sum ? dpg::dvdiv(sum[3 + k], (double)m) : 0.0;
    }
}

// sum: the eleven sums of step 4, NULL for an empty source
__global__ void align_solve_kernel(AlignArgs a, const double *sum)
{
    if (threadIdx.x != 0)
        return;
    CloudAlignDev &d = *a.dev;
    const int64_t m = d.matched;
    double S[3][3], Sx = 0.0, E = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        S[k / 3][k % 3] = sum ? sum[k] : 0.0;
    if (sum) {
        Sx = sum[9];
        E = sum[10];
    }
    const double rms = m > 0 ? dpg::dvsqrt(dpg::dvdiv(E, (double)m)) : 0.0;
    d.rms = rms;
    int64_t verdict = kAlignUpdated;
    if (a.final)
        verdict = DP_CLOUD_ALIGN_STOP_ITERATIONS;
    else if (m < (int64_t)a.min_pairs)
        verdict = DP_CLOUD_ALIGN_STOP_PAIRS;
    else if (a.step > 0 && a.rms_tol > 0.0 && fabs(rms - d.rms_prev) <= a.rms_tol)
        verdict = DP_CLOUD_ALIGN_STOP_RMS;
    else if (Sx == 0.0)
        verdict = DP_CLOUD_ALIGN_STOP_DEGENERATE;
    d.rms_prev = rms;
    if (verdict != kAlignUpdated) {
        d.verdict = verdict;
        return;
    }
    double N[4][4], V[4][4];
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    N[0][1] = N[1][0] = S[1][2] - S[2][1];
    N[0][2] = N[2][0] = S[2][0] - S[0][2];
    N[0][3] = N[3][0] = S[0][1] - S[1][0];
    N[1][2] = N[2][1] = S[0][1] + S[1][0];
    N[1][3] = N[3][1] = S[2][0] + S[0][2];
    N[2][3] = N[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            V[r][k] = r == k ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < DP_CLOUD_ALIGN_SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(N, V);
        jacobi_rotate<0, 2>(N, V);
        jacobi_rotate<0, 3>(N, V);
        jacobi_rotate<1, 2>(N, V);
        jacobi_rotate<1, 3>(N, V);
        jacobi_rotate<2, 3>(N, V);
    }
    int j = 0;
    double top = N[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (N[k][k] > top) {
            top = N[k][k];
            j = k;
        }
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = j == 0 ? V[k][0] : (j == 1 ? V[k][1] : (j == 2 ? V[k][2] : V[k][3]));
    const double len = dpg::dvsqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
    const double q0 = dpg::dvdiv(v[0], len), q1 = dpg::dvdiv(v[1], len), q2 = dpg::dvdiv(v[2], len),
                 q3 = dpg::dvdiv(v[3], len);
    double R[3][3];
    R[0][0] = ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3;
    R[0][1] = 2.0 * (q1 * q2 - q0 * q3);
    R[0][2] = 2.0 * (q1 * q3 + q0 * q2);
    R[1][0] = 2.0 * (q1 * q2 + q0 * q3);
    R[1][1] = ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3;
    R[1][2] = 2.0 * (q2 * q3 - q0 * q1);
    R[2][0] = 2.0 * (q1 * q3 - q0 * q2);
    R[2][1] = 2.0 * (q2 * q3 + q0 * q1);
    R[2][2] = ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3;
    double scale = 1.0;
    if (a.scale_mode) {
        double g = R[0][0] * S[0][0];
#pragma unroll
        for (int k = 1; k < 9; ++k)
            g = g + R[k % 3][k / 3] * S[k / 3][k % 3];
        scale = dpg::dvdiv(g, Sx);
    }
    double M[12];
    bool good = finite_f64(scale) && scale > 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            M[4 * r + k] = scale * R[r][k];
        M[4 * r + 3] = d.muq[r] - ((M[4 * r] * d.mux[0] + M[4 * r + 1] * d.mux[1]) + M[4 * r + 2] * d.mux[2]);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k)
        good = good && finite_f64(M[k]);
    if (!good) {
        d.verdict = DP_CLOUD_ALIGN_STOP_DEGENERATE;
        return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k)
        d.M[k] = M[k];
    d.scale = scale;
    d.verdict = kAlignUpdated;
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI: dp_cloud_transform
// ---------------------------------------------------------------------------

static bool all_finite(const double *m, int n)
{
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(m[k]))
            return false;
    return true;
}

static int transform_check(dp_ctx *c, const std::string &w, const void *points, int64_t n, int64_t stride,
                           const double *matrix, int64_t normal_offset)
{
    if (n < 0 || n > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n must be in 0..2^31 - 1");
    if (n > 0 && !points)
        return fail(c, DP_E_ARG, w + ": points must be given");
    if (stride < 12 || stride % 4)
        return fail(c, DP_E_ARG, w + ": stride must be a multiple of 4 and at least 12");
    if (!matrix)
        return fail(c, DP_E_ARG, w + ": matrix must be given");
    if (!all_finite(matrix, 12))
        return fail(c, DP_E_ARG, w + ": matrix must be finite");
    if (normal_offset != -1 && (normal_offset < 12 || normal_offset % 4 || normal_offset > stride - 12))
        return fail(c, DP_E_ARG, w + ": normal_offset must be -1 or a multiple of 4 in 12..stride - 12");
    return DP_OK;
}

// queues the transform of device records on s; dM: the device's M instead of matrix
static int transform_queue(dp_ctx *c, const void *d_in, int64_t n, int64_t in_stride, void *d_out, int64_t out_stride,
                           bool whole, const double *matrix, const double *dM, int64_t normal_offset, hipStream_t s)
{
    dpk::TransformArgs a{};
    a.in = (const char *)d_in;
    a.out = (char *)d_out;
    a.n = n;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.words = whole && d_in != d_out ? in_stride >> 2 : 0;
    a.normal_offset = normal_offset;
    if (matrix)
        std::memcpy(a.M, matrix, sizeof a.M);
    a.dM = dM;
    DP_HIP(c, dpk::launch_over(dpk::align_transform_kernel, dpk::mesh_blocks(n), a, s));
    return DP_OK;
}

extern "C" int dp_cloud_transform_device(dp_ctx *c, const void *d_points, int64_t n, int64_t stride,
                                         const double *matrix, int64_t normal_offset, void *d_out, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_transform_device";
    const int rc = transform_check(c, w, d_points, n, stride, matrix, normal_offset);
    if (rc != DP_OK)
        return rc;
    if (n > 0 && !d_out)
        return fail(c, DP_E_ARG, w + ": d_out must be given");
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return transform_queue(c, d_points, n, stride, d_out, stride, true, matrix, nullptr, normal_offset, s);
}

extern "C" int dp_cloud_transform(dp_ctx *c, const void *points, int64_t n, int64_t stride, const double *matrix,
                                  int64_t normal_offset, const void **out)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_transform";
    int rc = transform_check(c, w, points, n, stride, matrix, normal_offset);
    if (rc != DP_OK)
        return rc;
    if (!out)
        return fail(c, DP_E_ARG, w + ": out must be given");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudAlignScratch &r = c->cloudalign;
    const size_t bytes = (size_t)n * (size_t)stride;
    DP_HIP(c, r.in.reserve(std::max<size_t>(bytes, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(bytes, 1)));
    DP_HIP(c, r.hout.resize(std::max<size_t>(bytes, 1)));
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p, points, bytes, hipMemcpyHostToDevice, s));
    if ((rc = transform_queue(c, r.in.p, n, stride, r.out.p, stride, true, matrix, nullptr, normal_offset, s)) != DP_OK)
        return rc;
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.hout.data(), r.out.p, bytes, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    *out = n > 0 ? r.hout.data() : nullptr;
    return DP_OK;
}

// ---------------------------------------------------------------------------
// C ABI: dp_cloud_align
// ---------------------------------------------------------------------------

static int align_check(dp_ctx *c, const std::string &w, const void *source, int64_t n, int64_t sstride,
                       const void *target, int64_t nt, int64_t tstride, const dp_cloud_align_options *o,
                       const double *init, const double *matrix, const double *scale,
                       const dp_cloud_align_step *trace)
{
    const int rc = cloud_check_clouds(c, w, source, n, sstride, target, nt, tstride);
    if (rc != DP_OK) // its messages call the source the queries
        return rc;
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if (!(o->max_dist > 0.0f) || !std::isfinite(o->max_dist))
        return fail(c, DP_E_ARG, w + ": max_dist must be finite and > 0");
    if (o->iterations < 1 || o->iterations > 1000)
        return fail(c, DP_E_ARG, w + ": iterations must be in 1..1000");
    if (o->min_pairs < 3)
        return fail(c, DP_E_ARG, w + ": min_pairs must be at least 3");
    if (!(o->rms_tol >= 0.0) || !std::isfinite(o->rms_tol))
        return fail(c, DP_E_ARG, w + ": rms_tol must be finite and >= 0");
    if (o->flags & ~DP_CLOUD_ALIGN_SCALE)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    if (init && !all_finite(init, 12))
        return fail(c, DP_E_ARG, w + ": init must be finite");
    if (!matrix || !scale || !trace)
        return fail(c, DP_E_ARG, w + ": matrix, scale and trace must be given");
    return DP_OK;
}

// one level after another of C sums over n terms; *out: where the C results are
// (NULL when n is 0)
template <int C, int WHAT>
static int align_sums_queue(dp_ctx *c, const dpk::AlignArgs &a, int64_t n, const double **out, hipStream_t s)
{
    dpk::CloudAlignScratch &r = c->cloudalign;
    const double *src = nullptr;
    int64_t terms = n;
    int into = 0;
    for (bool first = true; terms > 0; first = false) {
        const int64_t blocks = dpk::mesh_blocks(terms);
        if (first)
            hipLaunchKernelGGL((dpk::align_sum_kernel<C, WHAT>), dim3((unsigned)blocks), dim3(dpk::kMeshLanes), 0, s, a,
                               src, r.sum[into].p, terms);
        else
            hipLaunchKernelGGL((dpk::align_sum_kernel<C, 0>), dim3((unsigned)blocks), dim3(dpk::kMeshLanes), 0, s, a, src,
                               r.sum[into].p, terms);
        DP_HIP(c, hipGetLastError());
        src = r.sum[into].p;
        into ^= 1;
        if (blocks == 1)
            break;
        terms = blocks;
    }
    *out = src;
    return DP_OK;
}

// the whole call on device clouds: queues on s and waits once per pass
static int align_run(dp_ctx *c, const dp_cloud_align_options &o, const void *d_source, int64_t n, int64_t sstride,
                     const void *d_target, int64_t nt, int64_t tstride, const double *init, double *matrix,
                     double *scale, dp_cloud_align_step *trace, int32_t *d_index, float *d_dist,
                     dp_cloud_align_stats *stats, hipStream_t s)
{
    dpk::CloudAlignScratch &r = c->cloudalign;
    dpk::CloudNearestScratch &g = c->cloudnearest;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    const int64_t b1 = dpk::mesh_blocks(n), b2 = dpk::mesh_blocks(b1);
    DP_HIP(c, r.y.reserve(3 * n1));
    if (!d_index) {
        DP_HIP(c, r.index.reserve(n1));
        DP_HIP(c, r.dist.reserve(n1));
        d_index = r.index.p;
        d_dist = r.dist.p;
    }
    DP_HIP(c, r.sum[0].reserve(11 * (size_t)std::max<int64_t>(b1, 1)));
    DP_HIP(c, r.sum[1].reserve(11 * (size_t)std::max<int64_t>(b2, 1)));
    DP_HIP(c, r.dev.reserve(1));
    DP_HIP(c, r.hdev.resize(1));
    std::memset(trace, 0, sizeof(dp_cloud_align_step) * ((size_t)o.iterations + 1));

    dpk::CloudAlignDev &h = *r.hdev.data();
    std::memset(&h, 0, sizeof h);
    for (int k = 0; k < 12; ++k)
        h.M[k] = init ? init[k] : (k % 5 == 0 ? 1.0 : 0.0);
    h.scale = 1.0;
    h.verdict = dpk::kAlignUpdated;
    DP_HIP(c, hipMemcpyAsync(r.dev.p, &h, sizeof h, hipMemcpyHostToDevice, s));

    dpk::CloudArgs ca{};
    ca.targets = (const char *)d_target;
    ca.queries = (const char *)r.y.p;
    ca.nt = nt;
    ca.nq = n;
    ca.tstride = tstride;
    ca.qstride = 12;
    ca.R = (double)o.max_dist;
    ca.R2 = (double)o.max_dist * (double)o.max_dist;
    ca.index = d_index;
    ca.dist = d_dist;
    int rc = cloud_targets_queue(c, ca, s);
    if (rc != DP_OK)
        return rc;

    dpk::AlignArgs a{};
    a.source = (const char *)d_source;
    a.targets = (const char *)d_target;
    a.n = n;
    a.sstride = sstride;
    a.tstride = tstride;
    a.y = r.y.p;
    a.index = d_index;
    a.dev = r.dev.p;
    a.count = g.count.dev.p;
    a.rms_tol = o.rms_tol;
    a.min_pairs = o.min_pairs;
    a.scale_mode = (o.flags & DP_CLOUD_ALIGN_SCALE) ? 1 : 0;
    hipLaunchKernelGGL(dpk::align_targets_kernel, dim3(1), dim3(64), 0, s, a);
    DP_HIP(c, hipGetLastError());

    DP_HIP(c, r.time.begin(s));
    int64_t updates = 0, reason = DP_CLOUD_ALIGN_STOP_ITERATIONS;
    for (int k = 0; k <= o.iterations; ++k) {
        a.step = k;
        a.final = k == o.iterations ? 1 : 0;
        // steps 1 and 2
        if ((rc = transform_queue(c, d_source, n, sstride, r.y.p, 12, false, nullptr, r.dev.p->M, -1, s)) != DP_OK)
            return rc;
        DP_HIP(c, g.count.zero(s));
        if ((rc = cloud_queries_queue(c, ca, s)) != DP_OK || (rc = cloud_nearest_walk_queue(c, ca, s)) != DP_OK)
            return rc;
        // steps 3 to 6
        const double *sums = nullptr;
        if ((rc = align_sums_queue<6, 1>(c, a, n, &sums, s)) != DP_OK)
            return rc;
        hipLaunchKernelGGL(dpk::align_mean_kernel, dim3(1), dim3(64), 0, s, a, sums);
        DP_HIP(c, hipGetLastError());
        if ((rc = align_sums_queue<11, 2>(c, a, n, &sums, s)) != DP_OK)
            return rc;
        hipLaunchKernelGGL(dpk::align_solve_kernel, dim3(1), dim3(64), 0, s, a, sums);
        DP_HIP(c, hipGetLastError());
        // the record and the verdict
        DP_HIP(c, hipMemcpyAsync(&h.matched, &r.dev.p->matched, 24, hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipStreamSynchronize(s));
        trace[k].matched = h.matched;
        trace[k].rms = h.rms;
        if (h.verdict != dpk::kAlignUpdated) {
            reason = h.verdict;
            break;
        }
        ++updates;
    }
    DP_HIP(c, r.time.end(s));
    static_assert(offsetof(dpk::CloudAlignDev, verdict) - offsetof(dpk::CloudAlignDev, matched) == 16,
                  "the record and the verdict are read as one 24-byte block");

    DP_HIP(c, g.count.read(s));
    DP_HIP(c, hipMemcpyAsync(g.count.extra(), g.grid.p, sizeof(dpk::CloudGrid), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(&h, r.dev.p, sizeof h, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    std::memcpy(matrix, h.M, sizeof h.M);
    *scale = h.scale;
    if (stats) {
        const dpk::CloudGrid *grid = (const dpk::CloudGrid *)g.count.extra();
        stats->targets = h.targets;
        stats->queries = g.count.sum(1);
        stats->skipped_queries = n - stats->queries;
        stats->skipped_targets = nt - stats->targets;
        stats->matched = g.count.sum(2);
        stats->unmatched = g.count.sum(3);
        stats->grid_cells = grid->cells;
        stats->max_cell_targets = grid->maxcell;
        stats->iterations_run = updates;
        stats->stop_reason = n == 0 || nt == 0 ? DP_CLOUD_ALIGN_STOP_EMPTY : reason;
        DP_HIP(c, g.time[0].ms(stats->grid_ms));
        DP_HIP(c, r.time.ms(stats->iterate_ms));
    }
    return DP_OK;
}

extern "C" int dp_cloud_align_device(dp_ctx *c, const void *d_source, int64_t n_source, int64_t source_stride,
                                     const void *d_target, int64_t n_target, int64_t target_stride,
                                     const dp_cloud_align_options *opts, const double *init, double *matrix,
                                     double *scale, dp_cloud_align_step *trace, int32_t *d_index, float *d_dist,
                                     dp_cloud_align_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_align_device";
    int rc = align_check(c, w, d_source, n_source, source_stride, d_target, n_target, target_stride, opts, init, matrix,
                         scale, trace);
    if (rc != DP_OK)
        return rc;
    if (!d_index != !d_dist)
        return fail(c, DP_E_ARG, w + ": d_index and d_dist must be given together");
    if ((rc = mesh_check_alias(c, w, {matrix, scale, trace, d_index, d_dist}, {d_source, d_target, init})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return align_run(c, *opts, d_source, n_source, source_stride, d_target, n_target, target_stride, init, matrix, scale,
                     trace, d_index, d_dist, stats, s);
}

extern "C" int dp_cloud_align(dp_ctx *c, const void *source, int64_t n_source, int64_t source_stride,
                              const void *target, int64_t n_target, int64_t target_stride,
                              const dp_cloud_align_options *opts, const double *init, double *matrix, double *scale,
                              dp_cloud_align_step *trace, const int32_t **index, const float **dist,
                              dp_cloud_align_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_align";
    int rc = align_check(c, w, source, n_source, source_stride, target, n_target, target_stride, opts, init, matrix,
                         scale, trace);
    if (rc != DP_OK)
        return rc;
    if (!index != !dist)
        return fail(c, DP_E_ARG, w + ": index and dist must be given together");
    if ((rc = mesh_check_alias(c, w, {matrix, scale, trace, index, dist}, {source, target, init})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudAlignScratch &r = c->cloudalign;
    const int64_t n = n_source, nt = n_target;
    // an array is staged from its first point to the end of its last
    const size_t sbytes = n > 0 ? (size_t)(n - 1) * (size_t)source_stride + 12 : 0;
    const size_t tbytes = nt > 0 ? (size_t)(nt - 1) * (size_t)target_stride + 12 : 0;
    PlanePacker pin, pout;
    const size_t is = pin.add(sbytes), it = pin.add(tbytes);
    const size_t oi = pout.add(index ? 4 * (size_t)n : 0), od = pout.add(index ? 4 * (size_t)n : 0);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hout.resize(std::max<size_t>(pout.total, 1)));
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + is, source, sbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + it, target, tbytes, hipMemcpyHostToDevice, s));
    if ((rc = align_run(c, *opts, r.in.p + is, n, source_stride, r.in.p + it, nt, target_stride, init, matrix, scale,
                        trace, index ? (int32_t *)(r.out.p + oi) : nullptr, index ? (float *)(r.out.p + od) : nullptr,
                        stats, s)) != DP_OK)
        return rc;
    if (index) {
        if (n > 0) {
            DP_HIP(c, hipMemcpyAsync(r.hout.data(), r.out.p, pout.total, hipMemcpyDeviceToHost, s));
            DP_HIP(c, hipStreamSynchronize(s));
        }
        *index = n > 0 ? (const int32_t *)(r.hout.data() + oi) : nullptr;
        *dist = n > 0 ? (const float *)(r.hout.data() + od) : nullptr;
    }
    return DP_OK;
}
