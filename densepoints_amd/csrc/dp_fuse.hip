// dp_fuse.hip -- gfx950 kernels of the depth-map fusion (spec in
// include/densepoints.h, dp_fuse_maps): every depth pixel of the requested
// views is back-projected and observed in the other views' depth maps; pixels
// that enough views agree with come out once, as the mean of the agreeing
// back-projections.
//
//   fuse_mask_kernel    one lane per pixel, a wave = 64 consecutive pixels of
//                       one plane; the loop over the other views is
//                       wave-uniform, so the view table (P, adjugate, plane
//                       pointers) is read with scalar loads; a wave without a
//                       depth leaves at once; one uint64 mask per depth pixel
//   fuse_count_kernel   fusable = popcount(mask) >= min_views; the suppression
//                       redoes the projection for the set bits below the
//                       pixel's own view only and reads the matched pixel's
//                       mask; one emitted flag per pixel, one count per block
//   (hipcub exclusive scan of the block counts; its last entry is the total)
//   fuse_emit_kernel    the records at the scanned offset plus the rank of the
//                       lane among the block's emitted pixels
//
// Blocks are numbered view-major and pixels are linear in a plane, so the
// output is in (k, y, x) order; the grids are sized from the plane sizes, which
// the host knows: no host read between the passes.  Every decision is a
// function of the planes and, for the suppression, of the pass-1 masks alone.
#include "dp_ctx.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

namespace dpk {
namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    const uint32_t lo = __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), lo);
}

__device__ __forceinline__ bool is_depth(float z) { return z > 0.0f && z <= 3.402823466e+38f; }

__device__ __forceinline__ void backproject(const FuseView &v, int x, int y, float z, double *X)
{
    const double zd = (double)z;
    const double b0 = zd * (double)x - v.P[3];
    const double b1 = zd * (double)y - v.P[7];
    const double b2 = zd - v.P[11];
    for (int j = 0; j < 3; ++j)
        X[j] = ((v.A[3 * j] * b0 + v.A[3 * j + 1] * b1) + v.A[3 * j + 2] * b2) / v.det;
}

// steps 1-4 of observe: the matched pixel of X in view s, its index and depth
__device__ __forceinline__ bool match(const FuseView &s, const double *X, double &d, int64_t &at, float &zs)
{
    d = ((s.P[8] * X[0] + s.P[9] * X[1]) + s.P[10] * X[2]) + s.P[11];
    if (!(d > 0.0))
        return false;
    const double h0 = ((s.P[0] * X[0] + s.P[1] * X[1]) + s.P[2] * X[2]) + s.P[3];
    const double h1 = ((s.P[4] * X[0] + s.P[5] * X[1]) + s.P[6] * X[2]) + s.P[7];
    double u, v;
    dpg::div2(h0, h1, d, u, v);
    if (!(fabs(u) < 2.0e9) || !(fabs(v) < 2.0e9))
        return false;
    const int32_t xi = (int32_t)rint(u), yi = (int32_t)rint(v);
    if (xi < 0 || xi >= s.W || yi < 0 || yi >= s.H)
        return false;
    at = (int64_t)yi * s.W + xi;
    zs = s.depth[at];
    return zs > 0.0f;
}

// steps 5-6 of observe
__device__ __forceinline__ bool agrees(const FuseArgs &a, const FuseView &s, double d, int64_t at, float zs,
                                       const double *nr)
{
    if (!(fabs((double)zs - d) <= a.tol * d))
        return false;
    if (!a.has_normals)
        return true;
    const double ns[3] = {(double)s.normal[3 * at], (double)s.normal[3 * at + 1], (double)s.normal[3 * at + 2]};
    const double c = dpg::dot3(nr, ns);
    return c >= 0.0 && c * c >= a.cos2 * (dpg::dot3(nr, nr) * dpg::dot3(ns, ns));
}

// one add per wave and counter, spread over kFuseStripes copies
__device__ __forceinline__ void wave_count(const FuseArgs &a, int counter, unsigned long long v, uint32_t stripe)
{
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(&a.count[(stripe & (kFuseStripes - 1)) * kFuseCounters + counter], v);
}

__global__ __launch_bounds__(kFuseBlock) void fuse_mask_kernel(FuseArgs a)
{
    const int k = blockIdx.y;
    const FuseView &r = a.tab[k];
    const int64_t npx = (int64_t)r.W * r.H;
    const int64_t i = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
    const float z = i < npx ? r.depth[i] : 0.0f;
    const bool part = is_depth(z);
    if (!__any(part))
        return;
    double X[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0};
    if (part) {
        backproject(r, (int)(i % r.W), (int)(i / r.W), z, X);
        if (a.has_normals)
            for (int j = 0; j < 3; ++j)
                nr[j] = (double)r.normal[3 * i + j];
    }
    uint64_t mask = 0;
    uint32_t matched = 0;
    for (int kp = 0; kp < a.K; ++kp) {
        if (kp == k)
            continue;
        const FuseView &s = a.tab[kp];
        double d;
        int64_t at;
        float zs;
        if (part && match(s, X, d, at, zs)) {
            ++matched;
            if (agrees(a, s, d, at, zs, nr))
                mask |= 1ull << kp;
        }
    }
    if (part)
        a.mask[r.poff + i] = mask;
    const uint32_t stripe = blockIdx.x * (kFuseBlock / 64) + (threadIdx.x >> 6);
    wave_count(a, 0, part ? 1ull : 0ull, stripe);
    wave_count(a, 1, (unsigned long long)matched, stripe);
    wave_count(a, 2, (unsigned long long)__popcll(mask), stripe);
}

__global__ __launch_bounds__(kFuseBlock) void fuse_count_kernel(FuseArgs a)
{
    __shared__ uint32_t wc[kFuseBlock / 64];
    const int k = blockIdx.y;
    const FuseView &r = a.tab[k];
    const int64_t npx = (int64_t)r.W * r.H;
    const int64_t i = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
    const float z = i < npx ? r.depth[i] : 0.0f;
    const bool part = is_depth(z);
    uint64_t lower = 0;
    bool fusable = false;
    if (part) {
        const uint64_t mask = a.mask[r.poff + i];
        fusable = __popcll(mask) >= a.min_views;
        if (fusable && !a.no_suppress)
            lower = mask & ((1ull << k) - 1ull);
    }
    bool emit = fusable;
    if (__any(lower != 0)) {
        double X[3] = {0.0, 0.0, 0.0};
        if (lower)
            backproject(r, (int)(i % r.W), (int)(i / r.W), z, X);
        for (int kp = 0; kp < k; ++kp) {
            const bool bit = (lower >> kp) & 1ull;
            if (!__any(bit))
                continue;
            const FuseView &s = a.tab[kp];
            double d;
            int64_t at;
            float zs;
            // a set bit's pixel matched in pass 1, by the same arithmetic
            if (bit && match(s, X, d, at, zs) && __popcll(a.mask[s.poff + at]) >= a.min_views)
                emit = false;
        }
    }
    if (i < npx)
        a.flag[r.poff + i] = emit ? 1 : 0;
    const uint64_t m = __ballot(emit);
    if ((threadIdx.x & 63) == 0)
        wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kFuseBlock / 64; ++w)
            t += wc[w];
        a.bcount[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
    wave_count(a, 3, fusable ? 1ull : 0ull, blockIdx.x * (kFuseBlock / 64) + (threadIdx.x >> 6));
}

__global__ __launch_bounds__(kFuseBlock) void fuse_emit_kernel(FuseArgs a)
{
    __shared__ uint32_t wc[kFuseBlock / 64];
    const int k = blockIdx.y;
    const FuseView &r = a.tab[k];
    const int64_t npx = (int64_t)r.W * r.H;
    const int64_t i = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
    const bool emit = i < npx && a.flag[r.poff + i];
    const uint64_t m = __ballot(emit);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        wc[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!m)
        return;
    int64_t at_out = (int64_t)a.boff[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] + lanes_below(m);
    for (int w = 0; w < wv; ++w)
        at_out += wc[w];
    const bool writes = emit && at_out < a.cap;
    if (!__any(writes))
        return;
    const int x = (int)(i % r.W), y = (int)(i / r.W);
    double acc[3] = {0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
    uint64_t mask = 0;
    if (writes) {
        backproject(r, x, y, r.depth[i], X);
        mask = a.mask[r.poff + i];
        for (int j = 0; j < 3; ++j) {
            acc[j] = X[j];
            if (a.has_normals)
                sum[j] = (double)r.normal[3 * i + j];
        }
    }
    for (int kp = 0; kp < a.K; ++kp) {
        const bool bit = (mask >> kp) & 1ull;
        if (!__any(bit))
            continue;
        const FuseView &s = a.tab[kp];
        double d;
        int64_t at;
        float zs;
        if (bit && match(s, X, d, at, zs)) {
            double Y[3];
            backproject(s, (int)(at % s.W), (int)(at / s.W), zs, Y);
            for (int j = 0; j < 3; ++j) {
                acc[j] += Y[j];
                if (a.has_normals)
                    sum[j] += (double)s.normal[3 * at + j];
            }
        }
    }
    if (!writes)
        return;
    const int nv = 1 + __popcll(mask);
    dp_fused_point p;
    const double q = dpg::dot3(sum, sum);
    const double len = q > 0.0 ? sqrt(q) : 1.0;
    for (int j = 0; j < 3; ++j) {
        p.pos[j] = (float)(acc[j] / (double)nv);
        p.normal[j] = q > 0.0 ? (float)(sum[j] / len) : 0.0f;
    }
    const uint32_t px = r.img[(int64_t)y * r.pitch + x];
    p.rgb[0] = (uint8_t)(px >> 16);
    p.rgb[1] = (uint8_t)(px >> 8);
    p.rgb[2] = (uint8_t)px;
    p.n_views = (uint8_t)nv;
    p.view = r.view;
    p.x = x;
    p.y = y;
    a.out[at_out] = p;
}

} // namespace

hipError_t launch_fuse_mask(const FuseArgs &a, unsigned gx, hipStream_t s)
{
    hipLaunchKernelGGL(fuse_mask_kernel, dim3(gx, (unsigned)a.K), dim3(kFuseBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fuse_count(const FuseArgs &a, unsigned gx, hipStream_t s)
{
    hipLaunchKernelGGL(fuse_count_kernel, dim3(gx, (unsigned)a.K), dim3(kFuseBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fuse_emit(const FuseArgs &a, unsigned gx, hipStream_t s)
{
    hipLaunchKernelGGL(fuse_emit_kernel, dim3(gx, (unsigned)a.K), dim3(kFuseBlock), 0, s, a);
    return hipGetLastError();
}

} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_fuse_options(dp_fuse_options *fo)
{
    if (!fo)
        return;
    fo->depth_tol = 0.01f;
    fo->min_views = 2;
    fo->min_normal_cos = 0.5f;
    fo->flags = 0;
}

// argument checks shared by both forms (they need no device)
static int fuse_check(dp_ctx *c, const int32_t *views, int n_views, const dp_fuse_options &o,
                      const float *const *depth, const float *const *normal, const void *n_out)
{
    if (!c)
        return DP_E_ARG;
    if (!(o.depth_tol >= 0.0f) || !std::isfinite(o.depth_tol))
        return fail(c, DP_E_ARG, "dp_fuse_maps: depth_tol must be finite and >= 0");
    if (o.min_views < 0 || o.min_views > 63)
        return fail(c, DP_E_ARG, "dp_fuse_maps: min_views must be in 0..63");
    if (!(o.min_normal_cos >= 0.0f && o.min_normal_cos <= 1.0f))
        return fail(c, DP_E_ARG, "dp_fuse_maps: min_normal_cos must be in 0..1");
    if (!n_out)
        return fail(c, DP_E_ARG, "dp_fuse_maps: n_out must be given");
    if (c->V <= 0)
        return fail(c, DP_E_STATE, "dp_fuse_maps: no views set");
    if (!views || n_views < 1 || n_views > c->V || n_views > 64)
        return fail(c, DP_E_ARG, "dp_fuse_maps: n_views must be in 1..min(V, 64)");
    uint64_t seen[2] = {0, 0};
    for (int k = 0; k < n_views; ++k) {
        const int32_t v = views[k];
        if (v < 0 || v >= c->V || ((seen[v >> 6] >> (v & 63)) & 1ull))
            return fail(c, DP_E_ARG, "dp_fuse_maps: view ids must be unique and < V");
        seen[v >> 6] |= 1ull << (v & 63);
    }
    if (!depth)
        return fail(c, DP_E_ARG, "dp_fuse_maps: depth planes must be given");
    for (int k = 0; k < n_views; ++k)
        if (!depth[k] || (normal && !normal[k]))
            return fail(c, DP_E_ARG, "dp_fuse_maps: a plane pointer is NULL");
    return DP_OK;
}

// the view table entry of the spec: adjugate and determinant of the left 3x3
static bool fuse_view(const dpg::ViewDev &v, dpk::FuseView &t)
{
    const double *P = v.P;
    const double h[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    for (int j = 0; j < 12; ++j)
        t.P[j] = P[j];
    t.A[0] = h[4] * h[8] - h[5] * h[7];
    t.A[1] = h[2] * h[7] - h[1] * h[8];
    t.A[2] = h[1] * h[5] - h[2] * h[4];
    t.A[3] = h[5] * h[6] - h[3] * h[8];
    t.A[4] = h[0] * h[8] - h[2] * h[6];
    t.A[5] = h[2] * h[3] - h[0] * h[5];
    t.A[6] = h[3] * h[7] - h[4] * h[6];
    t.A[7] = h[1] * h[6] - h[0] * h[7];
    t.A[8] = h[0] * h[4] - h[1] * h[3];
    t.det = (h[0] * t.A[0] + h[1] * t.A[3]) + h[2] * t.A[6];
    t.W = v.W;
    t.H = v.H;
    t.pitch = v.pitch;
    t.img = v.img;
    return t.det != 0.0 && std::isfinite(t.det);
}

extern "C" int dp_fuse_maps_device(dp_ctx *c, const int32_t *views, int n_views, const dp_fuse_options *fo,
                                   const float *const *d_depth, const float *const *d_normal,
                                   dp_fused_point *d_points, int64_t cap, int64_t *n_out, dp_fuse_stats *stats,
                                   void *stream)
{
    dp_fuse_options o;
    dp_default_fuse_options(&o);
    if (fo)
        o = *fo;
    int rc = fuse_check(c, views, n_views, o, d_depth, d_normal, n_out);
    if (rc != DP_OK)
        return rc;
    if (cap < 0 || (cap > 0 && !d_points))
        return fail(c, DP_E_ARG, "dp_fuse_maps_device: cap must be >= 0, with d_points given when > 0");
    std::vector<dpk::FuseView> tab((size_t)n_views);
    int64_t pixels = 0, max_px = 0;
    for (int k = 0; k < n_views; ++k) {
        dpk::FuseView &t = tab[(size_t)k];
        if (!fuse_view(c->hv[views[k]], t))
            return fail(c, DP_E_ARG, "dp_fuse_maps: a requested view's left 3x3 is singular");
        t.view = views[k];
        t.depth = d_depth[k];
        t.normal = d_normal ? d_normal[k] : nullptr;
        t.poff = pixels;
        const int64_t px = (int64_t)t.W * t.H;
        if (px > 0x7FFFFFFFll)
            return fail(c, DP_E_ARG, "dp_fuse_maps: view too large");
        pixels += px;
        max_px = std::max(max_px, px);
    }
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DP_HIP(c, c->u_e0.create());
    DP_HIP(c, c->u_e1.create());
    const unsigned gx = (unsigned)std::max<int64_t>((max_px + dpk::kFuseBlock - 1) / dpk::kFuseBlock, 1);
    const int64_t blocks = (int64_t)gx * n_views;
    if (blocks > 0x7FFFFFFFll - 1)
        return fail(c, DP_E_ARG, "dp_fuse_maps: too many pixels");
    const size_t ncount = (size_t)dpk::kFuseStripes * dpk::kFuseCounters;
    DP_HIP(c, c->r_z.reserve((size_t)std::max<int64_t>(pixels, 1)));
    DP_HIP(c, c->u_flag.reserve((size_t)std::max<int64_t>(pixels, 1)));
    DP_HIP(c, c->u_bcount.reserve((size_t)blocks + 1));
    DP_HIP(c, c->u_boff.reserve((size_t)blocks + 1));
    DP_HIP(c, c->u_count.reserve(ncount));
    DP_HIP(c, c->u_tab.reserve((size_t)n_views));
    DP_HIP(c, c->u_hcount.resize(ncount + 1));
    size_t scan_bytes = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, c->u_bcount.p, c->u_boff.p, (int)(blocks + 1), s));
    DP_HIP(c, c->scan_tmp.reserve(scan_bytes ? scan_bytes : 1));

    dpk::FuseArgs a{};
    a.tab = c->u_tab.p;
    a.K = n_views;
    a.min_views = o.min_views;
    a.no_suppress = (o.flags & DP_FUSE_NO_SUPPRESS) ? 1 : 0;
    a.has_normals = d_normal ? 1 : 0;
    a.tol = (double)o.depth_tol;
    a.cos2 = (double)o.min_normal_cos * (double)o.min_normal_cos;
    a.mask = c->r_z.p;
    a.flag = c->u_flag.p;
    a.bcount = c->u_bcount.p;
    a.boff = c->u_boff.p;
    a.count = c->u_count.p;
    a.out = d_points;
    a.cap = cap;

    // the table is a small pageable copy: staged before the call returns
    DP_HIP(c, hipMemcpyAsync(c->u_tab.p, tab.data(), sizeof(dpk::FuseView) * tab.size(), hipMemcpyHostToDevice, s));
    DP_HIP(c, hipEventRecord(c->u_e0, s));
    DP_HIP(c, hipMemsetAsync(c->u_count.p, 0, sizeof(unsigned long long) * ncount, s));
    DP_HIP(c, hipMemsetAsync(c->u_bcount.p + blocks, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_fuse_mask(a, gx, s));
    DP_HIP(c, dpk::launch_fuse_count(a, gx, s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, scan_bytes, c->u_bcount.p, c->u_boff.p,
                                               (int)(blocks + 1), s));
    DP_HIP(c, dpk::launch_fuse_emit(a, gx, s));
    DP_HIP(c, hipEventRecord(c->u_e1, s));
    // the one wait: the counters and the scan's total
    unsigned long long *h = c->u_hcount.data();
    DP_HIP(c, hipMemcpyAsync(h, c->u_count.p, sizeof(unsigned long long) * ncount, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + ncount, c->u_boff.p + blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    *n_out = (int64_t)h[ncount];
    if (stats) {
        int64_t sum[dpk::kFuseCounters] = {0, 0, 0, 0};
        for (int st = 0; st < dpk::kFuseStripes; ++st)
            for (int k = 0; k < dpk::kFuseCounters; ++k)
                sum[k] += (int64_t)h[st * dpk::kFuseCounters + k];
        float ms = 0.0f;
        DP_HIP(c, hipEventElapsedTime(&ms, c->u_e0, c->u_e1));
        stats->depth_pixels = sum[0];
        stats->matched_pairs = sum[1];
        stats->consistent_pairs = sum[2];
        stats->fusable = sum[3];
        stats->emitted = *n_out;
        stats->fuse_ms = (double)ms;
    }
    return DP_OK;
}

extern "C" int dp_fuse_maps(dp_ctx *c, const int32_t *views, int n_views, const dp_fuse_options *fo,
                            const float *const *depth, const float *const *normal, const dp_fused_point **out,
                            int64_t *n_out, dp_fuse_stats *stats)
{
    dp_fuse_options o;
    dp_default_fuse_options(&o);
    if (fo)
        o = *fo;
    int rc = fuse_check(c, views, n_views, o, depth, normal, n_out);
    if (rc != DP_OK)
        return rc;
    if (!out)
        return fail(c, DP_E_ARG, "dp_fuse_maps: out must be given");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // device copies of the planes, 256-B aligned, in one buffer; a pixel that
    // holds no depth cannot be emitted, which bounds the point buffer
    std::vector<size_t> od((size_t)n_views), on((size_t)n_views);
    std::vector<int64_t> nd((size_t)n_views, 0);
    size_t total = 0;
    for (int k = 0; k < n_views; ++k) {
        const size_t px = (size_t)c->hv[views[k]].W * (size_t)c->hv[views[k]].H;
        od[(size_t)k] = total;
        total += (4 * px + 255) & ~(size_t)255;
        if (normal) {
            on[(size_t)k] = total;
            total += (12 * px + 255) & ~(size_t)255;
        }
    }
    parallel_for(n_views, [&](int64_t k) {
        const int64_t px = (int64_t)c->hv[views[k]].W * c->hv[views[k]].H;
        const float *z = depth[k];
        int64_t n = 0;
        for (int64_t i = 0; i < px; ++i)
            n += z[i] > 0.0f && z[i] <= 3.402823466e+38f;
        nd[(size_t)k] = n;
    });
    int64_t cap = 0;
    for (int64_t n : nd)
        cap += n;
    DP_HIP(c, c->u_in.reserve(total ? total : 1));
    DP_HIP(c, c->u_pts.reserve((size_t)std::max<int64_t>(cap, 1)));
    std::vector<const float *> dd((size_t)n_views), dn((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const size_t px = (size_t)c->hv[views[k]].W * (size_t)c->hv[views[k]].H;
        dd[(size_t)k] = (const float *)(c->u_in.p + od[(size_t)k]);
        DP_HIP(c, hipMemcpyAsync(c->u_in.p + od[(size_t)k], depth[k], 4 * px, hipMemcpyHostToDevice, s));
        if (normal) {
            dn[(size_t)k] = (const float *)(c->u_in.p + on[(size_t)k]);
            DP_HIP(c, hipMemcpyAsync(c->u_in.p + on[(size_t)k], normal[k], 12 * px, hipMemcpyHostToDevice, s));
        }
    }
    int64_t n = 0;
    rc = dp_fuse_maps_device(c, views, n_views, &o, dd.data(), normal ? dn.data() : nullptr, c->u_pts.p, cap, &n,
                             stats, s);
    if (rc != DP_OK)
        return rc;
    if (n > cap)
        return fail(c, DP_E_HIP, "dp_fuse_maps: more points than depth pixels");
    DP_HIP(c, c->u_res.resize((size_t)std::max<int64_t>(n, 1)));
    if (n > 0) {
        DP_HIP(c, hipMemcpyAsync(c->u_res.data(), c->u_pts.p, sizeof(dp_fused_point) * (size_t)n,
                                 hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *out = n > 0 ? c->u_res.data() : nullptr;
    *n_out = n;
    return DP_OK;
}
