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
#include "dp_mapdev.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

namespace dpk {
namespace {

// steps 1-4 of observe: the matched pixel of X in view s, its index and depth
__device__ __forceinline__ bool match(const FuseView &s, const double *X, double &d, int64_t &at, float &zs)
{
    int32_t xi, yi;
    if (!nearest_pixel(s.inv.P, s.W, s.H, X, d, xi, yi))
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
        backproject(r.inv, (double)(int)(i % r.W), (double)(int)(i / r.W), (double)z, X);
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
    wave_count<kFuseStripes, kFuseCounters>(a.count, 0, part ? 1ull : 0ull, stripe);
    wave_count<kFuseStripes, kFuseCounters>(a.count, 1, (unsigned long long)matched, stripe);
    wave_count<kFuseStripes, kFuseCounters>(a.count, 2, (unsigned long long)__popcll(mask), stripe);
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
            backproject(r.inv, (double)(int)(i % r.W), (double)(int)(i / r.W), (double)z, X);
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
    const uint32_t stripe = blockIdx.x * (kFuseBlock / 64) + (threadIdx.x >> 6);
    wave_count<kFuseStripes, kFuseCounters>(a.count, 3, fusable ? 1ull : 0ull, stripe);
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
        backproject(r.inv, (double)x, (double)y, (double)r.depth[i], X);
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
            backproject(s.inv, (double)(int)(at % s.W), (double)(int)(at / s.W), (double)zs, Y);
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
    const int rc = check_view_list(c, "dp_fuse_maps", views, n_views, 64);
    if (rc != DP_OK)
        return rc;
    if (!depth)
        return fail(c, DP_E_ARG, "dp_fuse_maps: depth planes must be given");
    for (int k = 0; k < n_views; ++k)
        if (!depth[k] || (normal && !normal[k]))
            return fail(c, DP_E_ARG, "dp_fuse_maps: a plane pointer is NULL");
    return DP_OK;
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
        const dpg::ViewDev &v = c->hv[views[k]];
        if (!view_inverse(v, t.inv))
            return fail(c, DP_E_ARG, "dp_fuse_maps: a requested view's left 3x3 is singular");
        t.W = v.W;
        t.H = v.H;
        t.pitch = v.pitch;
        t.img = v.img;
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
    const unsigned gx = (unsigned)std::max<int64_t>((max_px + dpk::kFuseBlock - 1) / dpk::kFuseBlock, 1);
    const int64_t blocks = (int64_t)gx * n_views;
    if (blocks > 0x7FFFFFFFll - 1)
        return fail(c, DP_E_ARG, "dp_fuse_maps: too many pixels");
    DP_HIP(c, c->pix64.reserve((size_t)std::max<int64_t>(pixels, 1)));
    DP_HIP(c, c->fuse.flag.reserve((size_t)std::max<int64_t>(pixels, 1)));
    DP_HIP(c, c->fuse.bcount.reserve((size_t)blocks + 1));
    DP_HIP(c, c->fuse.boff.reserve((size_t)blocks + 1));
    DP_HIP(c, c->fuse.count.reserve(dpk::kFuseStripes, dpk::kFuseCounters, 1));
    DP_HIP(c, c->fuse.tab.reserve((size_t)n_views));
    size_t scan_bytes = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, c->fuse.bcount.p, c->fuse.boff.p, (int)(blocks + 1),
                                               s));
    DP_HIP(c, c->scan_tmp.reserve(scan_bytes ? scan_bytes : 1));

    dpk::FuseArgs a{};
    a.tab = c->fuse.tab.p;
    a.K = n_views;
    a.min_views = o.min_views;
    a.no_suppress = (o.flags & DP_FUSE_NO_SUPPRESS) ? 1 : 0;
    a.has_normals = d_normal ? 1 : 0;
    a.tol = (double)o.depth_tol;
    a.cos2 = (double)o.min_normal_cos * (double)o.min_normal_cos;
    a.mask = c->pix64.p;
    a.flag = c->fuse.flag.p;
    a.bcount = c->fuse.bcount.p;
    a.boff = c->fuse.boff.p;
    a.count = c->fuse.count.dev.p;
    a.out = d_points;
    a.cap = cap;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the table is read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(c->fuse.tab.p, tab.data(), sizeof(dpk::FuseView) * tab.size(), hipMemcpyHostToDevice, s));
    DP_HIP(c, c->fuse.time.begin(s));
    DP_HIP(c, c->fuse.count.zero(s));
    DP_HIP(c, hipMemsetAsync(c->fuse.bcount.p + blocks, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_fuse_mask(a, gx, s));
    DP_HIP(c, dpk::launch_fuse_count(a, gx, s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, scan_bytes, c->fuse.bcount.p, c->fuse.boff.p,
                                               (int)(blocks + 1), s));
    DP_HIP(c, dpk::launch_fuse_emit(a, gx, s));
    DP_HIP(c, c->fuse.time.end(s));
    // the one wait: the counters and the scan's total
    StripedCounters &n = c->fuse.count;
    DP_HIP(c, n.read(s));
    DP_HIP(c, hipMemcpyAsync(n.extra(), c->fuse.boff.p + blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    *n_out = (int64_t)n.extra()[0];
    if (stats) {
        stats->depth_pixels = n.sum(0);
        stats->matched_pairs = n.sum(1);
        stats->consistent_pairs = n.sum(2);
        stats->fusable = n.sum(3);
        stats->emitted = *n_out;
        DP_HIP(c, c->fuse.time.ms(stats->fuse_ms));
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
    PlanePacker pack;
    for (int k = 0; k < n_views; ++k) {
        od[(size_t)k] = pack.add(4 * view_pixels(c, views[k]));
        if (normal)
            on[(size_t)k] = pack.add(12 * view_pixels(c, views[k]));
    }
    parallel_for(n_views, [&](int64_t k) {
        const size_t px = view_pixels(c, views[k]);
        const float *z = depth[k];
        int64_t n = 0;
        for (size_t i = 0; i < px; ++i)
            n += dpk::is_depth(z[i]);
        nd[(size_t)k] = n;
    });
    int64_t cap = 0;
    for (int64_t n : nd)
        cap += n;
    DP_HIP(c, c->fuse.in.reserve(pack.total ? pack.total : 1));
    DP_HIP(c, c->fuse.pts.reserve((size_t)std::max<int64_t>(cap, 1)));
    std::vector<const float *> dd((size_t)n_views), dn((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        dd[(size_t)k] = (const float *)(c->fuse.in.p + od[(size_t)k]);
        DP_HIP(c, hipMemcpyAsync(c->fuse.in.p + od[(size_t)k], depth[k], 4 * px, hipMemcpyHostToDevice, s));
        if (normal) {
            dn[(size_t)k] = (const float *)(c->fuse.in.p + on[(size_t)k]);
            DP_HIP(c, hipMemcpyAsync(c->fuse.in.p + on[(size_t)k], normal[k], 12 * px, hipMemcpyHostToDevice, s));
        }
    }
    int64_t n = 0;
    rc = dp_fuse_maps_device(c, views, n_views, &o, dd.data(), normal ? dn.data() : nullptr, c->fuse.pts.p, cap, &n,
                             stats, s);
    if (rc != DP_OK)
        return rc;
    if (n > cap)
        return fail(c, DP_E_HIP, "dp_fuse_maps: more points than depth pixels");
    DP_HIP(c, c->fuse.res.resize((size_t)std::max<int64_t>(n, 1)));
    if (n > 0) {
        DP_HIP(c, hipMemcpyAsync(c->fuse.res.data(), c->fuse.pts.p, sizeof(dp_fused_point) * (size_t)n,
                                 hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *out = n > 0 ? c->fuse.res.data() : nullptr;
    *n_out = n;
    return DP_OK;
}
