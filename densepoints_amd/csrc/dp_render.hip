// dp_render.hip -- gfx950 kernels of the per-view depth / index / normal /
// score maps (spec in include/densepoints.h, dp_render_maps): every patch is an
// oriented disc in its own plane, each pixel keeps the nearest one.
//
//   render_pairs_kernel    one lane per patch walks the requested views it is
//                          visible in; the (patch, view) uniform fp64 -- frame,
//                          homography, adjugate, candidate box -- runs once per
//                          pair and is appended to a device list (one atomicAdd
//                          per wave and view step, ballot-ranked)
//   render_raster_kernel   one wave per pair, sized from the device-held count:
//                          lanes stride over the box 64 pixels at a time (three
//                          fp64 mul+add rows, one division) and atomicMin the
//                          key (f32 depth bits << 32 | index) into the z-buffer
//   render_resolve_kernel  one thread per pixel: key -> depth, index, and the
//                          winner's normal and score, as coalesced planes
//
// The result is a per-pixel minimum of values that depend on one (patch, view,
// pixel) alone: independent of the pair order and of the launch geometry.
#include "dp_ctx.h"
#include "dp_mapdev.h"

#include <cmath>
#include <cstdlib>

namespace dpk {
namespace {

__device__ __forceinline__ bool finite3(const float *f) { return isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]); }

// steps 2-4 of the pair spec and the homography; false = not a pair
__device__ bool make_pair(const dpg::ViewDev &v, const double *X, const double *n, double R, double max_radius,
                          bool facing_test, RenderPair &pr)
{
    if (facing_test) {
        const double d[3] = {X[0] - v.C[0], X[1] - v.C[1], X[2] - v.C[2]};
        if (!(dpg::dot3(n, d) > 0.0))
            return false;
    }
    const double d0 = row_of(v.P, 2, X);
    if (!(d0 > 0.0))
        return false;
    const double t = dpg::dot3(v.xr, n);
    const double e1[3] = {v.xr[0] - t * n[0], v.xr[1] - t * n[1], v.xr[2] - t * n[2]};
    const double s = dpg::dot3(e1, e1);
    if (!(s >= 1e-12))
        return false;
    double e2[3];
    dpg::cross3(n, e1, e2);
    // candidate box
    double cu, cv, qu, qv;
    dpg::project(v.P, X[0], X[1], X[2], cu, cv);
    if (!(fabs(cu) < 2.0e9) || !(fabs(cv) < 2.0e9))
        return false;
    dpg::project(v.P, X[0] + v.xr[0], X[1] + v.xr[1], X[2] + v.xr[2], qu, qv);
    const double du = qu - cu, dv = qv - cv;
    const double dxv = sqrt(du * du + dv * dv);
    const double Bq = (2.0 * R) * dxv + 2.0;
    const double B = Bq < max_radius ? Bq : max_radius;
    const int64_t x0 = (int64_t)floor(cu - B), x1 = (int64_t)ceil(cu + B);
    const int64_t y0 = (int64_t)floor(cv - B), y1 = (int64_t)ceil(cv + B);
    pr.x0 = (int32_t)(x0 > 0 ? x0 : 0);
    pr.x1 = (int32_t)(x1 < v.W - 1 ? x1 : v.W - 1);
    pr.y0 = (int32_t)(y0 > 0 ? y0 : 0);
    pr.y1 = (int32_t)(y1 < v.H - 1 ? y1 : v.H - 1);
    if (pr.x0 > pr.x1 || pr.y0 > pr.y1)
        return false;
    double h[9];
    for (int r = 0; r < 3; ++r) {
        const double *Pr = v.P + 4 * r;
        h[3 * r] = (Pr[0] * e1[0] + Pr[1] * e1[1]) + Pr[2] * e1[2];
        h[3 * r + 1] = (Pr[0] * e2[0] + Pr[1] * e2[1]) + Pr[2] * e2[2];
        h[3 * r + 2] = row_of(v.P, r, X);
    }
    pr.D = dpg::adjugate3(h, pr.A);
    pr.s = s;
    pr.RR = R * R;
    return true;
}

__global__ __launch_bounds__(256) void render_pairs_kernel(RenderArgs a, int64_t i0, int64_t i1, int chunk)
{
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long *npairs = a.count + kRenderCounters + chunk;
    uint64_t bits[2] = {0, 0};
    double X[3] = {0, 0, 0}, n[3] = {0, 0, 0}, R = 0.0;
    bool takes_part = false;
    if (i < i1 && (!a.keep || a.keep[i])) {
        const dp_patch &p = a.patches[i];
        const double rho = a.rho[i];
        if (finite3(p.pos) && finite3(p.normal) && p.ref < (uint32_t)a.V && rho > 0.0) {
            takes_part = true;
            for (int k = 0; k < 3; ++k) {
                X[k] = (double)p.pos[k];
                n[k] = (double)p.normal[k];
            }
            R = a.splat_scale * rho;
            for (int w = 0; w < 2; ++w)
                bits[w] = a.req[w] & (a.all_facing ? ~0ull : p.vis[w]);
        }
    }
    uint32_t my_pairs = 0;
    unsigned long long my_tests = 0;
    for (int w = 0; w < 2; ++w) {
        // the wave walks until every lane's mask word is empty (the ballots
        // below need all lanes in the loop)
        while (__any(bits[w] != 0)) {
            RenderPair pr;
            bool f = false;
            if (bits[w]) {
                const int b = __builtin_ctzll(bits[w]);
                bits[w] &= bits[w] - 1;
                const int view = w * 64 + b;
                f = make_pair(a.views[view], X, n, R, a.max_radius, a.all_facing != 0, pr);
                if (f) {
                    pr.slot = a.slot_of[view];
                    pr.index = (int32_t)i;
                }
            }
            const uint64_t m = __ballot(f);
            if (!m)
                continue;
            const int leader = __builtin_ctzll(m);
            unsigned long long at = 0;
            if ((int)(threadIdx.x & 63) == leader)
                at = atomicAdd(npairs, (unsigned long long)__popcll(m));
            at = __shfl(at, leader);
            if (f) {
                const int64_t k = (int64_t)at + lanes_below(m);
                if (k < a.pair_cap) // cannot fail: (i1 - i0) * n_slots <= pair_cap
                    a.pairs[k] = pr;
                ++my_pairs;
                my_tests += (unsigned long long)(pr.x1 - pr.x0 + 1) * (unsigned long long)(pr.y1 - pr.y0 + 1);
            }
        }
    }
    // statistics: one atomic per wave and counter
    uint32_t np = takes_part ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        np += __shfl_xor(np, o);
        my_pairs += __shfl_xor(my_pairs, o);
        my_tests += __shfl_xor(my_tests, o);
    }
    if ((threadIdx.x & 63) == 0 && np) {
        atomicAdd(&a.count[0], (unsigned long long)np);
        atomicAdd(&a.count[1], (unsigned long long)my_pairs);
        atomicAdd(&a.count[2], my_tests);
    }
}

__global__ __launch_bounds__(256) void render_raster_kernel(RenderArgs a, int chunk)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    int64_t np = (int64_t)a.count[kRenderCounters + chunk];
    np = np < a.pair_cap ? np : a.pair_cap;
    for (int64_t k = wave; k < np; k += nwaves) {
        const RenderPair &pr = a.pairs[k];
        const RenderSlot &sl = a.slots[pr.slot];
        unsigned long long *z = a.zbuf + sl.zoff;
        const int32_t W = sl.W;
        const int32_t x0 = pr.x0, x1 = pr.x1, y1 = pr.y1;
        const int32_t bw = x1 - x0 + 1;
        const double A0 = pr.A[0], A1 = pr.A[1], A2 = pr.A[2], A3 = pr.A[3], A4 = pr.A[4], A5 = pr.A[5],
                     A6 = pr.A[6], A7 = pr.A[7], A8 = pr.A[8];
        const double D = pr.D, s = pr.s, RR = pr.RR;
        const unsigned long long idx = (uint32_t)pr.index;
        int32_t y = pr.y0 + lane / bw, x = x0 + lane % bw;
        while (y <= y1) {
            const double fx = (double)x, fy = (double)y;
            const double pa = (A0 * fx + A1 * fy) + A2;
            const double pb = (A3 * fx + A4 * fy) + A5;
            const double pw = (A6 * fx + A7 * fy) + A8;
            if (((pw > 0.0 && D > 0.0) || (pw < 0.0 && D < 0.0)) && (pa * pa + pb * pb) * s <= RR * (pw * pw)) {
                const float zf = (float)(D / pw);
                if (zf > 0.0f) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | idx;
                    unsigned long long *cell = z + (int64_t)y * W + x;
                    // a stale read only costs an atomic: keys never grow
                    if (key < *(volatile unsigned long long *)cell)
                        atomicMin(cell, key);
                }
            }
            x += 64;
            while (x > x1) {
                x -= bw;
                ++y;
            }
        }
    }
}

__global__ __launch_bounds__(256) void render_resolve_kernel(RenderArgs a)
{
    const RenderSlot &sl = a.slots[blockIdx.y];
    const int64_t npx = (int64_t)sl.W * sl.H;
    uint32_t covered = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = a.zbuf[sl.zoff + i];
        const bool hit = key != ~0ull;
        const int32_t q = hit ? (int32_t)(uint32_t)key : -1;
        if (sl.depth)
            sl.depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (sl.index)
            sl.index[i] = q;
        if (sl.normal) {
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if (hit) {
                const dp_patch &p = a.patches[q];
                n0 = p.normal[0];
                n1 = p.normal[1];
                n2 = p.normal[2];
            }
            sl.normal[3 * i] = n0;
            sl.normal[3 * i + 1] = n1;
            sl.normal[3 * i + 2] = n2;
        }
        if (sl.score)
            sl.score[i] = hit ? a.patches[q].score : 0.0f;
        covered += hit ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1)
        covered += __shfl_xor(covered, o);
    if ((threadIdx.x & 63) == 0 && covered)
        atomicAdd(&a.count[3], (unsigned long long)covered);
}

} // namespace

hipError_t launch_render_pairs(const RenderArgs &a, int64_t i0, int64_t i1, int chunk, hipStream_t s)
{
    if (i1 <= i0)
        return hipSuccess;
    hipLaunchKernelGGL(render_pairs_kernel, dim3((unsigned)((i1 - i0 + 255) / 256)), dim3(256), 0, s, a, i0, i1,
                       chunk);
    return hipGetLastError();
}

hipError_t launch_render_raster(const RenderArgs &a, int chunk, hipStream_t s)
{
    // the pair count lives on the device: a fixed grid of waves strides over it
    const int64_t bound = a.pair_cap < 8192 ? a.pair_cap : 8192;
    hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, s, a, chunk);
    return hipGetLastError();
}

hipError_t launch_render_resolve(const RenderArgs &a, int max_pixels, hipStream_t s)
{
    if (a.n_slots <= 0 || max_pixels <= 0)
        return hipSuccess;
    int64_t bx = ((int64_t)max_pixels + 255) / 256;
    bx = bx < 1024 ? bx : 1024;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)bx, (unsigned)a.n_slots), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_render_options(dp_render_options *ro)
{
    if (!ro)
        return;
    ro->splat_scale = 1.0f;
    ro->max_radius_px = 32;
    ro->flags = 0;
}

// argument checks shared by both forms (they need no device)
static int render_check(dp_ctx *c, int64_t n, const void *patches, const int32_t *views, int n_views,
                        const dp_render_options &o)
{
    if (!c)
        return DP_E_ARG;
    if (n < 0 || n > 0x7FFFFFFFll || (n > 0 && !patches))
        return fail(c, DP_E_ARG, "dp_render_maps: n must be in 0..2^31-1 with patches given");
    if (!(o.splat_scale > 0.0f) || !std::isfinite(o.splat_scale))
        return fail(c, DP_E_ARG, "dp_render_maps: splat_scale must be > 0");
    if (o.max_radius_px < 1 || o.max_radius_px > 255)
        return fail(c, DP_E_ARG, "dp_render_maps: max_radius_px must be in 1..255");
    return check_view_list(c, "dp_render_maps", views, n_views, DP_MAX_VIEWS);
}

extern "C" int dp_render_maps_device(dp_ctx *c, const dp_patch *d_patches, int64_t n, const uint8_t *d_keep,
                                     const int32_t *views, int n_views, const dp_render_options *ro,
                                     float *const *d_depth, int32_t *const *d_index, float *const *d_normal,
                                     float *const *d_score, dp_render_stats *stats, void *stream)
{
    dp_render_options o;
    dp_default_render_options(&o);
    if (ro)
        o = *ro;
    int rc = render_check(c, n, d_patches, views, n_views, o);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;

    // slot tables and the z-buffer layout
    std::vector<dpk::RenderSlot> slots((size_t)n_views);
    std::vector<int32_t> slot_of(DP_MAX_VIEWS, -1);
    dpk::RenderArgs a{};
    int64_t zwords = 0;
    int max_pixels = 0;
    for (int k = 0; k < n_views; ++k) {
        const dpg::ViewDev &v = c->hv[views[k]];
        dpk::RenderSlot &sl = slots[k];
        sl.view = views[k];
        sl.W = v.W;
        sl.H = v.H;
        sl.pad = 0;
        sl.zoff = zwords;
        sl.depth = d_depth ? d_depth[k] : nullptr;
        sl.index = d_index ? d_index[k] : nullptr;
        sl.normal = d_normal ? d_normal[k] : nullptr;
        sl.score = d_score ? d_score[k] : nullptr;
        const int64_t px = (int64_t)v.W * v.H;
        if (px > 0x7FFFFFFFll)
            return fail(c, DP_E_ARG, "dp_render_maps: view too large");
        zwords += px;
        max_pixels = std::max(max_pixels, (int)px);
        slot_of[views[k]] = k;
        a.req[views[k] >> 6] |= 1ull << (views[k] & 63);
    }
    // pair list: patches go through in chunks of at most pair_cap / n_views, so
    // the list cannot overflow whatever the visible sets are
    int64_t pair_cap = std::min<int64_t>(std::max<int64_t>(n * n_views, 1), (int64_t)1 << 21);
    if (const char *e = getenv("DP_RENDER_PAIR_CAP")) // tests: several chunks on a small input
        pair_cap = std::max<int64_t>(std::atoll(e), n_views);
    const int64_t per_chunk = std::max<int64_t>(pair_cap / n_views, 1);
    const int64_t chunks = n > 0 ? (n + per_chunk - 1) / per_chunk : 0;
    const size_t ncount = (size_t)dpk::kRenderCounters + (size_t)chunks;

    DP_HIP(c, c->pix64.reserve((size_t)zwords));
    DP_HIP(c, c->render.pairs.reserve((size_t)pair_cap));
    DP_HIP(c, c->render.count.reserve(ncount));
    DP_HIP(c, c->render.slots.reserve((size_t)n_views));
    DP_HIP(c, c->render.slot_of.reserve((size_t)DP_MAX_VIEWS));
    if (n > 0)
        DP_HIP(c, c->f_rho.reserve((size_t)n));

    a.views = c->d_views;
    a.V = c->V;
    a.n_slots = n_views;
    a.patches = d_patches;
    a.keep = d_keep;
    a.rho = c->f_rho.p;
    a.n = n;
    a.slots = c->render.slots.p;
    a.slot_of = c->render.slot_of.p;
    a.splat_scale = (double)o.splat_scale;
    a.max_radius = (double)o.max_radius_px;
    a.all_facing = (o.flags & DP_RENDER_ALL_FACING) ? 1 : 0;
    a.pairs = c->render.pairs.p;
    a.pair_cap = pair_cap;
    a.zbuf = c->pix64.p;
    a.count = c->render.count.p;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the tables are read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(c->render.slots.p, slots.data(), sizeof(dpk::RenderSlot) * slots.size(),
                             hipMemcpyHostToDevice, s));
    DP_HIP(c, hipMemcpyAsync(c->render.slot_of.p, slot_of.data(), sizeof(int32_t) * slot_of.size(),
                             hipMemcpyHostToDevice, s));
    DP_HIP(c, c->render.time.begin(s));
    DP_HIP(c, hipMemsetAsync(c->render.count.p, 0, sizeof(unsigned long long) * ncount, s));
    DP_HIP(c, hipMemsetAsync(c->pix64.p, 0xFF, sizeof(unsigned long long) * (size_t)zwords, s));
    if (n > 0) {
        dpk::FilterArgs fa{};
        fa.views = c->d_views;
        fa.V = c->V;
        fa.patches = d_patches;
        fa.n = n;
        fa.rho = c->f_rho.p;
        fa.grid_scale = (double)c->opt.grid_scale;
        DP_HIP(c, dpk::launch_filter_rho(fa, s));
    }
    for (int64_t k = 0; k < chunks; ++k) {
        const int64_t i0 = k * per_chunk, i1 = std::min<int64_t>(n, i0 + per_chunk);
        DP_HIP(c, dpk::launch_render_pairs(a, i0, i1, (int)k, s));
        DP_HIP(c, dpk::launch_render_raster(a, (int)k, s));
    }
    DP_HIP(c, dpk::launch_render_resolve(a, max_pixels, s));
    DP_HIP(c, c->render.time.end(s));
    if (stats) {
        unsigned long long h[dpk::kRenderCounters];
        DP_HIP(c, hipMemcpyAsync(h, c->render.count.p, sizeof(h), hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipStreamSynchronize(s));
        stats->patches = (int64_t)h[0];
        stats->pairs = (int64_t)h[1];
        stats->pixel_tests = (int64_t)h[2];
        stats->covered_pixels = (int64_t)h[3];
        DP_HIP(c, c->render.time.ms(stats->render_ms));
    }
    return DP_OK;
}

extern "C" int dp_render_maps(dp_ctx *c, const dp_patch *patches, int64_t n, const uint8_t *keep,
                              const int32_t *views, int n_views, const dp_render_options *ro, float *const *depth,
                              int32_t *const *index, float *const *normal, float *const *score,
                              dp_render_stats *stats)
{
    dp_render_options o;
    dp_default_render_options(&o);
    if (ro)
        o = *ro;
    int rc = render_check(c, n, patches, views, n_views, o);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // device planes of the outputs asked for, 256-B aligned, in one buffer
    struct Plane {
        void *host;
        size_t off, bytes;
    };
    std::vector<Plane> planes;
    PlanePacker pack;
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        void *const host[4] = {depth ? depth[k] : nullptr, index ? index[k] : nullptr, normal ? normal[k] : nullptr,
                               score ? score[k] : nullptr};
        for (int j = 0; j < 4; ++j) {
            const size_t bytes = (j == 2 ? 12 : 4) * px;
            planes.push_back({host[j], host[j] ? pack.add(bytes) : 0, bytes});
        }
    }
    DP_HIP(c, c->render.out.reserve(pack.total ? pack.total : 1));
    // the device form's plane tables: entry 4 k + j of planes, null where not wanted
    std::vector<float *> dd(n_views), dn(n_views), ds(n_views);
    std::vector<int32_t *> di(n_views);
    for (int k = 0; k < n_views; ++k) {
        auto at = [&](int j) { return planes[4 * k + j].host ? c->render.out.p + planes[4 * k + j].off : nullptr; };
        dd[k] = (float *)at(0);
        di[k] = (int32_t *)at(1);
        dn[k] = (float *)at(2);
        ds[k] = (float *)at(3);
    }
    if (n > 0) {
        DP_HIP(c, c->f_pat.reserve((size_t)n));
        DP_HIP(c, hipMemcpyAsync(c->f_pat.p, patches, sizeof(dp_patch) * (size_t)n, hipMemcpyHostToDevice, s));
        if (keep) {
            DP_HIP(c, c->f_keep.reserve((size_t)n));
            DP_HIP(c, hipMemcpyAsync(c->f_keep.p, keep, (size_t)n, hipMemcpyHostToDevice, s));
        }
    }
    rc = dp_render_maps_device(c, n > 0 ? c->f_pat.p : nullptr, n, keep && n > 0 ? c->f_keep.p : nullptr, views,
                               n_views, &o, dd.data(), di.data(), dn.data(), ds.data(), stats, s);
    if (rc != DP_OK)
        return rc;
    for (const Plane &p : planes)
        if (p.host)
            DP_HIP(c, hipMemcpyAsync(p.host, c->render.out.p + p.off, p.bytes, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}
