// dp_meshrender.hip -- gfx950 kernels of the per-view depth / triangle-index /
// normal maps of a triangle mesh (spec in include/densepoints.h,
// dp_mesh_render): dp_render.hip's three stages with a triangle in the place of
// the disc.
//
//   meshrender_pairs_kernel    one lane per triangle walks the requested views;
//                              the (triangle, view) uniform fp64 -- three
//                              projections, three edge rows, D, the facing, the
//                              box -- runs once per pair and is appended to a
//                              device list.  A box is cut into bands of rows of
//                              at most kMeshRenderBudget pixels; the list slot
//                              and the pair's first band number come from ONE
//                              atomicAdd per wave and view step on a packed
//                              counter (bands << 22 | pairs), so the first band
//                              numbers ascend with the slots
//   meshrender_raster_kernel   a fixed grid of waves shares the device-held band
//                              total evenly: a wave finds the pair of its first
//                              band by bisection, then walks its run of bands
//                              (consecutive bands of a pair are one walk), lanes
//                              striding 64 pixels at a time: three fp64 mul+add
//                              rows, the sign test, one division, atomicMin of
//                              the key (f32 depth bits << 32 | triangle)
//   meshrender_resolve_kernel  one thread per pixel: key -> depth, index and the
//                              winner's face normal, as coalesced planes
//
// The result is a per-pixel minimum of values that depend on one (triangle,
// view, pixel) alone: independent of the pair order, the bands and the launch
// geometry.  The edge rows are written as the spec writes them; see its note on
// shared edges before touching an operand order.
#include "dp_ctx.h"
#include "dp_mapdev.h"
#include "dp_meshdev.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace dpk {
namespace {

constexpr int kMeshRenderCounters = 7; // triangles, invalid, pairs, clipped, culled, pixel tests, covered pixels
constexpr int kPairBits = 22;          // of a chunk's packed counter: the pairs (<= kMaxItemCap); above them the bands (< 2^42)
constexpr int64_t kMaxItemCap = (int64_t)1 << 20;
constexpr int64_t kMeshRenderBudget = 2048; // pixels of a band: 32 steps of a wave
constexpr unsigned long long kPairMask = (1ull << kPairBits) - 1;

struct MeshRenderArgs {
    const dpg::ViewDev *views;
    const MeshRenderSlot *slots;
    int32_t n_slots, cull_back;
    const dp_mesh_vertex *verts;
    const int32_t *tris;
    int64_t nv, nt;
    MeshRenderPair *pairs;
    int64_t pair_cap;
    unsigned long long *zbuf;  // per pixel: f32 depth bits << 32 | triangle, ~0 = empty
    unsigned long long *count; // kMeshRenderCounters, then one packed counter per chunk
};

// rows of a band of a box bw pixels wide, and the bands of its bh rows
__device__ __forceinline__ int64_t band_rows(int64_t bw) { return bw < kMeshRenderBudget ? kMeshRenderBudget / bw : 1; }

// cross product of the homogeneous points a, b (the spec's r_k)
__device__ __forceinline__ void edge_row(const double *a, const double *b, double *r)
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

enum PairResult { kNoPair, kClipped, kCulled, kPair };

// steps 1-3 of the pair spec
__device__ PairResult make_pair(const dpg::ViewDev &v, const MeshRenderSlot &sl, const double X[3][3], bool cull_back,
                                MeshRenderPair &pr)
{
    double h[3][3];
    int front = 0;
    for (int k = 0; k < 3; ++k) {
        for (int r = 0; r < 3; ++r)
            h[k][r] = row_of(v.P, r, X[k]);
        front += h[k][2] > 0.0 ? 1 : 0;
    }
    if (front < 3)
        return front > 0 ? kClipped : kNoPair;
    for (int k = 0; k < 3; ++k)
        edge_row(h[(k + 1) % 3], h[(k + 2) % 3], pr.r + 3 * k);
    const double D = (h[0][0] * pr.r[0] + h[0][1] * pr.r[1]) + h[0][2] * pr.r[2];
    if (!isfinite(D) || D == 0.0)
        return kNoPair;
    if (cull_back && !((D > 0.0 && sl.m < 0.0) || (D < 0.0 && sl.m > 0.0)))
        return kCulled;
    double u[3], w[3];
    for (int k = 0; k < 3; ++k) {
        dpg::div2(h[k][0], h[k][1], h[k][2], u[k], w[k]);
        if (!(fabs(u[k]) < 2.0e9) || !(fabs(w[k]) < 2.0e9))
            return kNoPair;
    }
    const int64_t x0 = (int64_t)floor(fmin(fmin(u[0], u[1]), u[2])), x1 = (int64_t)ceil(fmax(fmax(u[0], u[1]), u[2]));
    const int64_t y0 = (int64_t)floor(fmin(fmin(w[0], w[1]), w[2])), y1 = (int64_t)ceil(fmax(fmax(w[0], w[1]), w[2]));
    pr.x0 = (int32_t)(x0 > 0 ? x0 : 0);
    pr.x1 = (int32_t)(x1 < sl.W - 1 ? x1 : sl.W - 1);
    pr.y0 = (int32_t)(y0 > 0 ? y0 : 0);
    pr.y1 = (int32_t)(y1 < sl.H - 1 ? y1 : sl.H - 1);
    if (pr.x0 > pr.x1 || pr.y0 > pr.y1)
        return kNoPair;
    pr.D = D;
    return kPair;
}

__global__ __launch_bounds__(kMeshLanes) void meshrender_pairs_kernel(MeshRenderArgs a, int64_t t0, int64_t t1, int chunk)
{
    const int64_t t = t0 + mesh_item();
    const int lane = threadIdx.x & 63;
    unsigned long long *packed = a.count + kMeshRenderCounters + chunk;
    int32_t vi[3];
    double X[3][3];
    bool takes_part = false, invalid = false;
    if (t < t1) {
        if (load_valid_triangle(a.tris, a.nt, a.nv, t, vi)) {
            takes_part = true;
            for (int k = 0; k < 3; ++k) {
                const float *p = a.verts[vi[k]].pos;
                takes_part = takes_part && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
                for (int j = 0; j < 3; ++j)
                    X[k][j] = (double)p[j];
            }
        } else {
            invalid = true;
        }
    }
    uint32_t my_pairs = 0, my_clipped = 0, my_culled = 0;
    unsigned long long my_tests = 0;
    // every lane of the wave walks every slot: the ballots and the scan below
    // need all of them
    for (int k = 0; k < a.n_slots; ++k) {
        const MeshRenderSlot &sl = a.slots[k];
        MeshRenderPair pr;
        PairResult res = kNoPair;
        if (takes_part)
            res = make_pair(a.views[sl.view], sl, X, a.cull_back != 0, pr);
        my_clipped += res == kClipped ? 1u : 0u;
        my_culled += res == kCulled ? 1u : 0u;
        const bool f = res == kPair;
        uint32_t nb = 0;
        if (f) {
            const int64_t bw = (int64_t)pr.x1 - pr.x0 + 1, bh = (int64_t)pr.y1 - pr.y0 + 1, rows = band_rows(bw);
            nb = (uint32_t)((bh + rows - 1) / rows); // <= 2^21 + 1: a view has < 2^31 pixels
            ++my_pairs;
            my_tests += (unsigned long long)(bw * bh);
        }
        const uint64_t m = __ballot(f);
        if (!m)
            continue;
        uint32_t incl = nb; // the wave's inclusive scan of the band counts (< 2^28)
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o)
                incl += y;
        }
        const unsigned long long bands = __shfl(incl, 63);
        const int leader = __builtin_ctzll(m);
        unsigned long long at = 0;
        if (lane == leader)
            at = atomicAdd(packed, bands << kPairBits | (unsigned long long)__popcll(m));
        at = __shfl(at, leader);
        if (f) {
            const int64_t slot = (int64_t)(at & kPairMask) + lanes_below(m);
            pr.first = (int64_t)(at >> kPairBits) + (incl - nb);
            pr.slot = k;
            pr.index = (int32_t)t;
            if (slot < a.pair_cap) // cannot fail: (t1 - t0) * n_slots <= pair_cap
                a.pairs[slot] = pr;
        }
    }
    // statistics: one atomic per wave and counter
    const unsigned long long v[6] = {takes_part ? 1ull : 0ull, invalid ? 1ull : 0ull, my_pairs, my_clipped, my_culled,
                                     my_tests};
    for (int j = 0; j < 6; ++j)
        wave_count<1, kMeshRenderCounters>(a.count, j, v[j], 0);
}

__global__ __launch_bounds__(256) void meshrender_raster_kernel(MeshRenderArgs a, int chunk)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const unsigned long long packed = a.count[kMeshRenderCounters + chunk];
    int64_t np = (int64_t)(packed & kPairMask);
    np = np < a.pair_cap ? np : a.pair_cap;
    const int64_t bands = (int64_t)(packed >> kPairBits);
    // this wave's run of bands
    const int64_t per = (bands + nwaves - 1) / nwaves;
    int64_t g = wave * per;
    const int64_t g1 = g + per < bands ? g + per : bands;
    if (g >= g1 || np <= 0)
        return;
    // the last pair whose first band is <= g (pair 0 starts at band 0)
    int64_t lo = 0, hi = np - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.pairs[mid].first <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    for (int64_t k = lo; k < np && g < g1; ++k) {
        const MeshRenderPair &pr = a.pairs[k];
        const MeshRenderSlot &sl = a.slots[pr.slot];
        unsigned long long *z = a.zbuf + sl.zoff;
        const int64_t W = sl.W, x0 = pr.x0, x1 = pr.x1;
        const int64_t bw = x1 - x0 + 1, bh = (int64_t)pr.y1 - pr.y0 + 1, rows = band_rows(bw);
        const int64_t nb = (bh + rows - 1) / rows;
        // bands [b, be) of the pair are rows [ya, yb]
        const int64_t b = g - pr.first;
        const int64_t be = nb - b < g1 - g ? nb : b + (g1 - g);
        g += be - b;
        const int64_t ya = pr.y0 + b * rows;
        const int64_t yb = be == nb ? (int64_t)pr.y1 : pr.y0 + be * rows - 1;
        const double r0 = pr.r[0], r1 = pr.r[1], r2 = pr.r[2], r3 = pr.r[3], r4 = pr.r[4], r5 = pr.r[5], r6 = pr.r[6],
                     r7 = pr.r[7], r8 = pr.r[8];
        const double D = pr.D;
        const unsigned long long idx = (uint32_t)pr.index;
        int64_t y = ya + lane / bw, x = x0 + lane % bw;
        while (y <= yb) {
            const double fx = (double)x, fy = (double)y;
            const double l0 = (r0 * fx + r1 * fy) + r2;
            const double l1 = (r3 * fx + r4 * fy) + r5;
            const double l2 = (r6 * fx + r7 * fy) + r8;
            if ((D > 0.0 && l0 >= 0.0 && l1 >= 0.0 && l2 >= 0.0) || (D < 0.0 && l0 <= 0.0 && l1 <= 0.0 && l2 <= 0.0)) {
                const double w = (l0 + l1) + l2;
                if (w != 0.0) {
                    const float zf = (float)(D / w);
                    if (is_depth(zf)) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | idx;
                        unsigned long long *cell = z + y * W + x;
                        // a stale read only costs an atomic: keys never grow
                        if (key < *(volatile unsigned long long *)cell)
                            atomicMin(cell, key);
                    }
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

__global__ __launch_bounds__(256) void meshrender_resolve_kernel(MeshRenderArgs a)
{
    const MeshRenderSlot &sl = a.slots[blockIdx.y];
    const int64_t npx = (int64_t)sl.W * sl.H;
    unsigned long long covered = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = a.zbuf[sl.zoff + i];
        const bool hit = key != ~0ull;
        const int32_t q = hit ? (int32_t)(uint32_t)key : -1;
        if (sl.depth)
            sl.depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (sl.index)
            sl.index[i] = q;
        if (sl.normal) {
            float n[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {
                // a winner is a triangle that took part: its indices are vertices
                const float *p0 = a.verts[a.tris[3 * (int64_t)q]].pos, *p1 = a.verts[a.tris[3 * (int64_t)q + 1]].pos,
                            *p2 = a.verts[a.tris[3 * (int64_t)q + 2]].pos;
                double e[3], f[3], N[3];
                for (int j = 0; j < 3; ++j) {
                    e[j] = (double)p1[j] - (double)p0[j];
                    f[j] = (double)p2[j] - (double)p0[j];
                }
                dpg::cross3(e, f, N);
                const double s = sqrt(dpg::dot3(N, N));
                if (isfinite(s) && s > 0.0)
                    for (int j = 0; j < 3; ++j)
                        n[j] = (float)(N[j] / s);
            }
            sl.normal[3 * i] = n[0];
            sl.normal[3 * i + 1] = n[1];
            sl.normal[3 * i + 2] = n[2];
        }
        covered += hit ? 1ull : 0ull;
    }
    wave_count<1, kMeshRenderCounters>(a.count, 6, covered, 0);
}

hipError_t launch_pairs(const MeshRenderArgs &a, int64_t t0, int64_t t1, int chunk, hipStream_t s)
{
    if (t1 <= t0)
        return hipSuccess;
    hipLaunchKernelGGL(meshrender_pairs_kernel, dim3((unsigned)mesh_blocks(t1 - t0)), dim3(kMeshLanes), 0, s, a, t0, t1,
                       chunk);
    return hipGetLastError();
}

hipError_t launch_raster(const MeshRenderArgs &a, int chunk, hipStream_t s)
{
    // the band total lives on the device: a fixed grid of waves shares it
    hipLaunchKernelGGL(meshrender_raster_kernel, dim3(2048), dim3(256), 0, s, a, chunk);
    return hipGetLastError();
}

hipError_t launch_resolve(const MeshRenderArgs &a, int64_t max_pixels, hipStream_t s)
{
    if (a.n_slots <= 0 || max_pixels <= 0)
        return hipSuccess;
    int64_t bx = (max_pixels + 255) / 256;
    bx = bx < 1024 ? bx : 1024;
    hipLaunchKernelGGL(meshrender_resolve_kernel, dim3((unsigned)bx, (unsigned)a.n_slots), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mesh_render_options(dp_mesh_render_options *mro)
{
    if (mro)
        mro->flags = 0;
}

// argument checks shared by both forms (they need no device); m[k] = the
// determinant of the left 3x3 of view k's projection
static int meshrender_check(dp_ctx *c, const std::string &w, const void *vertices, int64_t nv, const void *tris,
                            int64_t nt, const int32_t *views, int n_views, const dp_mesh_render_options &o,
                            std::vector<double> &m)
{
    int rc = mesh_check_counts(c, w, tris, nt, nv);
    if (rc != DP_OK)
        return rc;
    if (nv > 0 && !vertices)
        return fail(c, DP_E_ARG, w + ": vertices must be given");
    if (o.flags & ~DP_MESH_RENDER_CULL_BACK)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    if ((rc = check_view_list(c, w.c_str(), views, n_views, DP_MAX_VIEWS)) != DP_OK)
        return rc;
    m.resize((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const double *P = c->hv[views[k]].P;
        m[k] = (P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8])) +
               P[2] * (P[4] * P[9] - P[5] * P[8]);
        if (!std::isfinite(m[k]) || m[k] == 0.0)
            return fail(c, DP_E_ARG, w + ": a view's projection has a singular or non-finite left 3x3");
        if ((int64_t)c->hv[views[k]].W * c->hv[views[k]].H > 0x7FFFFFFFll)
            return fail(c, DP_E_ARG, w + ": view too large");
    }
    return DP_OK;
}

// queues the render of a device mesh into device planes on s
static int meshrender_queue(dp_ctx *c, const dp_mesh_vertex *d_vertices, int64_t nv, const int32_t *d_triangles,
                            int64_t nt, const int32_t *views, int n_views, const dp_mesh_render_options &o,
                            const std::vector<double> &m, float *const *d_depth, int32_t *const *d_index,
                            float *const *d_normal, hipStream_t s)
{
    dpk::MeshRenderScratch &r = c->meshrender;
    std::vector<dpk::MeshRenderSlot> slots((size_t)n_views);
    int64_t zwords = 0, max_pixels = 0;
    for (int k = 0; k < n_views; ++k) {
        const dpg::ViewDev &v = c->hv[views[k]];
        dpk::MeshRenderSlot &sl = slots[k];
        sl.view = views[k];
        sl.W = v.W;
        sl.H = v.H;
        sl.pad = 0;
        sl.zoff = zwords;
        sl.m = m[k];
        sl.depth = d_depth ? d_depth[k] : nullptr;
        sl.index = d_index ? d_index[k] : nullptr;
        sl.normal = d_normal ? d_normal[k] : nullptr;
        const int64_t px = (int64_t)v.W * v.H;
        zwords += px;
        max_pixels = std::max(max_pixels, px);
    }
    // pair list: triangles go through in chunks of at most item_cap / n_views,
    // so the list cannot overflow whatever the views see
    int64_t item_cap = std::min<int64_t>(std::max<int64_t>(nt * n_views, 1), dpk::kMaxItemCap);
    if (const char *e = getenv("DP_MESH_RENDER_ITEM_CAP")) // tests: several chunks on a small mesh
        item_cap = std::min<int64_t>(std::max<int64_t>(std::atoll(e), n_views), dpk::kMaxItemCap);
    const int64_t per_chunk = std::max<int64_t>(item_cap / n_views, 1);
    const int64_t chunks = nt > 0 ? (nt + per_chunk - 1) / per_chunk : 0;
    const size_t ncount = (size_t)dpk::kMeshRenderCounters + (size_t)chunks;

    DP_HIP(c, c->pix64.reserve((size_t)std::max<int64_t>(zwords, 1)));
    DP_HIP(c, r.pairs.reserve((size_t)item_cap));
    DP_HIP(c, r.count.reserve(ncount));
    DP_HIP(c, r.slots.reserve((size_t)n_views));

    dpk::MeshRenderArgs a{};
    a.views = c->d_views;
    a.slots = r.slots.p;
    a.n_slots = n_views;
    a.cull_back = (o.flags & DP_MESH_RENDER_CULL_BACK) ? 1 : 0;
    a.verts = d_vertices;
    a.tris = d_triangles;
    a.nv = nv;
    a.nt = nt;
    a.pairs = r.pairs.p;
    a.pair_cap = item_cap;
    a.zbuf = c->pix64.p;
    a.count = r.count.p;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the table is read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(r.slots.p, slots.data(), sizeof(dpk::MeshRenderSlot) * slots.size(), hipMemcpyHostToDevice,
                             s));
    DP_HIP(c, r.time.begin(s));
    DP_HIP(c, hipMemsetAsync(r.count.p, 0, sizeof(unsigned long long) * ncount, s));
    if (zwords > 0)
        DP_HIP(c, hipMemsetAsync(c->pix64.p, 0xFF, sizeof(unsigned long long) * (size_t)zwords, s));
    for (int64_t k = 0; k < chunks; ++k) {
        const int64_t t0 = k * per_chunk, t1 = std::min<int64_t>(nt, t0 + per_chunk);
        DP_HIP(c, dpk::launch_pairs(a, t0, t1, (int)k, s));
        DP_HIP(c, dpk::launch_raster(a, (int)k, s));
    }
    DP_HIP(c, dpk::launch_resolve(a, max_pixels, s));
    DP_HIP(c, r.time.end(s));
    return DP_OK;
}

// the statistics read and its wait
static int meshrender_stats(dp_ctx *c, dp_mesh_render_stats *stats, hipStream_t s)
{
    unsigned long long h[dpk::kMeshRenderCounters];
    DP_HIP(c, hipMemcpyAsync(h, c->meshrender.count.p, sizeof(h), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    stats->triangles = (int64_t)h[0];
    stats->invalid_triangles = (int64_t)h[1];
    stats->pairs = (int64_t)h[2];
    stats->clipped_pairs = (int64_t)h[3];
    stats->culled_pairs = (int64_t)h[4];
    stats->pixel_tests = (int64_t)h[5];
    stats->covered_pixels = (int64_t)h[6];
    DP_HIP(c, c->meshrender.time.ms(stats->render_ms));
    return DP_OK;
}

extern "C" int dp_mesh_render_device(dp_ctx *c, const dp_mesh_vertex *d_vertices, int64_t n_vertices,
                                     const int32_t *d_triangles, int64_t n_triangles, const int32_t *views, int n_views,
                                     const dp_mesh_render_options *mro, float *const *d_depth, int32_t *const *d_index,
                                     float *const *d_normal, dp_mesh_render_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    dp_mesh_render_options o;
    dp_default_mesh_render_options(&o);
    if (mro)
        o = *mro;
    std::vector<double> m;
    int rc = meshrender_check(c, "dp_mesh_render_device", d_vertices, n_vertices, d_triangles, n_triangles, views, n_views,
                              o, m);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = meshrender_queue(c, d_vertices, n_vertices, d_triangles, n_triangles, views, n_views, o, m, d_depth,
                               d_index, d_normal, s)) != DP_OK)
        return rc;
    return stats ? meshrender_stats(c, stats, s) : DP_OK;
}

extern "C" int dp_mesh_render(dp_ctx *c, const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                              int64_t n_triangles, const int32_t *views, int n_views, const dp_mesh_render_options *mro,
                              float *const *depth, int32_t *const *index, float *const *normal,
                              dp_mesh_render_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    dp_mesh_render_options o;
    dp_default_mesh_render_options(&o);
    if (mro)
        o = *mro;
    std::vector<double> m;
    int rc = meshrender_check(c, "dp_mesh_render", vertices, n_vertices, triangles, n_triangles, views, n_views, o, m);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::MeshRenderScratch &r = c->meshrender;
    const int64_t nv = n_vertices, nt = n_triangles;
    // staged inputs: the vertices (16 B each), then the triangles
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    DP_HIP(c, r.in.reserve(std::max<size_t>(vbytes + 12 * (size_t)nt, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + vbytes, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    // device planes of the outputs asked for, 256-B aligned, in one buffer
    struct Plane {
        void *host;
        size_t off, bytes;
    };
    std::vector<Plane> planes;
    PlanePacker pack;
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        void *const host[3] = {depth ? depth[k] : nullptr, index ? index[k] : nullptr, normal ? normal[k] : nullptr};
        for (int j = 0; j < 3; ++j) {
            const size_t bytes = (j == 2 ? 12 : 4) * px;
            planes.push_back({host[j], host[j] ? pack.add(bytes) : 0, bytes});
        }
    }
    DP_HIP(c, r.out.reserve(pack.total ? pack.total : 1));
    // the device form's plane tables: entry 3 k + j of planes, null where not wanted
    std::vector<float *> dd(n_views), dn(n_views);
    std::vector<int32_t *> di(n_views);
    for (int k = 0; k < n_views; ++k) {
        auto at = [&](int j) { return planes[3 * k + j].host ? r.out.p + planes[3 * k + j].off : nullptr; };
        dd[k] = (float *)at(0);
        di[k] = (int32_t *)at(1);
        dn[k] = (float *)at(2);
    }
    if ((rc = meshrender_queue(c, nv > 0 ? (const dp_mesh_vertex *)r.in.p : nullptr, nv,
                               nt > 0 ? (const int32_t *)(r.in.p + vbytes) : nullptr, nt, views, n_views, o, m, dd.data(),
                               di.data(), dn.data(), s)) != DP_OK)
        return rc;
    for (const Plane &p : planes)
        if (p.host && p.bytes)
            DP_HIP(c, hipMemcpyAsync(p.host, r.out.p + p.off, p.bytes, hipMemcpyDeviceToHost, s));
    if (stats)
        return meshrender_stats(c, stats, s);
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}
