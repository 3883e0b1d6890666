// dp_meshsmooth.hip -- gfx950 kernels of the mesh adjacency, the Taubin
// smoothing and the vertex normals (spec in include/densepoints.h,
// dp_mesh_adjacency / dp_mesh_smooth / dp_mesh_normals) and their C ABI.
//
// The adjacency:
//   adj_keys_kernel     one lane per triangle: the guard, the classes (invalid,
//                       degenerate, proper) and six keys u << nb | v per proper
//                       triangle, all ones otherwise; nb = the bits of
//                       n_vertices, so a key needs 2 nb bits and the padding
//                       sorts behind every key
//   (one hipcub radix sort of the 6T keys over those 2 nb bits)
//   adj_heads_kernel    the first key of every run of equal keys is a directed
//                       entry (u, v); entries per block
//   (exclusive scan of the blocks' entries; its last word is E)
//   adj_emit_kernel     entry number = scanned offset + rank in the block; the
//                       run's length is count(u, v), found by doubling steps and
//                       a bisection (a run is 1 or 2 long on a manifold mesh, and
//                       a million copies of one triangle stay 20 probes); every
//                       sorted key's entry number is kept for the offsets
//   adj_offsets_kernel  one lane per vertex: offsets[v] = the entry number of the
//                       first key >= v << nb (a bisection of the sorted keys)
//   adj_rows_kernel     one lane per row: the flag byte, the isolated, boundary
//                       and nonmanifold counts, the longest row
// The neighbours and counts are written into the memory of the unsorted keys
// (dead after the sort, and exactly as large), and from there the smoothing
// reads them; a caller's buffers get the first min(cap, E) entries in the same
// kernel.
//
// The smoothing keeps positions as 3 floats per vertex in two context-owned
// arrays; a step is one lane per vertex walking its row (a contiguous int32
// run) in ascending order with an fp64 sum: a fan is just a longer loop.
//
// The normals sort 3T pairs (vertex; triangle) by the vertex alone: the radix
// sort is stable and the pairs are made in triangle order, so every vertex's
// triangles come out ascending; one lane per vertex walks them.
//
// Integer atomics only (the striped counters and one atomicMax); no float sum
// depends on the schedule.
#include "dp_meshdev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

constexpr int kSmoothStripes = 64;
// invalid, degenerate triangles; isolated vertices; directed boundary and
// nonmanifold entries; boundary vertices; zero normals
constexpr int kSmoothCounters = 7;
constexpr unsigned long long kPadKey = ~0ull;
constexpr uint32_t kPadVertex = ~0u;

struct AdjArgs {
    const int32_t *tris;
    int64_t nt, nv, nk; // nk = 6 nt keys
    int64_t nbt, nbv, nbk;
    int nb;             // the bits of n_vertices
    unsigned long long *keys, *sorted, *bcount, *boff, *count;
    int32_t *nbr, *cnt; // in the memory of `keys`, valid after the sort
    int32_t *hpos, *off, *maxval;
    uint8_t *vflags;
    // outputs, any may be null
    int32_t *o_off, *o_nbr, *o_cnt;
    int64_t cap;
    uint8_t *o_flags;
};

struct SmoothArgs {
    const dp_mesh_vertex *verts;
    dp_mesh_vertex *out;
    int64_t nv;
    const int32_t *off, *nbr;
    const uint8_t *vflags;
    const float *src;
    float *dst;
    double f;
    int pin; // boundary vertices are pinned
};

struct NormalArgs {
    const int32_t *tris;
    const dp_mesh_vertex *verts;
    int64_t nt, nv, n3; // n3 = 3 nt pairs
    uint32_t *ikeys, *ikeys_sorted;
    int32_t *itris, *itris_sorted;
    float *normals;
    unsigned long long *count;
};

__device__ __forceinline__ void smooth_count(unsigned long long *count, int counter, unsigned long long v)
{
    wave_count<kSmoothStripes, kSmoothCounters>(count, counter, v, blockIdx.x * (kMeshLanes / 64) + (threadIdx.x >> 6));
}

// the classes of triangle t: v holds its indices when it is valid
__device__ __forceinline__ void classify(const int32_t *tris, int64_t nt, int64_t nv, int64_t t, int32_t v[3],
                                         bool &valid, bool &proper)
{
    valid = load_valid_triangle(tris, nt, nv, t, v);
    proper = valid && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
}

__global__ __launch_bounds__(kMeshLanes) void adj_keys_kernel(AdjArgs a)
{
    const int64_t t = mesh_item();
    int32_t v[3] = {0, 0, 0};
    bool valid, proper;
    classify(a.tris, a.nt, a.nv, t, v, valid, proper);
    if (t < a.nt) {
        unsigned long long *k = a.keys + 6 * t; // 6 t + 5 < nk
        for (int e = 0; e < 3; ++e) {
            const unsigned long long u = (unsigned long long)(uint32_t)v[e], w1 = (unsigned long long)(uint32_t)v[(e + 1) % 3],
                                     w2 = (unsigned long long)(uint32_t)v[(e + 2) % 3];
            k[2 * e] = proper ? (u << a.nb | w1) : kPadKey;
            k[2 * e + 1] = proper ? (u << a.nb | w2) : kPadKey;
        }
    }
    smooth_count(a.count, 0, t < a.nt && !valid ? 1ull : 0ull);
    smooth_count(a.count, 1, valid && !proper ? 1ull : 0ull);
}

__device__ __forceinline__ bool is_head(const AdjArgs &a, int64_t i)
{
    if (i >= a.nk)
        return false;
    const unsigned long long k = a.sorted[i];
    return k != kPadKey && (i == 0 || a.sorted[i - 1] != k);
}

__global__ __launch_bounds__(kMeshLanes) void adj_heads_kernel(AdjArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const uint32_t total = block_sum<kMeshLanes>(is_head(a, mesh_item()) ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshLanes) void adj_emit_kernel(AdjArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const int64_t i = mesh_item();
    const bool head = is_head(a, i);
    const int64_t pos = (int64_t)a.boff[blockIdx.x] + block_exclusive(head ? 1u : 0u, wsum);
    if (i >= a.nk)
        return;
    a.hpos[i] = (int32_t)pos; // pos <= E <= nk
    if (!head)
        return;
    // the end of the run of k: sorted[lo] == k, sorted[hi] != k or hi == nk
    const unsigned long long k = a.sorted[i];
    int64_t lo = i, step = 1;
    while (i + step < a.nk && a.sorted[i + step] == k) {
        lo = i + step;
        step <<= 1;
    }
    int64_t hi = i + step < a.nk ? i + step : a.nk;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.sorted[mid] == k)
            lo = mid;
        else
            hi = mid;
    }
    const int32_t v = (int32_t)(k & ((1ull << a.nb) - 1ull)), run = (int32_t)(hi - i);
    a.nbr[pos] = v; // pos < nk: one entry at most per key
    a.cnt[pos] = run;
    if (pos < a.cap) {
        if (a.o_nbr)
            a.o_nbr[pos] = v;
        if (a.o_cnt)
            a.o_cnt[pos] = run;
    }
}

__global__ __launch_bounds__(kMeshLanes) void adj_offsets_kernel(AdjArgs a)
{
    const int64_t v = mesh_item();
    if (v > a.nv)
        return;
    // v <= nv < 2^nb: the key fits 2 nb <= 62 bits and is below the padding
    const unsigned long long key = (unsigned long long)v << a.nb;
    int64_t lo = 0, hi = a.nk;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.sorted[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int32_t o = lo < a.nk ? a.hpos[lo] : (int32_t)a.boff[a.nbk];
    a.off[v] = o;
    if (a.o_off)
        a.o_off[v] = o;
}

__global__ __launch_bounds__(kMeshLanes) void adj_rows_kernel(AdjArgs a)
{
    const int64_t v = mesh_item();
    int32_t len = 0;
    unsigned long long nbd = 0, nn = 0;
    uint8_t flag = 0;
    if (v < a.nv) {
        const int32_t lo = a.off[v], hi = a.off[v + 1];
        len = hi - lo;
        for (int32_t e = lo; e < hi; ++e) {
            const int32_t c = a.cnt[e];
            nbd += c == 1 ? 1ull : 0ull;
            nn += c > 2 ? 1ull : 0ull;
        }
        flag = (uint8_t)((nbd ? DP_VERTEX_BOUNDARY : 0) | (nn ? DP_VERTEX_NONMANIFOLD : 0));
        a.vflags[v] = flag;
        if (a.o_flags)
            a.o_flags[v] = flag;
    }
    smooth_count(a.count, 2, v < a.nv && len == 0 ? 1ull : 0ull);
    smooth_count(a.count, 3, nbd);
    smooth_count(a.count, 4, nn);
    smooth_count(a.count, 5, (flag & DP_VERTEX_BOUNDARY) ? 1ull : 0ull);
    int32_t m = len;
    for (int o = 32; o > 0; o >>= 1)
        m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0)
        atomicMax(a.maxval, m);
}

__global__ __launch_bounds__(kMeshLanes) void smooth_unpack_kernel(SmoothArgs a)
{
    const int64_t v = mesh_item();
    if (v >= a.nv)
        return;
    const float *p = a.verts[v].pos;
    const float x = p[0], y = p[1], z = p[2];
    a.dst[3 * v] = x;
    a.dst[3 * v + 1] = y;
    a.dst[3 * v + 2] = z;
}

__global__ __launch_bounds__(kMeshLanes) void smooth_step_kernel(SmoothArgs a)
{
    const int64_t v = mesh_item();
    if (v >= a.nv)
        return;
    const float px = a.src[3 * v], py = a.src[3 * v + 1], pz = a.src[3 * v + 2];
    const int32_t lo = a.off[v], hi = a.off[v + 1];
    float ox = px, oy = py, oz = pz;
    if (hi > lo && !(a.pin && (a.vflags[v] & DP_VERTEX_BOUNDARY))) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int32_t e = lo; e < hi; ++e) {
            const float *q = a.src + 3 * (int64_t)a.nbr[e]; // a neighbour is a vertex of a proper triangle: < nv
            sx = sx + (double)q[0];
            sy = sy + (double)q[1];
            sz = sz + (double)q[2];
        }
        const double n = (double)(hi - lo);
        const double mx = dpg::dvdiv(sx, n), my = dpg::dvdiv(sy, n), mz = dpg::dvdiv(sz, n);
        const double x = (double)px, y = (double)py, z = (double)pz;
        ox = (float)(x + a.f * (mx - x));
        oy = (float)(y + a.f * (my - y));
        oz = (float)(z + a.f * (mz - z));
    }
    a.dst[3 * v] = ox;
    a.dst[3 * v + 1] = oy;
    a.dst[3 * v + 2] = oz;
}

__global__ __launch_bounds__(kMeshLanes) void smooth_pack_kernel(SmoothArgs a)
{
    const int64_t v = mesh_item();
    if (v >= a.nv)
        return;
    // a record is 16 bytes with 4-byte alignment: three position words and the colour word, pad included
    const uint32_t *pos = (const uint32_t *)(a.src + 3 * v);
    const uint32_t w0 = pos[0], w1 = pos[1], w2 = pos[2], w3 = ((const uint32_t *)(a.verts + v))[3];
    uint32_t *dst = (uint32_t *)(a.out + v);
    dst[0] = w0;
    dst[1] = w1;
    dst[2] = w2;
    dst[3] = w3;
}

__global__ __launch_bounds__(kMeshLanes) void normal_keys_kernel(NormalArgs a)
{
    const int64_t t = mesh_item();
    int32_t v[3] = {0, 0, 0};
    bool valid, proper;
    classify(a.tris, a.nt, a.nv, t, v, valid, proper);
    if (t < a.nt)
        for (int e = 0; e < 3; ++e) { // 3 t + 2 < n3
            a.ikeys[3 * t + e] = proper ? (uint32_t)v[e] : kPadVertex;
            a.itris[3 * t + e] = (int32_t)t;
        }
    smooth_count(a.count, 0, t < a.nt && !valid ? 1ull : 0ull);
    smooth_count(a.count, 1, valid && !proper ? 1ull : 0ull);
}

// the first pair of the sorted pairs whose vertex is >= v
__device__ __forceinline__ int64_t first_pair(const NormalArgs &a, uint32_t v)
{
    int64_t lo = 0, hi = a.n3;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.ikeys_sorted[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMeshLanes) void normal_vertex_kernel(NormalArgs a)
{
    const int64_t v = mesh_item();
    bool zero = false;
    if (v < a.nv) {
        // v + 1 <= nv <= 2^31 - 1, below the padding
        const int64_t lo = first_pair(a, (uint32_t)v), hi = first_pair(a, (uint32_t)v + 1u);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int64_t e = lo; e < hi; ++e) {
            // a pair with a vertex below the padding names a proper triangle: t < nt, its indices < nv
            const int32_t *tri = a.tris + 3 * (int64_t)a.itris_sorted[e];
            const float *p0 = a.verts[tri[0]].pos, *p1 = a.verts[tri[1]].pos, *p2 = a.verts[tri[2]].pos;
            const double e1x = (double)p1[0] - (double)p0[0], e1y = (double)p1[1] - (double)p0[1],
                         e1z = (double)p1[2] - (double)p0[2];
            const double e2x = (double)p2[0] - (double)p0[0], e2y = (double)p2[1] - (double)p0[1],
                         e2z = (double)p2[2] - (double)p0[2];
            sx = sx + (e1y * e2z - e1z * e2y);
            sy = sy + (e1z * e2x - e1x * e2z);
            sz = sz + (e1x * e2y - e1y * e2x);
        }
        const double l2 = (sx * sx + sy * sy) + sz * sz;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (l2 > 0.0 && l2 <= 1.7976931348623157e308) {
            const double l = dpg::dvsqrt(l2);
            nx = (float)dpg::dvdiv(sx, l);
            ny = (float)dpg::dvdiv(sy, l);
            nz = (float)dpg::dvdiv(sz, l);
        } else {
            zero = true;
        }
        a.normals[3 * v] = nx;
        a.normals[3 * v + 1] = ny;
        a.normals[3 * v + 2] = nz;
    }
    smooth_count(a.count, 6, zero ? 1ull : 0ull);
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mesh_smooth_options(dp_mesh_smooth_options *mso)
{
    if (!mso)
        return;
    *mso = dp_mesh_smooth_options{};
    mso->iterations = 10;
    mso->lambda = 0.5f;
    mso->mu = -0.53f;
}

namespace {

using dpk::AdjArgs;
using dpk::kSmoothCounters;
using dpk::kSmoothStripes;
using dpk::mesh_blocks;
using dpk::NormalArgs;
using dpk::SmoothArgs;

struct AdjRun {
    AdjArgs a{};
    size_t tmp_bytes = 0;
    int end_bit = 1;
};

// the bits of n: the least nb with n < 2^nb
int bits_of(int64_t n)
{
    int nb = 0;
    while ((n >> nb) != 0)
        ++nb;
    return nb;
}

int smooth_check_entries(dp_ctx *c, const std::string &w, int64_t nt)
{
    if (6 * nt > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": 6 * n_triangles must be <= 2^31 - 1 (offsets are int32)");
    return DP_OK;
}

int smooth_check_options(dp_ctx *c, const std::string &w, const dp_mesh_smooth_options &o)
{
    if (o.iterations < 0 || o.iterations > 1000)
        return fail(c, DP_E_ARG, w + ": iterations must be in 0..1000");
    if (!(o.lambda > 0.0f && o.lambda <= 1.0f))
        return fail(c, DP_E_ARG, w + ": lambda must be in (0, 1]");
    if (!(o.mu <= 0.0f) || std::isinf(o.mu))
        return fail(c, DP_E_ARG, w + ": mu must be finite and <= 0");
    if (o.flags & ~DP_SMOOTH_FREE_BOUNDARY)
        return fail(c, DP_E_ARG, w + ": unknown flag bits");
    return DP_OK;
}

int smooth_counters(dp_ctx *c)
{
    DP_HIP(c, c->smooth.count.reserve(kSmoothStripes, kSmoothCounters, 2)); // + E, the largest valence
    return DP_OK;
}

// the scratch of an adjacency and the sizes of the hipcub calls
int adj_prepare(dp_ctx *c, const int32_t *d_tris, int64_t nt, int64_t nv, hipStream_t s, AdjRun &run)
{
    AdjArgs &a = run.a;
    dpk::MeshSmoothScratch &m = c->smooth;
    a.tris = d_tris;
    a.nt = nt;
    a.nv = nv;
    a.nk = 6 * nt;
    a.nbt = mesh_blocks(nt);
    a.nbv = mesh_blocks(nv);
    a.nbk = mesh_blocks(a.nk);
    a.nb = bits_of(nv);
    run.end_bit = std::max(2 * a.nb, 1);
    const size_t nk = (size_t)std::max<int64_t>(a.nk, 1);
    DP_HIP(c, m.keys.reserve(nk));
    DP_HIP(c, m.keys_sorted.reserve(nk));
    DP_HIP(c, m.hpos.reserve(nk));
    DP_HIP(c, m.off.reserve((size_t)nv + 1));
    DP_HIP(c, m.vflags.reserve((size_t)std::max<int64_t>(nv, 1)));
    DP_HIP(c, m.maxval.reserve(1));
    DP_HIP(c, m.bcount.reserve((size_t)a.nbk + 1));
    DP_HIP(c, m.boff.reserve((size_t)a.nbk + 1));
    int rc = smooth_counters(c);
    if (rc != DP_OK)
        return rc;
    a.keys = m.keys.p;
    a.sorted = m.keys_sorted.p;
    a.nbr = (int32_t *)m.keys.p;
    a.cnt = a.nbr + a.nk;
    a.hpos = m.hpos.p;
    a.off = m.off.p;
    a.vflags = m.vflags.p;
    a.maxval = m.maxval.p;
    a.bcount = m.bcount.p;
    a.boff = m.boff.p;
    a.count = m.count.dev.p;
    size_t b = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, a.bcount, a.boff, (int)a.nbk + 1, s));
    run.tmp_bytes = b;
    if (a.nk > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortKeys(nullptr, b, a.keys, a.sorted, (int)a.nk, 0, run.end_bit, s));
        run.tmp_bytes = std::max(run.tmp_bytes, b);
    }
    DP_HIP(c, c->scan_tmp.reserve(run.tmp_bytes ? run.tmp_bytes : 1));
    return DP_OK;
}

// queues the whole adjacency, the counters zeroed first
int adj_build(dp_ctx *c, AdjRun &run, hipStream_t s)
{
    const AdjArgs &a = run.a;
    size_t b = run.tmp_bytes;
    DP_HIP(c, c->smooth.count.zero(s));
    DP_HIP(c, hipMemsetAsync(a.maxval, 0, sizeof(int32_t), s));
    DP_HIP(c, hipMemsetAsync(a.bcount + a.nbk, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_over(dpk::adj_keys_kernel, a.nbt, a, s));
    if (a.nk > 0)
        DP_HIP(c, hipcub::DeviceRadixSort::SortKeys(c->scan_tmp.p, b, a.keys, a.sorted, (int)a.nk, 0, run.end_bit, s));
    DP_HIP(c, dpk::launch_over(dpk::adj_heads_kernel, a.nbk, a, s));
    b = run.tmp_bytes;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, a.bcount, a.boff, (int)a.nbk + 1, s));
    DP_HIP(c, dpk::launch_over(dpk::adj_emit_kernel, a.nbk, a, s));
    DP_HIP(c, dpk::launch_over(dpk::adj_offsets_kernel, mesh_blocks(a.nv + 1), a, s));
    DP_HIP(c, dpk::launch_over(dpk::adj_rows_kernel, a.nbv, a, s));
    return DP_OK;
}

// queues the copies of the counters and, behind them, E and the largest valence
int adj_read(dp_ctx *c, const AdjRun &run, hipStream_t s)
{
    unsigned long long *h = c->smooth.count.extra();
    h[0] = h[1] = 0;
    DP_HIP(c, c->smooth.count.read(s));
    DP_HIP(c, hipMemcpyAsync(h, run.a.boff + run.a.nbk, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + 1, run.a.maxval, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return DP_OK;
}

dp_mesh_adjacency_stats adj_stats(dp_ctx *c, const AdjRun &run, double ms)
{
    const dpk::StripedCounters &k = c->smooth.count;
    const unsigned long long *h = c->smooth.count.extra();
    dp_mesh_adjacency_stats r{};
    r.vertices_in = run.a.nv;
    r.triangles_in = run.a.nt;
    r.invalid_triangles = k.sum(0);
    r.degenerate_triangles = k.sum(1);
    r.isolated_vertices = k.sum(2);
    r.edges = (int64_t)h[0] / 2;
    r.boundary_edges = k.sum(3) / 2;
    r.nonmanifold_edges = k.sum(4) / 2;
    r.boundary_vertices = k.sum(5);
    r.max_valence = (int64_t)(int32_t)(uint32_t)h[1];
    r.adjacency_ms = ms;
    return r;
}

// queues the steps of a smoothing of d_verts into d_out behind the adjacency of `run`; returns the steps
int smooth_steps(dp_ctx *c, const AdjRun &run, const dp_mesh_smooth_options &o, const dp_mesh_vertex *d_verts,
                 dp_mesh_vertex *d_out, hipStream_t s, int64_t &steps)
{
    const int64_t nv = run.a.nv, nbv = run.a.nbv;
    steps = 0;
    DP_HIP(c, c->smooth.pos[0].reserve((size_t)std::max<int64_t>(3 * nv, 1)));
    DP_HIP(c, c->smooth.pos[1].reserve((size_t)std::max<int64_t>(3 * nv, 1)));
    SmoothArgs a{};
    a.verts = d_verts;
    a.out = d_out;
    a.nv = nv;
    a.off = run.a.off;
    a.nbr = run.a.nbr;
    a.vflags = run.a.vflags;
    a.pin = (o.flags & DP_SMOOTH_FREE_BOUNDARY) ? 0 : 1;
    int cur = 0;
    a.dst = c->smooth.pos[cur].p;
    DP_HIP(c, dpk::launch_over(dpk::smooth_unpack_kernel, nbv, a, s));
    for (int it = 0; it < o.iterations; ++it)
        for (int half = 0; half < 2; ++half) {
            if (half == 1 && o.mu == 0.0f)
                continue;
            a.f = (double)(half == 0 ? o.lambda : o.mu);
            a.src = c->smooth.pos[cur].p;
            a.dst = c->smooth.pos[cur ^ 1].p;
            DP_HIP(c, dpk::launch_over(dpk::smooth_step_kernel, nbv, a, s));
            cur ^= 1;
            ++steps;
        }
    a.src = c->smooth.pos[cur].p;
    DP_HIP(c, dpk::launch_over(dpk::smooth_pack_kernel, nbv, a, s));
    return DP_OK;
}

dp_mesh_smooth_stats smooth_stats(const dp_mesh_adjacency_stats &j, const dp_mesh_smooth_options &o, int64_t steps,
                                  double ms)
{
    dp_mesh_smooth_stats r{};
    r.vertices_in = j.vertices_in;
    r.triangles_in = j.triangles_in;
    r.invalid_triangles = j.invalid_triangles;
    r.degenerate_triangles = j.degenerate_triangles;
    r.isolated_vertices = j.isolated_vertices;
    r.edges = j.edges;
    r.boundary_edges = j.boundary_edges;
    r.nonmanifold_edges = j.nonmanifold_edges;
    r.boundary_vertices = j.boundary_vertices;
    r.max_valence = j.max_valence;
    // a boundary vertex has an incident edge: its row is not empty
    r.pinned_vertices = (o.flags & DP_SMOOTH_FREE_BOUNDARY) ? 0 : j.boundary_vertices;
    r.movable_vertices = j.vertices_in - j.isolated_vertices - r.pinned_vertices;
    r.steps = steps;
    r.adjacency_ms = j.adjacency_ms;
    r.smooth_ms = ms;
    return r;
}

// queues the normals of a device mesh: the keys, the sort, the walk
int normals_build(dp_ctx *c, const dp_mesh_vertex *d_verts, int64_t nv, const int32_t *d_tris, int64_t nt,
                  float *d_normals, hipStream_t s)
{
    dpk::MeshSmoothScratch &m = c->smooth;
    NormalArgs a{};
    a.tris = d_tris;
    a.verts = d_verts;
    a.nt = nt;
    a.nv = nv;
    a.n3 = 3 * nt;
    const size_t n3 = (size_t)std::max<int64_t>(a.n3, 1);
    DP_HIP(c, m.ikeys.reserve(n3));
    DP_HIP(c, m.ikeys_sorted.reserve(n3));
    DP_HIP(c, m.itris.reserve(n3));
    DP_HIP(c, m.itris_sorted.reserve(n3));
    int rc = smooth_counters(c);
    if (rc != DP_OK)
        return rc;
    a.ikeys = m.ikeys.p;
    a.ikeys_sorted = m.ikeys_sorted.p;
    a.itris = m.itris.p;
    a.itris_sorted = m.itris_sorted.p;
    a.normals = d_normals;
    a.count = m.count.dev.p;
    const int end_bit = std::max(bits_of(nv), 1);
    size_t b = 0;
    if (a.n3 > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.ikeys, a.ikeys_sorted, a.itris, a.itris_sorted,
                                                     (int)a.n3, 0, end_bit, s));
        DP_HIP(c, c->scan_tmp.reserve(b ? b : 1));
    }
    DP_HIP(c, m.count.zero(s));
    DP_HIP(c, dpk::launch_over(dpk::normal_keys_kernel, mesh_blocks(nt), a, s));
    if (a.n3 > 0)
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.ikeys, a.ikeys_sorted, a.itris, a.itris_sorted,
                                                     (int)a.n3, 0, end_bit, s));
    DP_HIP(c, dpk::launch_over(dpk::normal_vertex_kernel, mesh_blocks(nv), a, s));
    return DP_OK;
}

dp_mesh_normals_stats normals_stats(dp_ctx *c, int64_t nv, int64_t nt, double ms)
{
    const dpk::StripedCounters &k = c->smooth.count;
    dp_mesh_normals_stats r{};
    r.vertices_in = nv;
    r.triangles_in = nt;
    r.invalid_triangles = k.sum(0);
    r.degenerate_triangles = k.sum(1);
    r.zero_normals = k.sum(6);
    r.normals_ms = ms;
    return r;
}

int section_ms(dp_ctx *c, int k, double &ms)
{
    DP_HIP(c, c->smooth.time[k].ms(ms));
    return DP_OK;
}

} // namespace

extern "C" int dp_mesh_adjacency_device(dp_ctx *c, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices,
                                        int32_t *d_offsets, int32_t *d_neighbours, int32_t *d_edge_triangles,
                                        int64_t entry_cap, uint8_t *d_vertex_flags, int64_t *n_entries,
                                        dp_mesh_adjacency_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_adjacency_device";
    int rc = n_triangles >= 0 && n_vertices >= 0 ? smooth_check_entries(c, w, n_triangles) : DP_OK;
    if (rc == DP_OK)
        rc = mesh_check_counts(c, w, d_triangles, n_triangles, n_vertices);
    if (rc == DP_OK && !n_entries)
        rc = fail(c, DP_E_ARG, w + ": n_entries must be given");
    if (rc == DP_OK && entry_cap < 0)
        rc = fail(c, DP_E_ARG, w + ": a cap must be >= 0");
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {d_offsets, d_neighbours, d_edge_triangles, d_vertex_flags}, {d_triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    AdjRun run;
    if ((rc = adj_prepare(c, d_triangles, n_triangles, n_vertices, s, run)) != DP_OK)
        return rc;
    run.a.o_off = d_offsets;
    run.a.o_nbr = d_neighbours;
    run.a.o_cnt = d_edge_triangles;
    run.a.cap = entry_cap;
    run.a.o_flags = d_vertex_flags;
    DP_HIP(c, c->smooth.time[0].begin(s));
    if ((rc = adj_build(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].end(s));
    // the one wait: the counts and statistics
    if ((rc = adj_read(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = section_ms(c, 0, ms)) != DP_OK)
        return rc;
    *n_entries = (int64_t)c->smooth.count.extra()[0];
    if (stats)
        *stats = adj_stats(c, run, ms);
    return DP_OK;
}

extern "C" int dp_mesh_adjacency(dp_ctx *c, const int32_t *triangles, int64_t n_triangles, int64_t n_vertices,
                                 const int32_t **offsets, const int32_t **neighbours, const int32_t **edge_triangles,
                                 const uint8_t **vertex_flags, int64_t *n_entries, dp_mesh_adjacency_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_adjacency";
    int rc = n_triangles >= 0 && n_vertices >= 0 ? smooth_check_entries(c, w, n_triangles) : DP_OK;
    if (rc == DP_OK)
        rc = mesh_check_counts(c, w, triangles, n_triangles, n_vertices);
    if (rc == DP_OK && !n_entries)
        rc = fail(c, DP_E_ARG, w + ": n_entries must be given");
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    DP_HIP(c, c->smooth.in.reserve((size_t)std::max<int64_t>(12 * nt, 1)));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.in.p, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    AdjRun run;
    if ((rc = adj_prepare(c, (const int32_t *)c->smooth.in.p, nt, nv, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].begin(s));
    if ((rc = adj_build(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].end(s));
    // E sizes the host copies of the rows
    if ((rc = adj_read(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    const int64_t E = (int64_t)c->smooth.count.extra()[0];
    // pinned: the offsets, then the neighbours, then the counts
    DP_HIP(c, c->smooth.hcsr.resize((size_t)(nv + 1 + 2 * E)));
    DP_HIP(c, c->smooth.hflags.resize((size_t)std::max<int64_t>(nv, 1)));
    int32_t *h = c->smooth.hcsr.data();
    DP_HIP(c, hipMemcpyAsync(h, run.a.off, 4 * (size_t)(nv + 1), hipMemcpyDeviceToHost, s));
    if (E > 0) {
        DP_HIP(c, hipMemcpyAsync(h + nv + 1, run.a.nbr, 4 * (size_t)E, hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipMemcpyAsync(h + nv + 1 + E, run.a.cnt, 4 * (size_t)E, hipMemcpyDeviceToHost, s));
    }
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.hflags.data(), run.a.vflags, (size_t)nv, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = section_ms(c, 0, ms)) != DP_OK)
        return rc;
    if (offsets)
        *offsets = h;
    if (neighbours)
        *neighbours = E > 0 ? h + nv + 1 : nullptr;
    if (edge_triangles)
        *edge_triangles = E > 0 ? h + nv + 1 + E : nullptr;
    if (vertex_flags)
        *vertex_flags = nv > 0 ? c->smooth.hflags.data() : nullptr;
    *n_entries = E;
    if (stats)
        *stats = adj_stats(c, run, ms);
    return DP_OK;
}

extern "C" int dp_mesh_smooth_device(dp_ctx *c, const dp_mesh_smooth_options *mso, const dp_mesh_vertex *d_vertices,
                                     int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                                     dp_mesh_vertex *d_vertices_out, dp_mesh_smooth_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_smooth_device";
    dp_mesh_smooth_options o;
    dp_default_mesh_smooth_options(&o);
    if (mso)
        o = *mso;
    int rc = n_triangles >= 0 && n_vertices >= 0 ? smooth_check_entries(c, w, n_triangles) : DP_OK;
    if (rc == DP_OK)
        rc = mesh_check_counts(c, w, d_triangles, n_triangles, n_vertices);
    if (rc == DP_OK && n_vertices > 0 && (!d_vertices || !d_vertices_out))
        rc = fail(c, DP_E_ARG, w + ": vertices and vertices_out must be given");
    if (rc == DP_OK)
        rc = smooth_check_options(c, w, o);
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {d_vertices_out}, {d_vertices, d_triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    AdjRun run;
    if ((rc = adj_prepare(c, d_triangles, n_triangles, n_vertices, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].begin(s));
    if ((rc = adj_build(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].end(s));
    int64_t steps = 0;
    DP_HIP(c, c->smooth.time[1].begin(s));
    if ((rc = smooth_steps(c, run, o, d_vertices, d_vertices_out, s, steps)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[1].end(s));
    if (!stats)
        return DP_OK;
    // the one wait: the statistics
    if ((rc = adj_read(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    double ams = 0.0, sms = 0.0;
    if ((rc = section_ms(c, 0, ams)) != DP_OK || (rc = section_ms(c, 1, sms)) != DP_OK)
        return rc;
    *stats = smooth_stats(adj_stats(c, run, ams), o, steps, sms);
    return DP_OK;
}

extern "C" int dp_mesh_smooth(dp_ctx *c, const dp_mesh_smooth_options *mso, const dp_mesh_vertex *vertices,
                              int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                              const dp_mesh_vertex **vertices_out, dp_mesh_smooth_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_smooth";
    dp_mesh_smooth_options o;
    dp_default_mesh_smooth_options(&o);
    if (mso)
        o = *mso;
    int rc = n_triangles >= 0 && n_vertices >= 0 ? smooth_check_entries(c, w, n_triangles) : DP_OK;
    if (rc == DP_OK)
        rc = mesh_check_counts(c, w, triangles, n_triangles, n_vertices);
    if (rc == DP_OK && n_vertices > 0 && !vertices)
        rc = fail(c, DP_E_ARG, w + ": vertices must be given");
    if (rc == DP_OK)
        rc = smooth_check_options(c, w, o);
    if (rc == DP_OK && !vertices_out)
        rc = fail(c, DP_E_ARG, w + ": vertices_out must be given");
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    // staged inputs: the vertices (16 B each), then the triangles
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    DP_HIP(c, c->smooth.in.reserve(std::max<size_t>(vbytes + 12 * (size_t)nt, 1)));
    DP_HIP(c, c->smooth.verts.reserve((size_t)std::max<int64_t>(nv, 1)));
    DP_HIP(c, c->smooth.hverts.resize((size_t)std::max<int64_t>(nv, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.in.p, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.in.p + vbytes, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    AdjRun run;
    if ((rc = adj_prepare(c, (const int32_t *)(c->smooth.in.p + vbytes), nt, nv, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].begin(s));
    if ((rc = adj_build(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[0].end(s));
    int64_t steps = 0;
    DP_HIP(c, c->smooth.time[1].begin(s));
    if ((rc = smooth_steps(c, run, o, (const dp_mesh_vertex *)c->smooth.in.p, c->smooth.verts.p, s, steps)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[1].end(s));
    if ((rc = adj_read(c, run, s)) != DP_OK)
        return rc;
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.hverts.data(), c->smooth.verts.p, vbytes, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ams = 0.0, sms = 0.0;
    if ((rc = section_ms(c, 0, ams)) != DP_OK || (rc = section_ms(c, 1, sms)) != DP_OK)
        return rc;
    *vertices_out = nv > 0 ? c->smooth.hverts.data() : nullptr;
    if (stats)
        *stats = smooth_stats(adj_stats(c, run, ams), o, steps, sms);
    return DP_OK;
}

namespace {

int normals_check(dp_ctx *c, const std::string &w, const void *verts, int64_t nv, const void *tris, int64_t nt)
{
    if (nt >= 0 && nv >= 0 && 3 * nt > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": 3 * n_triangles must be <= 2^31 - 1");
    int rc = mesh_check_counts(c, w, tris, nt, nv);
    if (rc == DP_OK && nv > 0 && !verts)
        rc = fail(c, DP_E_ARG, w + ": vertices must be given");
    return rc;
}

} // namespace

extern "C" int dp_mesh_normals_device(dp_ctx *c, const dp_mesh_vertex *d_vertices, int64_t n_vertices,
                                      const int32_t *d_triangles, int64_t n_triangles, float *d_normals,
                                      dp_mesh_normals_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_normals_device";
    int rc = normals_check(c, w, d_vertices, n_vertices, d_triangles, n_triangles);
    if (rc == DP_OK && n_vertices > 0 && !d_normals)
        rc = fail(c, DP_E_ARG, w + ": normals must be given");
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {d_normals}, {d_vertices, d_triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DP_HIP(c, c->smooth.time[1].begin(s));
    if ((rc = normals_build(c, d_vertices, n_vertices, d_triangles, n_triangles, d_normals, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[1].end(s));
    if (!stats)
        return DP_OK;
    // the one wait: the statistics
    DP_HIP(c, c->smooth.count.read(s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = section_ms(c, 1, ms)) != DP_OK)
        return rc;
    *stats = normals_stats(c, n_vertices, n_triangles, ms);
    return DP_OK;
}

extern "C" int dp_mesh_normals(dp_ctx *c, const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                               int64_t n_triangles, const float **normals, dp_mesh_normals_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_normals";
    int rc = normals_check(c, w, vertices, n_vertices, triangles, n_triangles);
    if (rc == DP_OK && !normals)
        rc = fail(c, DP_E_ARG, w + ": normals must be given");
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    DP_HIP(c, c->smooth.in.reserve(std::max<size_t>(vbytes + 12 * (size_t)nt, 1)));
    DP_HIP(c, c->smooth.normals.reserve((size_t)std::max<int64_t>(3 * nv, 1)));
    DP_HIP(c, c->smooth.hnormals.resize((size_t)std::max<int64_t>(3 * nv, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.in.p, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.in.p + vbytes, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    DP_HIP(c, c->smooth.time[1].begin(s));
    if ((rc = normals_build(c, (const dp_mesh_vertex *)c->smooth.in.p, nv, (const int32_t *)(c->smooth.in.p + vbytes), nt,
                            c->smooth.normals.p, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->smooth.time[1].end(s));
    DP_HIP(c, c->smooth.count.read(s));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->smooth.hnormals.data(), c->smooth.normals.p, 12 * (size_t)nv, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = section_ms(c, 1, ms)) != DP_OK)
        return rc;
    *normals = nv > 0 ? c->smooth.hnormals.data() : nullptr;
    if (stats)
        *stats = normals_stats(c, nv, nt, ms);
    return DP_OK;
}
