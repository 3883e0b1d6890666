// dp_meshclean.hip -- gfx950 kernels of the mesh clean-up (spec in
// include/densepoints.h, dp_mesh_components / dp_mesh_clean) and their C ABI.
//
//   clean_init_kernel      parent[v] = v, the flags and counts zero, the sort
//                          keys all ones (the padding of the rank sort)
//   clean_union_kernel     one lane per triangle: the guard, the USED stores
//                          (idempotent) and two unions of a lock-free union-find
//                          whose parents only ever decrease (parent[v] <= v), so
//                          the final root of a set is its smallest index whatever
//                          the schedule; no lane waits for another lane
//   clean_flatten_kernel   parent[v] = root(v) (the label), the used vertices
//                          per root, the roots per block
//   clean_tricount_kernel  the valid triangles per root
//   (hipcub max of the per-root triangle counts = Tmax; exclusive scan of the
//   roots per block)
//   clean_number_kernel    roots numbered in ascending order, the table rows,
//                          the sort keys (Tmax - T_c) << 32 | c
//   (one hipcub radix sort of the keys: the position of c's key is rank(c))
//   clean_select_kernel    rank and KEPT per component
//   clean_label_kernels    vertex_component / triangle_component
//   clean_vcount / tcount  kept vertices / triangles per block (two scans)
//   clean_vemit / temit    the kept records at the scanned offset plus the rank
//                          in the block, each compared with its cap before the
//                          write; the maps
//
// The per-root counts are integer atomicAdds, aggregated in the wave first: a
// real mesh is one huge component plus dust, so nearly every lane of a wave
// holds the same root; the wave loops over the distinct roots of its lanes and
// one lane issues one add per distinct root.
//
// Every index read from a triangle is compared with n_vertices before it is
// used as an address: an invalid triangle reaches neither parent[] nor the
// vertex array.
#include "dp_meshdev.h"
#include "dp_wave.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

constexpr int kCleanBlock = kMeshLanes;
constexpr int kCleanStripes = 64;  // each counter kept kCleanStripes times (summed by the host)
constexpr int kCleanCounters = 3;  // invalid triangles, used vertices, kept components
constexpr unsigned long long kPadKey = ~0ull;

struct CleanArgs {
    const int32_t *tris;          // nt x 3
    const dp_mesh_vertex *verts;  // nv (the clean only)
    int64_t nt, nv;
    int64_t nbt, nbv;             // blocks over the triangles, over the vertices
    int32_t *parent, *tcnt, *vcnt, *cnum, *vmap, *tmax;
    uint8_t *used, *keptc;
    unsigned long long *keys, *keys_sorted;
    unsigned long long *bcount, *boff; // three segments: roots [nbv + 1], kept vertices [nbv + 1], kept triangles [nbt + 1]
    unsigned long long *count;         // kCleanStripes x kCleanCounters
    int64_t nsort;                     // keys sorted: C where the host knows it, else nv (padded)
    // selection
    int64_t min_triangles;
    float min_fraction;
    int32_t max_components;
    // outputs, any may be null
    dp_mesh_component *comps;
    int64_t ccap;
    int32_t *vcomp, *tcomp;
    dp_mesh_vertex *vout;
    int64_t vcap;
    int32_t *tout;
    int64_t tcap;
    int32_t *vmap_out, *tmap_out;
};

__device__ __forceinline__ int64_t seg_roots(const CleanArgs &) { return 0; }
__device__ __forceinline__ int64_t seg_verts(const CleanArgs &a) { return a.nbv + 1; }
__device__ __forceinline__ int64_t seg_tris(const CleanArgs &a) { return 2 * (a.nbv + 1); }

__device__ __forceinline__ int64_t item_of() { return mesh_item(); }

// parent[] is read and linked by many lanes at once: the loads are atomic, so a
// lane never acts on a cached copy that another lane's link has replaced
__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t v)
{
    return __hip_atomic_load(&parent[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v: a strict descent (parent[x] < x off the root), halving the path
// on the way with atomicMin, which keeps parents decreasing
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t v)
{
    int32_t p = load_parent(parent, v);
    while (p != v) {
        const int32_t g = load_parent(parent, p);
        if (g != p)
            atomicMin(&parent[v], g);
        v = p;
        p = g;
    }
    return v;
}

// joins the sets of a and b: the larger root goes under the smaller.  A failed
// compare-and-swap means that root was linked by somebody else meanwhile; the
// value it returns is that link, so the next find starts below it.  Every
// iteration follows or makes a strictly decreasing step: the loop is bounded by
// the data and waits for nobody.
__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b)
            return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi)
            return;
        a = old;
        b = lo;
    }
}

// counter += the wave's sum of v, on the wave's stripe (every lane calls)
__device__ __forceinline__ void clean_count(const CleanArgs &a, int counter, unsigned long long v)
{
    wave_count<kCleanStripes, kCleanCounters>(a.count, counter, v, blockIdx.x * (kCleanBlock / 64) + (threadIdx.x >> 6));
}

// cnt[key] += 1 for every lane with `on`, as one add per distinct key of the
// wave: the first pending lane's key is broadcast, the lanes that hold it are
// counted by a ballot and retire, and the first of them adds (every lane calls)
__device__ __forceinline__ void wave_add_by_key(int32_t *cnt, int32_t key, bool on)
{
    bool pending = on;
    while (__ballot(pending) != 0ull) {
        if (pending) {
            const int32_t k = uni(key);
            if (key == k) {
                const uint64_t same = __ballot(true);
                if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)same) - 1)
                    atomicAdd(&cnt[k], (int32_t)__popcll(same));
                pending = false;
            }
        }
    }
}

// the triangle's indices; false (and nothing else read) unless all three are vertices
__device__ __forceinline__ bool load_triangle(const CleanArgs &a, int64_t t, int32_t v[3])
{
    return load_valid_triangle(a.tris, a.nt, a.nv, t, v);
}

__global__ __launch_bounds__(kCleanBlock) void clean_init_kernel(CleanArgs a)
{
    const int64_t v = item_of();
    if (v >= a.nv)
        return;
    a.parent[v] = (int32_t)v;
    a.used[v] = 0;
    a.tcnt[v] = 0;
    a.vcnt[v] = 0;
    a.keys[v] = kPadKey;
}

__global__ __launch_bounds__(kCleanBlock) void clean_union_kernel(CleanArgs a)
{
    const int64_t t = item_of();
    int32_t v[3];
    const bool valid = load_triangle(a, t, v);
    if (valid) {
        a.used[v[0]] = 1;
        a.used[v[1]] = 1;
        a.used[v[2]] = 1;
        unite(a.parent, v[0], v[1]);
        unite(a.parent, v[0], v[2]);
    }
    clean_count(a, 0, t < a.nt && !valid ? 1ull : 0ull);
}

__global__ __launch_bounds__(kCleanBlock) void clean_flatten_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    const int64_t v = item_of();
    bool used = false, root = false;
    int32_t r = 0;
    if (v < a.nv) {
        r = find_root(a.parent, (int32_t)v);
        a.parent[v] = r; // a lane that still descends through v lands on its root
        used = a.used[v] != 0;
        root = used && r == (int32_t)v;
    }
    wave_add_by_key(a.vcnt, r, used);
    const uint32_t total = block_sum<kCleanBlock>(root ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_roots(a) + blockIdx.x] = total;
    clean_count(a, 1, used ? 1ull : 0ull);
}

__global__ __launch_bounds__(kCleanBlock) void clean_tricount_kernel(CleanArgs a)
{
    const int64_t t = item_of();
    int32_t v[3];
    const bool valid = load_triangle(a, t, v);
    wave_add_by_key(a.tcnt, valid ? a.parent[v[0]] : 0, valid);
}

__global__ __launch_bounds__(kCleanBlock) void clean_number_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    const int64_t v = item_of();
    const bool root = v < a.nv && a.used[v] != 0 && a.parent[v] == (int32_t)v;
    const int64_t c = (int64_t)a.boff[seg_roots(a) + blockIdx.x] + block_exclusive(root ? 1u : 0u, wsum);
    if (!root)
        return;
    // c <= v: one root at most per vertex below this one
    const int32_t T = a.tcnt[v], tmax = *a.tmax;
    a.cnum[v] = (int32_t)c;
    a.keys[c] = (unsigned long long)(uint32_t)(tmax - T) << 32 | (unsigned long long)c;
    if (c < a.ccap) {
        dp_mesh_component row;
        row.root = (int32_t)v;
        row.vertices = a.vcnt[v];
        row.triangles = T;
        row.rank = 0; // clean_select_kernel's
        a.comps[c] = row;
    }
}

__global__ __launch_bounds__(kCleanBlock) void clean_select_kernel(CleanArgs a)
{
    const int64_t r = item_of();
    bool kept = false;
    const unsigned long long key = r < a.nsort ? a.keys_sorted[r] : kPadKey;
    if (key != kPadKey) {
        const int64_t c = (int64_t)(key & 0xFFFFFFFFull);
        const int64_t tmax = (int64_t)*a.tmax, T = tmax - (int64_t)(key >> 32);
        kept = T >= a.min_triangles && (double)T >= (double)a.min_fraction * (double)tmax &&
               (a.max_components == 0 || r < (int64_t)a.max_components);
        a.keptc[c] = kept ? 1 : 0;
        if (c < a.ccap)
            a.comps[c].rank = (int32_t)r;
    }
    clean_count(a, 2, kept ? 1ull : 0ull);
}

__global__ __launch_bounds__(kCleanBlock) void clean_vlabel_kernel(CleanArgs a)
{
    const int64_t v = item_of();
    if (v < a.nv)
        a.vcomp[v] = a.used[v] ? a.cnum[a.parent[v]] : -1;
}

__global__ __launch_bounds__(kCleanBlock) void clean_tlabel_kernel(CleanArgs a)
{
    const int64_t t = item_of();
    int32_t v[3];
    const bool valid = load_triangle(a, t, v);
    if (t < a.nt)
        a.tcomp[t] = valid ? a.cnum[a.parent[v[0]]] : -1;
}

__device__ __forceinline__ bool vertex_kept(const CleanArgs &a, int64_t v)
{
    return v < a.nv && a.used[v] != 0 && a.keptc[a.cnum[a.parent[v]]] != 0;
}

__global__ __launch_bounds__(kCleanBlock) void clean_vcount_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    const uint32_t total = block_sum<kCleanBlock>(vertex_kept(a, item_of()) ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_verts(a) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kCleanBlock) void clean_tcount_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    int32_t v[3];
    const bool keep = load_triangle(a, item_of(), v) && a.keptc[a.cnum[a.parent[v[0]]]] != 0;
    const uint32_t total = block_sum<kCleanBlock>(keep ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_tris(a) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kCleanBlock) void clean_vemit_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    const int64_t v = item_of();
    const bool keep = vertex_kept(a, v);
    const int64_t id = (int64_t)a.boff[seg_verts(a) + blockIdx.x] + block_exclusive(keep ? 1u : 0u, wsum);
    if (v >= a.nv)
        return;
    a.vmap[v] = keep ? (int32_t)id : -1;
    if (a.vmap_out)
        a.vmap_out[v] = keep ? (int32_t)id : -1;
    if (keep && id < a.vcap) {
        // a record is 16 bytes with 4-byte alignment: four words, pad included
        const uint32_t *src = (const uint32_t *)(a.verts + v);
        uint32_t *dst = (uint32_t *)(a.vout + id);
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
        dst[0] = w0;
        dst[1] = w1;
        dst[2] = w2;
        dst[3] = w3;
    }
}

__global__ __launch_bounds__(kCleanBlock) void clean_temit_kernel(CleanArgs a)
{
    __shared__ uint32_t wsum[kCleanBlock / 64];
    const int64_t t = item_of();
    int32_t v[3];
    const bool keep = load_triangle(a, t, v) && a.keptc[a.cnum[a.parent[v[0]]]] != 0;
    const int64_t id = (int64_t)a.boff[seg_tris(a) + blockIdx.x] + block_exclusive(keep ? 1u : 0u, wsum);
    if (t >= a.nt)
        return;
    if (a.tmap_out)
        a.tmap_out[t] = keep ? (int32_t)id : -1;
    if (keep && id < a.tcap) {
        // the three vertices of a kept triangle are kept: they are in its component
        a.tout[3 * id] = a.vmap[v[0]];
        a.tout[3 * id + 1] = a.vmap[v[1]];
        a.tout[3 * id + 2] = a.vmap[v[2]];
    }
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mesh_clean_options(dp_mesh_clean_options *mco)
{
    if (!mco)
        return;
    *mco = dp_mesh_clean_options{};
    mco->min_triangles = 1;
}

namespace {

using dpk::CleanArgs;
using dpk::kCleanCounters;
using dpk::kCleanStripes;

struct CleanRun {
    CleanArgs a{};
    size_t tmp_bytes = 0;
};

int clean_check_options(dp_ctx *c, const std::string &w, const dp_mesh_clean_options &o)
{
    if (o.min_triangles < 0)
        return fail(c, DP_E_ARG, w + ": min_triangles must be >= 0");
    if (!(o.min_fraction >= 0.0f && o.min_fraction <= 1.0f))
        return fail(c, DP_E_ARG, w + ": min_fraction must be in 0..1");
    if (o.max_components < 0)
        return fail(c, DP_E_ARG, w + ": max_components must be >= 0");
    if (o.flags != 0)
        return fail(c, DP_E_ARG, w + ": unknown flag bits");
    return DP_OK;
}

// the scratch of a run and the sizes of the hipcub calls
int clean_prepare(dp_ctx *c, const int32_t *d_tris, int64_t nt, const dp_mesh_vertex *d_verts, int64_t nv,
                  const dp_mesh_clean_options &o, hipStream_t s, CleanRun &run)
{
    CleanArgs &a = run.a;
    a.tris = d_tris;
    a.verts = d_verts;
    a.nt = nt;
    a.nv = nv;
    a.nbt = (nt + dpk::kCleanBlock - 1) / dpk::kCleanBlock;
    a.nbv = (nv + dpk::kCleanBlock - 1) / dpk::kCleanBlock;
    a.nsort = nv;
    a.min_triangles = o.min_triangles;
    a.min_fraction = o.min_fraction;
    a.max_components = o.max_components;
    const size_t n = (size_t)std::max<int64_t>(nv, 1), nb = (size_t)(2 * (a.nbv + 1) + a.nbt + 1);
    DP_HIP(c, c->clean.parent.reserve(n));
    DP_HIP(c, c->clean.tcnt.reserve(n));
    DP_HIP(c, c->clean.vcnt.reserve(n));
    DP_HIP(c, c->clean.cnum.reserve(n));
    DP_HIP(c, c->clean.vmap.reserve(n));
    DP_HIP(c, c->clean.tmax.reserve(1));
    DP_HIP(c, c->clean.used.reserve(n));
    DP_HIP(c, c->clean.keptc.reserve(n));
    DP_HIP(c, c->clean.keys.reserve(n));
    DP_HIP(c, c->clean.keys_sorted.reserve(n));
    DP_HIP(c, c->clean.bcount.reserve(nb));
    DP_HIP(c, c->clean.boff.reserve(nb));
    DP_HIP(c, c->clean.count.reserve(kCleanStripes, kCleanCounters, 4)); // + C, VO, TO, Tmax
    a.parent = c->clean.parent.p;
    a.tcnt = c->clean.tcnt.p;
    a.vcnt = c->clean.vcnt.p;
    a.cnum = c->clean.cnum.p;
    a.vmap = c->clean.vmap.p;
    a.tmax = c->clean.tmax.p;
    a.used = c->clean.used.p;
    a.keptc = c->clean.keptc.p;
    a.keys = c->clean.keys.p;
    a.keys_sorted = c->clean.keys_sorted.p;
    a.bcount = c->clean.bcount.p;
    a.boff = c->clean.boff.p;
    a.count = c->clean.count.dev.p;
    size_t b = 0;
    const int nscan = (int)std::max(a.nbv, a.nbt) + 1;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, a.bcount, a.boff, nscan, s));
    run.tmp_bytes = b;
    if (nv > 0) {
        DP_HIP(c, hipcub::DeviceReduce::Max(nullptr, b, a.tcnt, a.tmax, (int)nv, s));
        run.tmp_bytes = std::max(run.tmp_bytes, b);
        DP_HIP(c, hipcub::DeviceRadixSort::SortKeys(nullptr, b, a.keys, a.keys_sorted, (int)nv, 0, 64, s));
        run.tmp_bytes = std::max(run.tmp_bytes, b);
    }
    DP_HIP(c, c->scan_tmp.reserve(run.tmp_bytes ? run.tmp_bytes : 1));
    return DP_OK;
}

// labels, per-root counts, Tmax and the number of components (the roots' scan)
int clean_label(dp_ctx *c, CleanRun &run, hipStream_t s)
{
    const CleanArgs &a = run.a;
    size_t b = run.tmp_bytes;
    DP_HIP(c, c->clean.count.zero(s));
    DP_HIP(c, hipMemsetAsync(a.tmax, 0, sizeof(int32_t), s));
    DP_HIP(c, hipMemsetAsync(a.bcount + a.nbv, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_over(dpk::clean_init_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_union_kernel, a.nbt, a, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_flatten_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_tricount_kernel, a.nbt, a, s));
    if (a.nv > 0)
        DP_HIP(c, hipcub::DeviceReduce::Max(c->scan_tmp.p, b, a.tcnt, a.tmax, (int)a.nv, s));
    b = run.tmp_bytes;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, a.bcount, a.boff, (int)a.nbv + 1, s));
    return DP_OK;
}

// component numbers, table rows, ranks and the selection
int clean_select(dp_ctx *c, CleanRun &run, hipStream_t s)
{
    const CleanArgs &a = run.a;
    size_t b = run.tmp_bytes;
    DP_HIP(c, dpk::launch_over(dpk::clean_number_kernel, a.nbv, a, s));
    if (a.nsort > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortKeys(c->scan_tmp.p, b, a.keys, a.keys_sorted, (int)a.nsort, 0, 64, s));
        DP_HIP(c, dpk::launch_over(dpk::clean_select_kernel, (a.nsort + dpk::kCleanBlock - 1) / dpk::kCleanBlock, a, s));
    }
    return DP_OK;
}

int clean_labels_out(dp_ctx *c, CleanRun &run, hipStream_t s)
{
    const CleanArgs &a = run.a;
    if (a.vcomp)
        DP_HIP(c, dpk::launch_over(dpk::clean_vlabel_kernel, a.nbv, a, s));
    if (a.tcomp)
        DP_HIP(c, dpk::launch_over(dpk::clean_tlabel_kernel, a.nbt, a, s));
    return DP_OK;
}

// the kept vertices and triangles per block and their scans
int clean_count_kept(dp_ctx *c, CleanRun &run, hipStream_t s)
{
    const CleanArgs &a = run.a;
    const int64_t sv = a.nbv + 1, st = 2 * (a.nbv + 1);
    size_t b = run.tmp_bytes;
    DP_HIP(c, hipMemsetAsync(a.bcount + sv + a.nbv, 0, sizeof(unsigned long long), s));
    DP_HIP(c, hipMemsetAsync(a.bcount + st + a.nbt, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_over(dpk::clean_vcount_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_tcount_kernel, a.nbt, a, s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, a.bcount + sv, a.boff + sv, (int)a.nbv + 1, s));
    b = run.tmp_bytes;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, a.bcount + st, a.boff + st, (int)a.nbt + 1, s));
    return DP_OK;
}

int clean_emit(dp_ctx *c, CleanRun &run, hipStream_t s)
{
    const CleanArgs &a = run.a;
    DP_HIP(c, dpk::launch_over(dpk::clean_vemit_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::clean_temit_kernel, a.nbt, a, s));
    return DP_OK;
}

// the counters and, behind them, C, (with `kept`) the kept totals and Tmax; waits
int clean_read(dp_ctx *c, const CleanRun &run, bool kept, hipStream_t s)
{
    const CleanArgs &a = run.a;
    unsigned long long *h = c->clean.count.extra();
    h[1] = h[2] = h[3] = 0;
    DP_HIP(c, c->clean.count.read(s));
    DP_HIP(c, hipMemcpyAsync(h, a.boff + a.nbv, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (kept) {
        DP_HIP(c, hipMemcpyAsync(h + 1, a.boff + (a.nbv + 1) + a.nbv, sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipMemcpyAsync(h + 2, a.boff + 2 * (a.nbv + 1) + a.nbt, sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, s));
    }
    DP_HIP(c, hipMemcpyAsync(h + 3, a.tmax, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}

// what clean_read read as statistics; without `kept` (dp_mesh_components) nothing was selected
dp_mesh_clean_stats clean_stats(dp_ctx *c, const CleanRun &run, bool kept, double ms)
{
    const unsigned long long *h = c->clean.count.extra();
    const int64_t sum[kCleanCounters] = {c->clean.count.sum(0), c->clean.count.sum(1), c->clean.count.sum(2)};
    dp_mesh_clean_stats r{};
    r.vertices_in = run.a.nv;
    r.triangles_in = run.a.nt;
    r.invalid_triangles = sum[0];
    r.unused_vertices = run.a.nv - sum[1];
    r.components = (int64_t)h[0];
    r.largest_triangles = (int64_t)(int32_t)(uint32_t)h[3];
    r.components_kept = kept ? sum[2] : r.components;
    r.vertices_out = kept ? (int64_t)h[1] : sum[1];
    r.triangles_out = kept ? (int64_t)h[2] : run.a.nt - sum[0];
    r.clean_ms = ms;
    return r;
}

// the time of the first `sections` timed sections
int clean_elapsed(dp_ctx *c, int sections, double &ms)
{
    ms = 0.0;
    for (int k = 0; k < sections; ++k) {
        double t = 0.0;
        DP_HIP(c, c->clean.time[k].ms(t));
        ms += t;
    }
    return DP_OK;
}

} // namespace

extern "C" int dp_mesh_components_device(dp_ctx *c, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices,
                                         int32_t *d_vertex_component, int32_t *d_triangle_component,
                                         dp_mesh_component *d_components, int64_t component_cap,
                                         int64_t *n_components, dp_mesh_clean_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_components_device";
    int rc = mesh_check_counts(c, w, d_triangles, n_triangles, n_vertices);
    if (rc == DP_OK && !n_components)
        rc = fail(c, DP_E_ARG, w + ": n_components must be given");
    if (rc == DP_OK)
        rc = mesh_check_cap(c, w, d_components, component_cap);
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {d_vertex_component, d_triangle_component, d_components}, {d_triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    dp_mesh_clean_options o;
    dp_default_mesh_clean_options(&o);
    CleanRun run;
    if ((rc = clean_prepare(c, d_triangles, n_triangles, nullptr, n_vertices, o, s, run)) != DP_OK)
        return rc;
    run.a.comps = d_components;
    run.a.ccap = component_cap;
    run.a.vcomp = d_vertex_component;
    run.a.tcomp = d_triangle_component;
    DP_HIP(c, c->clean.time[0].begin(s));
    if ((rc = clean_label(c, run, s)) != DP_OK || (rc = clean_select(c, run, s)) != DP_OK ||
        (rc = clean_labels_out(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].end(s));
    // the one wait: the counts and statistics
    if ((rc = clean_read(c, run, false, s)) != DP_OK)
        return rc;
    double ms = 0.0;
    if ((rc = clean_elapsed(c, 1, ms)) != DP_OK)
        return rc;
    const dp_mesh_clean_stats st = clean_stats(c, run, false, ms);
    *n_components = st.components;
    if (stats)
        *stats = st;
    return DP_OK;
}

extern "C" int dp_mesh_components(dp_ctx *c, const int32_t *triangles, int64_t n_triangles, int64_t n_vertices,
                                  int32_t *vertex_component, int32_t *triangle_component,
                                  const dp_mesh_component **components, int64_t *n_components,
                                  dp_mesh_clean_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_components";
    int rc = mesh_check_counts(c, w, triangles, n_triangles, n_vertices);
    if (rc == DP_OK && (!n_components || !components))
        rc = fail(c, DP_E_ARG, w + ": components and n_components must be given");
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {vertex_component, triangle_component}, {triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    DP_HIP(c, c->clean.in.reserve((size_t)std::max<int64_t>(12 * nt, 1)));
    DP_HIP(c, c->clean.maps.reserve((size_t)std::max<int64_t>(nv + nt, 1)));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.in.p, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    dp_mesh_clean_options o;
    dp_default_mesh_clean_options(&o);
    CleanRun run;
    if ((rc = clean_prepare(c, (const int32_t *)c->clean.in.p, nt, nullptr, nv, o, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].begin(s));
    if ((rc = clean_label(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].end(s));
    // the number of components sizes the table and the sort
    if ((rc = clean_read(c, run, false, s)) != DP_OK)
        return rc;
    const int64_t C = (int64_t)c->clean.count.extra()[0];
    DP_HIP(c, c->clean.comps.reserve((size_t)std::max<int64_t>(C, 1)));
    DP_HIP(c, c->clean.hcomps.resize((size_t)std::max<int64_t>(C, 1)));
    run.a.comps = c->clean.comps.p;
    run.a.ccap = C;
    run.a.nsort = C;
    run.a.vcomp = vertex_component ? c->clean.maps.p : nullptr;
    run.a.tcomp = triangle_component ? c->clean.maps.p + nv : nullptr;
    DP_HIP(c, c->clean.time[1].begin(s));
    if ((rc = clean_select(c, run, s)) != DP_OK || (rc = clean_labels_out(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[1].end(s));
    if (C > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.hcomps.data(), c->clean.comps.p, sizeof(dp_mesh_component) * (size_t)C,
                                 hipMemcpyDeviceToHost, s));
    if (vertex_component && nv > 0)
        DP_HIP(c, hipMemcpyAsync(vertex_component, run.a.vcomp, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
    if (triangle_component && nt > 0)
        DP_HIP(c, hipMemcpyAsync(triangle_component, run.a.tcomp, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = clean_elapsed(c, 2, ms)) != DP_OK)
        return rc;
    const dp_mesh_clean_stats st = clean_stats(c, run, false, ms);
    *components = C > 0 ? c->clean.hcomps.data() : nullptr;
    *n_components = C;
    if (stats)
        *stats = st;
    return DP_OK;
}

extern "C" int dp_mesh_clean_device(dp_ctx *c, const dp_mesh_clean_options *mco, const dp_mesh_vertex *d_vertices,
                                    int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                                    dp_mesh_vertex *d_vertices_out, int64_t vertex_cap, int64_t *n_vertices_out,
                                    int32_t *d_triangles_out, int64_t triangle_cap, int64_t *n_triangles_out,
                                    int32_t *d_vertex_map, int32_t *d_triangle_map, dp_mesh_clean_stats *stats,
                                    void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_clean_device";
    dp_mesh_clean_options o;
    dp_default_mesh_clean_options(&o);
    if (mco)
        o = *mco;
    int rc = mesh_check_counts(c, w, d_triangles, n_triangles, n_vertices);
    if (rc == DP_OK && n_vertices > 0 && !d_vertices)
        rc = fail(c, DP_E_ARG, w + ": vertices must be given");
    if (rc == DP_OK)
        rc = clean_check_options(c, w, o);
    if (rc == DP_OK && (!n_vertices_out || !n_triangles_out))
        rc = fail(c, DP_E_ARG, w + ": n_vertices_out and n_triangles_out must be given");
    if (rc == DP_OK)
        rc = mesh_check_cap(c, w, d_vertices_out, vertex_cap);
    if (rc == DP_OK)
        rc = mesh_check_cap(c, w, d_triangles_out, triangle_cap);
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {d_vertices_out, d_triangles_out, d_vertex_map, d_triangle_map},
                               {d_vertices, d_triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    CleanRun run;
    if ((rc = clean_prepare(c, d_triangles, n_triangles, d_vertices, n_vertices, o, s, run)) != DP_OK)
        return rc;
    run.a.vout = d_vertices_out;
    run.a.vcap = vertex_cap;
    run.a.tout = d_triangles_out;
    run.a.tcap = triangle_cap;
    run.a.vmap_out = d_vertex_map;
    run.a.tmap_out = d_triangle_map;
    DP_HIP(c, c->clean.time[0].begin(s));
    if ((rc = clean_label(c, run, s)) != DP_OK || (rc = clean_select(c, run, s)) != DP_OK ||
        (rc = clean_count_kept(c, run, s)) != DP_OK || (rc = clean_emit(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].end(s));
    // the one wait: the counts and statistics
    if ((rc = clean_read(c, run, true, s)) != DP_OK)
        return rc;
    double ms = 0.0;
    if ((rc = clean_elapsed(c, 1, ms)) != DP_OK)
        return rc;
    const dp_mesh_clean_stats st = clean_stats(c, run, true, ms);
    *n_vertices_out = st.vertices_out;
    *n_triangles_out = st.triangles_out;
    if (stats)
        *stats = st;
    return DP_OK;
}

extern "C" int dp_mesh_clean(dp_ctx *c, const dp_mesh_clean_options *mco, const dp_mesh_vertex *vertices,
                             int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                             const dp_mesh_vertex **vertices_out, int64_t *n_vertices_out,
                             const int32_t **triangles_out, int64_t *n_triangles_out, int32_t *vertex_map,
                             int32_t *triangle_map, dp_mesh_clean_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_clean";
    dp_mesh_clean_options o;
    dp_default_mesh_clean_options(&o);
    if (mco)
        o = *mco;
    int rc = mesh_check_counts(c, w, triangles, n_triangles, n_vertices);
    if (rc == DP_OK && n_vertices > 0 && !vertices)
        rc = fail(c, DP_E_ARG, w + ": vertices must be given");
    if (rc == DP_OK)
        rc = clean_check_options(c, w, o);
    if (rc == DP_OK && (!n_vertices_out || !n_triangles_out || !vertices_out || !triangles_out))
        rc = fail(c, DP_E_ARG, w + ": the result and count pointers must be given");
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {vertex_map, triangle_map}, {vertices, triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    // staged inputs: the vertices (16 B each), then the triangles
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    DP_HIP(c, c->clean.in.reserve(std::max<size_t>(vbytes + 12 * (size_t)nt, 1)));
    DP_HIP(c, c->clean.maps.reserve((size_t)std::max<int64_t>(nv + nt, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.in.p, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.in.p + vbytes, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    CleanRun run;
    if ((rc = clean_prepare(c, (const int32_t *)(c->clean.in.p + vbytes), nt, (const dp_mesh_vertex *)c->clean.in.p, nv, o,
                            s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].begin(s));
    if ((rc = clean_label(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[0].end(s));
    // the number of components sizes the sort
    if ((rc = clean_read(c, run, false, s)) != DP_OK)
        return rc;
    run.a.nsort = (int64_t)c->clean.count.extra()[0];
    DP_HIP(c, c->clean.time[1].begin(s));
    if ((rc = clean_select(c, run, s)) != DP_OK || (rc = clean_count_kept(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[1].end(s));
    // the kept totals size the results
    if ((rc = clean_read(c, run, true, s)) != DP_OK)
        return rc;
    const unsigned long long *h = c->clean.count.extra();
    const int64_t vo = (int64_t)h[1], to = (int64_t)h[2];
    DP_HIP(c, c->clean.verts.reserve((size_t)std::max<int64_t>(vo, 1)));
    DP_HIP(c, c->clean.tris.reserve((size_t)std::max<int64_t>(3 * to, 1)));
    DP_HIP(c, c->clean.hverts.resize((size_t)std::max<int64_t>(vo, 1)));
    DP_HIP(c, c->clean.htris.resize((size_t)std::max<int64_t>(3 * to, 1)));
    run.a.vout = c->clean.verts.p;
    run.a.vcap = vo;
    run.a.tout = c->clean.tris.p;
    run.a.tcap = to;
    run.a.vmap_out = vertex_map ? c->clean.maps.p : nullptr;
    run.a.tmap_out = triangle_map ? c->clean.maps.p + nv : nullptr;
    DP_HIP(c, c->clean.time[2].begin(s));
    if ((rc = clean_emit(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->clean.time[2].end(s));
    if (vo > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.hverts.data(), c->clean.verts.p, sizeof(dp_mesh_vertex) * (size_t)vo,
                                 hipMemcpyDeviceToHost, s));
    if (to > 0)
        DP_HIP(c, hipMemcpyAsync(c->clean.htris.data(), c->clean.tris.p, 12 * (size_t)to, hipMemcpyDeviceToHost, s));
    if (vertex_map && nv > 0)
        DP_HIP(c, hipMemcpyAsync(vertex_map, run.a.vmap_out, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
    if (triangle_map && nt > 0)
        DP_HIP(c, hipMemcpyAsync(triangle_map, run.a.tmap_out, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    if ((rc = clean_elapsed(c, 3, ms)) != DP_OK)
        return rc;
    const dp_mesh_clean_stats st = clean_stats(c, run, true, ms);
    *vertices_out = vo > 0 ? c->clean.hverts.data() : nullptr;
    *triangles_out = to > 0 ? c->clean.htris.data() : nullptr;
    *n_vertices_out = vo;
    *n_triangles_out = to;
    if (stats)
        *stats = st;
    return DP_OK;
}
