// dp_meshdecimate.hip -- gfx950 kernels of the mesh simplification by vertex
// clustering (spec in include/densepoints.h, dp_mesh_decimate) and its C ABI.
//
//   dec_mark_kernel      one lane per triangle: the guard, the classes, the USED
//                        stores (idempotent)
//   dec_keys_kernel      one lane per vertex: the cell of a used vertex as one key
//                        (k_z, k_y, k_x, 21 bits each, offset by 2^20), all ones
//                        for an unused vertex
//   (one stable hipcub radix sort of (key, vertex): a cluster is a run of equal
//   keys and its members come out in ascending index)
//   dec_vheads_kernel    the first key of every run is a cluster; clusters per block
//   (exclusive scan; its last word is K)
//   dec_number_kernel    the cluster of every used vertex, the first sorted
//                        position of every cluster (and, behind the last, the end)
//   dec_clusters_kernel  the largest member count
//   dec_tkeys_kernel     one lane per triangle: collapsed or not, the canonical
//                        triple as one key of 3 nb bits (nb = the bits of
//                        n_vertices, which bounds K), all ones when the triangle
//                        does not take part
//   (one stable sort of (key, triangle): the first of a run has the lowest index.
//   With 3 nb > 63 -- more than 2^21 vertices -- the triple does not fit one key:
//   two stable sorts, by the last two clusters and then by the first)
//   dec_theads_kernel    the first triangle of every run is kept and marks its
//                        three clusters as survivors; the others are duplicates
//   dec_scount / tcount  survivors and kept triangles per block (two scans)
//   dec_pairs_kernel     QUADRIC: the 1..3 distinct (cluster, triangle) pairs of
//                        every proper triangle (one stable sort by the cluster:
//                        every cluster's triangles ascending)
//   dec_walk_kernel      one lane per cluster: its output number, and for a
//                        survivor the walk over its members (fp64 sums of the
//                        positions, integer sums of the colours), in QUADRIC mode
//                        the walk over its triangles, the solve and the
//                        acceptance test; the 16-byte record
//   dec_temit / vmap     the kept triangles at the scanned offset plus the rank
//                        in the block, compared with the cap before the write;
//                        the maps
//
// One lane walks a whole cluster: the sums' order is part of the result, and a
// cluster of very many members is slow but correct.  Integer atomics only (the
// striped counters and one atomicMax); every index read from a triangle is
// compared with n_vertices before it is used as an address.
#include "dp_meshdev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

constexpr int kDecStripes = 64;
// invalid, degenerate triangles; used, clamped vertices; collapsed, duplicate
// triangles; quadric, mean placements
constexpr int kDecCounters = 8;
constexpr unsigned long long kPadKey = ~0ull;
constexpr uint32_t kPadCluster = ~0u;
constexpr int64_t kCellLo = -(1ll << 20), kCellHi = (1ll << 20) - 1;

struct DecArgs {
    const dp_mesh_vertex *verts;
    const int32_t *tris;
    int64_t nv, nt, n3; // n3 = 3 nt pairs
    int64_t nbv, nbt;
    double origin[3], cell;
    int quadric;
    int nb;   // the bits of n_vertices
    int wide; // 3 nb > 63: the triple is sorted in two passes
    uint8_t *used, *tkeep, *surv;
    unsigned long long *vkeys, *vkeys_sorted, *tkeys, *tkeys_sorted;
    unsigned long long *bcount, *boff; // three segments: clusters [nbv + 1], survivors [nbv + 1], kept triangles [nbt + 1]
    unsigned long long *count;
    int32_t *vidx, *vidx_sorted, *cid, *cstart, *cout, *maxval;
    int32_t *tin, *tmid, *tsorted; // the triangle numbers before the sort(s), between the two, after
    uint32_t *pkeys, *pkeys_sorted;
    int32_t *ptris, *ptris_sorted;
    // outputs, any may be null
    dp_mesh_vertex *vout;
    int64_t vcap;
    int32_t *tout;
    int64_t tcap;
    int32_t *vmap_out, *tmap_out;
};

__device__ __forceinline__ int64_t seg_clusters(const DecArgs &) { return 0; }
__device__ __forceinline__ int64_t seg_survivors(const DecArgs &a) { return a.nbv + 1; }
__device__ __forceinline__ int64_t seg_tris(const DecArgs &a) { return 2 * (a.nbv + 1); }

// K, valid once the clusters' scan has run
__device__ __forceinline__ int64_t cluster_count(const DecArgs &a) { return (int64_t)a.boff[seg_clusters(a) + a.nbv]; }

__device__ __forceinline__ void dec_count(const DecArgs &a, int counter, unsigned long long v)
{
    wave_count<kDecStripes, kDecCounters>(a.count, counter, v, blockIdx.x * (kMeshLanes / 64) + (threadIdx.x >> 6));
}

// the classes of triangle t: v holds its indices when it is valid
__device__ __forceinline__ void classify(const DecArgs &a, int64_t t, int32_t v[3], bool &valid, bool &proper)
{
    valid = load_valid_triangle(a.tris, a.nt, a.nv, t, v);
    proper = valid && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
}

// the clusters of a proper triangle's indices; false (and nothing else read) for any other t
__device__ __forceinline__ bool triangle_clusters(const DecArgs &a, int64_t t, int32_t A[3])
{
    int32_t v[3];
    bool valid, proper;
    classify(a, t, v, valid, proper);
    if (!proper)
        return false;
    // a proper triangle's vertices are used: their clusters are numbered
    A[0] = a.cid[v[0]];
    A[1] = a.cid[v[1]];
    A[2] = a.cid[v[2]];
    return true;
}

// the rotation of three distinct clusters that puts the smallest first
__device__ __forceinline__ void canonical(const int32_t A[3], unsigned long long &x, unsigned long long &y,
                                          unsigned long long &z)
{
    const int r = A[0] < A[1] ? (A[0] < A[2] ? 0 : 2) : (A[1] < A[2] ? 1 : 2);
    x = (unsigned long long)(uint32_t)A[r];
    y = (unsigned long long)(uint32_t)A[(r + 1) % 3];
    z = (unsigned long long)(uint32_t)A[(r + 2) % 3];
}

// one axis of the cell of a position; true when the bounds changed it
__device__ __forceinline__ bool cell_axis(double p, double origin, double cell, int64_t &k)
{
    const double q = floor(dpg::dvdiv(p - origin, cell));
    if (!(q >= -1048576.0)) {
        k = kCellLo;
        return true;
    }
    if (q > 1048575.0) {
        k = kCellHi;
        return true;
    }
    k = (int64_t)q;
    return false;
}

// the cell of (x, y, z) as a key ordered like (k_z, k_y, k_x): 63 bits
__device__ __forceinline__ unsigned long long cell_key(const DecArgs &a, float x, float y, float z, bool &clamped)
{
    int64_t kx, ky, kz;
    const bool cx = cell_axis((double)x, a.origin[0], a.cell, kx);
    const bool cy = cell_axis((double)y, a.origin[1], a.cell, ky);
    const bool cz = cell_axis((double)z, a.origin[2], a.cell, kz);
    clamped = cx || cy || cz;
    return (unsigned long long)(kz - kCellLo) << 42 | (unsigned long long)(ky - kCellLo) << 21 |
           (unsigned long long)(kx - kCellLo);
}

// a record is 16 bytes with 4-byte alignment: four words, pad included (one 128-bit load)
__device__ __forceinline__ void load_record(const dp_mesh_vertex *verts, int64_t v, uint32_t w[4])
{
    const uint32_t *src = (const uint32_t *)(verts + v);
    const uint32_t w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
    w[0] = w0;
    w[1] = w1;
    w[2] = w2;
    w[3] = w3;
}

__global__ __launch_bounds__(kMeshLanes) void dec_mark_kernel(DecArgs a)
{
    const int64_t t = mesh_item();
    int32_t v[3] = {0, 0, 0};
    bool valid, proper;
    classify(a, t, v, valid, proper);
    if (proper) {
        a.used[v[0]] = 1;
        a.used[v[1]] = 1;
        a.used[v[2]] = 1;
    }
    dec_count(a, 0, t < a.nt && !valid ? 1ull : 0ull);
    dec_count(a, 1, valid && !proper ? 1ull : 0ull);
}

__global__ __launch_bounds__(kMeshLanes) void dec_keys_kernel(DecArgs a)
{
    const int64_t v = mesh_item();
    bool used = false, clamped = false;
    if (v < a.nv) {
        used = a.used[v] != 0;
        unsigned long long key = kPadKey;
        if (used) {
            uint32_t w[4];
            load_record(a.verts, v, w);
            key = cell_key(a, __uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), clamped);
        }
        a.vkeys[v] = key;
        a.vidx[v] = (int32_t)v;
    }
    dec_count(a, 2, used ? 1ull : 0ull);
    dec_count(a, 3, clamped ? 1ull : 0ull);
}

__device__ __forceinline__ bool is_cluster_head(const DecArgs &a, int64_t i)
{
    if (i >= a.nv)
        return false;
    const unsigned long long k = a.vkeys_sorted[i];
    return k != kPadKey && (i == 0 || a.vkeys_sorted[i - 1] != k);
}

__global__ __launch_bounds__(kMeshLanes) void dec_vheads_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const uint32_t total = block_sum<kMeshLanes>(is_cluster_head(a, mesh_item()) ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_clusters(a) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshLanes) void dec_number_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const int64_t i = mesh_item();
    const bool head = is_cluster_head(a, i);
    // the heads at or before i, less one: the cluster of position i
    const int64_t c = (int64_t)a.boff[seg_clusters(a) + blockIdx.x] + block_exclusive(head ? 1u : 0u, wsum) + (head ? 1 : 0) - 1;
    if (i >= a.nv || a.vkeys_sorted[i] == kPadKey)
        return;
    // a key below the padding belongs to a used vertex: 0 <= c < K <= nv
    a.cid[a.vidx_sorted[i]] = (int32_t)c;
    if (head)
        a.cstart[c] = (int32_t)i;
    if (i + 1 == a.nv || a.vkeys_sorted[i + 1] == kPadKey)
        a.cstart[c + 1] = (int32_t)(i + 1); // the last used vertex: c + 1 = K <= nv, the end of the last run
}

__global__ __launch_bounds__(kMeshLanes) void dec_clusters_kernel(DecArgs a)
{
    const int64_t c = mesh_item();
    int32_t m = c < cluster_count(a) ? a.cstart[c + 1] - a.cstart[c] : 0;
    for (int o = 32; o > 0; o >>= 1)
        m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0)
        atomicMax(a.maxval, m);
}

__global__ __launch_bounds__(kMeshLanes) void dec_tkeys_kernel(DecArgs a)
{
    const int64_t t = mesh_item();
    int32_t A[3] = {0, 0, 0};
    const bool proper = triangle_clusters(a, t, A);
    const bool collapsed = proper && (A[0] == A[1] || A[1] == A[2] || A[0] == A[2]);
    if (t < a.nt) {
        unsigned long long key = kPadKey;
        if (proper && !collapsed) {
            // x, y, z < 2^nb: the key fits 3 nb <= 63 bits (2 nb <= 62 of them in the wide form), below the padding
            unsigned long long x, y, z;
            canonical(A, x, y, z);
            key = a.wide ? (y << a.nb | z) : (x << (2 * a.nb) | y << a.nb | z);
        }
        a.tkeys[t] = key;
        a.tin[t] = (int32_t)t;
    }
    dec_count(a, 4, collapsed ? 1ull : 0ull);
}

// the wide form's second key: the first cluster of the triangle at every position of the first sort
__global__ __launch_bounds__(kMeshLanes) void dec_thigh_kernel(DecArgs a)
{
    const int64_t i = mesh_item();
    if (i >= a.nt)
        return;
    unsigned long long key = kPadKey;
    if (a.tkeys_sorted[i] != kPadKey) {
        int32_t A[3];
        unsigned long long x, y, z;
        triangle_clusters(a, a.tmid[i], A); // a key below the padding: a proper triangle
        canonical(A, x, y, z);
        key = x;
    }
    a.tkeys[i] = key;
}

__global__ __launch_bounds__(kMeshLanes) void dec_theads_kernel(DecArgs a)
{
    const int64_t i = mesh_item();
    bool part = false, head = false;
    if (i < a.nt) {
        const unsigned long long key = a.tkeys_sorted[i];
        part = key != kPadKey;
        if (part) {
            // a key below the padding names a proper triangle: its indices are vertices, its clusters < K
            const int64_t t = a.tsorted[i];
            int32_t A[3];
            triangle_clusters(a, t, A);
            head = i == 0 || a.tkeys_sorted[i - 1] != key;
            if (!head && a.wide) {
                // equal first clusters: the run goes on only with the other two equal as well
                int32_t B[3];
                unsigned long long x, y, z, xp, yp, zp;
                triangle_clusters(a, a.tsorted[i - 1], B);
                canonical(A, x, y, z);
                canonical(B, xp, yp, zp);
                head = y != yp || z != zp;
            }
            if (head) {
                a.tkeep[t] = 1;
                a.surv[A[0]] = 1;
                a.surv[A[1]] = 1;
                a.surv[A[2]] = 1;
            }
        }
    }
    dec_count(a, 5, part && !head ? 1ull : 0ull);
}

__device__ __forceinline__ bool cluster_survives(const DecArgs &a, int64_t c)
{
    return c < cluster_count(a) && a.surv[c] != 0;
}

__global__ __launch_bounds__(kMeshLanes) void dec_scount_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const uint32_t total = block_sum<kMeshLanes>(cluster_survives(a, mesh_item()) ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_survivors(a) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshLanes) void dec_tcount_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const int64_t t = mesh_item();
    const uint32_t total = block_sum<kMeshLanes>(t < a.nt && a.tkeep[t] != 0 ? 1u : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[seg_tris(a) + blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshLanes) void dec_pairs_kernel(DecArgs a)
{
    const int64_t t = mesh_item();
    int32_t A[3] = {0, 0, 0};
    const bool proper = triangle_clusters(a, t, A);
    if (t >= a.nt)
        return;
    // once per cluster: an entry that repeats an earlier one is padding (3 t + 2 < n3)
    const bool first[3] = {proper, proper && A[1] != A[0], proper && A[2] != A[0] && A[2] != A[1]};
    for (int e = 0; e < 3; ++e) {
        a.pkeys[3 * t + e] = first[e] ? (uint32_t)A[e] : kPadCluster;
        a.ptris[3 * t + e] = (int32_t)t;
    }
}

// the first pair of the sorted pairs whose cluster is >= c
__device__ __forceinline__ int64_t first_pair(const DecArgs &a, uint32_t c)
{
    int64_t lo = 0, hi = a.n3;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.pkeys_sorted[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the quadric's offset from the mean m of cluster c; false when the cluster is not solvable
__device__ __forceinline__ bool quadric_offset(const DecArgs &a, int64_t c, const double m[3], double x[3])
{
    // c + 1 <= K <= nv <= 2^31 - 1, below the padding
    const int64_t lo = first_pair(a, (uint32_t)c), hi = first_pair(a, (uint32_t)c + 1u);
    double Axx = 0.0, Axy = 0.0, Axz = 0.0, Ayy = 0.0, Ayz = 0.0, Azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    for (int64_t e = lo; e < hi; ++e) {
        // a pair with a cluster below the padding names a proper triangle: t < nt, its indices < nv
        const int32_t *tri = a.tris + 3 * (int64_t)a.ptris_sorted[e];
        uint32_t w0[4], w1[4], w2[4];
        load_record(a.verts, tri[0], w0);
        load_record(a.verts, tri[1], w1);
        load_record(a.verts, tri[2], w2);
        const double p0x = (double)__uint_as_float(w0[0]), p0y = (double)__uint_as_float(w0[1]),
                     p0z = (double)__uint_as_float(w0[2]);
        const double e1x = (double)__uint_as_float(w1[0]) - p0x, e1y = (double)__uint_as_float(w1[1]) - p0y,
                     e1z = (double)__uint_as_float(w1[2]) - p0z;
        const double e2x = (double)__uint_as_float(w2[0]) - p0x, e2y = (double)__uint_as_float(w2[1]) - p0y,
                     e2z = (double)__uint_as_float(w2[2]) - p0z;
        const double gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
        const double rx = p0x - m[0], ry = p0y - m[1], rz = p0z - m[2];
        const double d = (gx * rx + gy * ry) + gz * rz;
        Axx = Axx + gx * gx;
        Axy = Axy + gx * gy;
        Axz = Axz + gx * gz;
        Ayy = Ayy + gy * gy;
        Ayz = Ayz + gy * gz;
        Azz = Azz + gz * gz;
        bx = bx + d * gx;
        by = by + d * gy;
        bz = bz + d * gz;
    }
    const double c00 = Ayy * Azz - Ayz * Ayz, c01 = Axz * Ayz - Axy * Azz, c02 = Axy * Ayz - Axz * Ayy;
    const double c11 = Axx * Azz - Axz * Axz, c12 = Axy * Axz - Axx * Ayz, c22 = Axx * Ayy - Axy * Axy;
    const double det = (Axx * c00 + Axy * c01) + Axz * c02;
    const double t = dpg::dvdiv((Axx + Ayy) + Azz, 3.0);
    // a NaN fails the first comparison
    if (!(fabs(det) <= 1.7976931348623157e308) || !(det > DP_DECIMATE_DET_EPS * ((t * t) * t)))
        return false;
    x[0] = dpg::dvdiv((c00 * bx + c01 * by) + c02 * bz, det);
    x[1] = dpg::dvdiv((c01 * bx + c11 * by) + c12 * bz, det);
    x[2] = dpg::dvdiv((c02 * bx + c12 * by) + c22 * bz, det);
    return true;
}

__device__ __forceinline__ bool finite_f32(float f) { return fabsf(f) <= 3.402823466e+38f; }

__global__ __launch_bounds__(kMeshLanes) void dec_walk_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const int64_t c = mesh_item();
    const bool alive = cluster_survives(a, c);
    const int64_t id = (int64_t)a.boff[seg_survivors(a) + blockIdx.x] + block_exclusive(alive ? 1u : 0u, wsum);
    bool placed = false;
    if (c < cluster_count(a))
        a.cout[c] = alive ? (int32_t)id : -1;
    if (alive) {
        const int32_t lo = a.cstart[c], hi = a.cstart[c + 1];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        unsigned long long r0 = 0, r1 = 0, r2 = 0;
        for (int32_t e = lo; e < hi; ++e) {
            uint32_t w[4];
            load_record(a.verts, a.vidx_sorted[e], w); // a member is a used vertex: < nv
            sx = sx + (double)__uint_as_float(w[0]);
            sy = sy + (double)__uint_as_float(w[1]);
            sz = sz + (double)__uint_as_float(w[2]);
            r0 += w[3] & 255u;
            r1 += (w[3] >> 8) & 255u;
            r2 += (w[3] >> 16) & 255u;
        }
        const unsigned long long n = (unsigned long long)(hi - lo); // a cluster has a member
        const double m[3] = {dpg::dvdiv(sx, (double)n), dpg::dvdiv(sy, (double)n), dpg::dvdiv(sz, (double)n)};
        float px = (float)m[0], py = (float)m[1], pz = (float)m[2];
        double x[3];
        if (a.quadric && quadric_offset(a, c, m, x)) {
            const float cx = (float)(m[0] + x[0]), cy = (float)(m[1] + x[1]), cz = (float)(m[2] + x[2]);
            bool clamped;
            // equal keys are equal cells, the bounds included
            if (finite_f32(cx) && finite_f32(cy) && finite_f32(cz) && cell_key(a, cx, cy, cz, clamped) == a.vkeys_sorted[lo]) {
                px = cx;
                py = cy;
                pz = cz;
                placed = true;
            }
        }
        if (id < a.vcap) {
            const uint32_t rgb = (uint32_t)((2 * r0 + n) / (2 * n)) | (uint32_t)((2 * r1 + n) / (2 * n)) << 8 |
                                 (uint32_t)((2 * r2 + n) / (2 * n)) << 16;
            uint32_t *dst = (uint32_t *)(a.vout + id);
            dst[0] = __float_as_uint(px);
            dst[1] = __float_as_uint(py);
            dst[2] = __float_as_uint(pz);
            dst[3] = rgb; // pad = 0
        }
    }
    dec_count(a, 6, placed ? 1ull : 0ull);
    dec_count(a, 7, alive && !placed ? 1ull : 0ull);
}

__global__ __launch_bounds__(kMeshLanes) void dec_temit_kernel(DecArgs a)
{
    __shared__ uint32_t wsum[kMeshLanes / 64];
    const int64_t t = mesh_item();
    const bool keep = t < a.nt && a.tkeep[t] != 0;
    const int64_t id = (int64_t)a.boff[seg_tris(a) + blockIdx.x] + block_exclusive(keep ? 1u : 0u, wsum);
    if (t >= a.nt)
        return;
    if (a.tmap_out)
        a.tmap_out[t] = keep ? (int32_t)id : -1;
    if (keep && id < a.tcap) {
        // a kept triangle is proper and its three clusters survive
        int32_t A[3];
        triangle_clusters(a, t, A);
        a.tout[3 * id] = a.cout[A[0]];
        a.tout[3 * id + 1] = a.cout[A[1]];
        a.tout[3 * id + 2] = a.cout[A[2]];
    }
}

__global__ __launch_bounds__(kMeshLanes) void dec_vmap_kernel(DecArgs a)
{
    const int64_t v = mesh_item();
    if (v < a.nv)
        a.vmap_out[v] = a.used[v] ? a.cout[a.cid[v]] : -1;
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mesh_decimate_options(dp_mesh_decimate_options *mdo)
{
    if (!mdo)
        return;
    *mdo = dp_mesh_decimate_options{};
    mdo->mode = DP_DECIMATE_MEAN;
}

namespace {

using dpk::DecArgs;
using dpk::kDecCounters;
using dpk::kDecStripes;
using dpk::mesh_blocks;

struct DecRun {
    DecArgs a{};
    size_t tmp_bytes = 0;
    int tri_end[2] = {1, 1}; // the end bits of the triangle sort(s)
    int pair_end = 1;
};

// the bits of n: the least nb with n < 2^nb
int bits_of(int64_t n)
{
    int nb = 0;
    while ((n >> nb) != 0)
        ++nb;
    return nb;
}

// everything but the pointers, in the header's order
int decimate_check(dp_ctx *c, const std::string &w, const dp_mesh_decimate_options *o, const void *verts, int64_t nv,
                   const void *tris, int64_t nt)
{
    if (nt >= 0 && nv >= 0 && 3 * nt > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": 3 * n_triangles must be <= 2^31 - 1");
    int rc = mesh_check_counts(c, w, tris, nt, nv);
    if (rc != DP_OK)
        return rc;
    if (nv > 0 && !verts)
        return fail(c, DP_E_ARG, w + ": vertices must be given");
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if (!(o->cell > 0.0f) || std::isinf(o->cell))
        return fail(c, DP_E_ARG, w + ": cell must be finite and > 0");
    if (!std::isfinite(o->origin[0]) || !std::isfinite(o->origin[1]) || !std::isfinite(o->origin[2]))
        return fail(c, DP_E_ARG, w + ": origin must be finite");
    if (o->mode != DP_DECIMATE_MEAN && o->mode != DP_DECIMATE_QUADRIC)
        return fail(c, DP_E_ARG, w + ": mode must be DP_DECIMATE_MEAN or DP_DECIMATE_QUADRIC");
    if (o->flags != 0)
        return fail(c, DP_E_ARG, w + ": unknown flag bits");
    return DP_OK;
}

// the scratch of a run and the sizes of the hipcub calls
int decimate_prepare(dp_ctx *c, const dp_mesh_decimate_options &o, const dp_mesh_vertex *d_verts, int64_t nv,
                     const int32_t *d_tris, int64_t nt, hipStream_t s, DecRun &run)
{
    DecArgs &a = run.a;
    dpk::MeshDecimateScratch &m = c->decimate;
    a.verts = d_verts;
    a.tris = d_tris;
    a.nv = nv;
    a.nt = nt;
    a.n3 = 3 * nt;
    a.nbv = mesh_blocks(nv);
    a.nbt = mesh_blocks(nt);
    for (int k = 0; k < 3; ++k)
        a.origin[k] = (double)o.origin[k];
    a.cell = (double)o.cell;
    a.quadric = o.mode == DP_DECIMATE_QUADRIC ? 1 : 0;
    a.nb = bits_of(nv);
    a.wide = 3 * a.nb > 63 ? 1 : 0;
    // the padding's bit above the key's: it sorts behind every key
    run.tri_end[0] = (a.wide ? 2 : 3) * a.nb + 1;
    run.tri_end[1] = a.nb + 1;
    run.pair_end = std::min(a.nb + 1, 32);
    const size_t n = (size_t)std::max<int64_t>(nv, 1), t = (size_t)std::max<int64_t>(nt, 1);
    const size_t nblk = (size_t)(2 * (a.nbv + 1) + a.nbt + 1);
    DP_HIP(c, m.used.reserve(n));
    DP_HIP(c, m.surv.reserve(n));
    DP_HIP(c, m.tkeep.reserve(t));
    DP_HIP(c, m.vkeys.reserve(n));
    DP_HIP(c, m.vkeys_sorted.reserve(n));
    DP_HIP(c, m.vidx.reserve(n));
    DP_HIP(c, m.vidx_sorted.reserve(n));
    DP_HIP(c, m.cid.reserve(n));
    DP_HIP(c, m.cstart.reserve(n + 1));
    DP_HIP(c, m.cout.reserve(n));
    DP_HIP(c, m.maxval.reserve(1));
    DP_HIP(c, m.tkeys.reserve(t));
    DP_HIP(c, m.tkeys_sorted.reserve(t));
    DP_HIP(c, m.tval[0].reserve(t));
    DP_HIP(c, m.tval[1].reserve(t));
    DP_HIP(c, m.bcount.reserve(nblk));
    DP_HIP(c, m.boff.reserve(nblk));
    DP_HIP(c, m.count.reserve(kDecStripes, kDecCounters, 4)); // + K, VO, TO, the largest cluster
    if (a.quadric) {
        const size_t n3 = (size_t)std::max<int64_t>(a.n3, 1);
        DP_HIP(c, m.pkeys.reserve(n3));
        DP_HIP(c, m.pkeys_sorted.reserve(n3));
        DP_HIP(c, m.ptris.reserve(n3));
        DP_HIP(c, m.ptris_sorted.reserve(n3));
    }
    a.used = m.used.p;
    a.surv = m.surv.p;
    a.tkeep = m.tkeep.p;
    a.vkeys = m.vkeys.p;
    a.vkeys_sorted = m.vkeys_sorted.p;
    a.vidx = m.vidx.p;
    a.vidx_sorted = m.vidx_sorted.p;
    a.cid = m.cid.p;
    a.cstart = m.cstart.p;
    a.cout = m.cout.p;
    a.maxval = m.maxval.p;
    a.tkeys = m.tkeys.p;
    a.tkeys_sorted = m.tkeys_sorted.p;
    a.tin = m.tval[0].p;
    a.tmid = m.tval[1].p;
    a.tsorted = a.wide ? m.tval[0].p : m.tval[1].p;
    a.bcount = m.bcount.p;
    a.boff = m.boff.p;
    a.count = m.count.dev.p;
    a.pkeys = m.pkeys.p;
    a.pkeys_sorted = m.pkeys_sorted.p;
    a.ptris = m.ptris.p;
    a.ptris_sorted = m.ptris_sorted.p;
    size_t b = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, a.bcount, a.boff, (int)std::max(a.nbv, a.nbt) + 1, s));
    run.tmp_bytes = b;
    if (nv > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.vkeys, a.vkeys_sorted, a.vidx, a.vidx_sorted, (int)nv, 0,
                                                     64, s));
        run.tmp_bytes = std::max(run.tmp_bytes, b);
    }
    if (nt > 0) {
        for (int pass = 0; pass <= a.wide; ++pass) {
            DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.tkeys, a.tkeys_sorted, a.tin, a.tmid, (int)nt, 0,
                                                         run.tri_end[pass], s));
            run.tmp_bytes = std::max(run.tmp_bytes, b);
        }
        if (a.quadric) {
            DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.pkeys, a.pkeys_sorted, a.ptris, a.ptris_sorted,
                                                         (int)a.n3, 0, run.pair_end, s));
            run.tmp_bytes = std::max(run.tmp_bytes, b);
        }
    }
    DP_HIP(c, c->scan_tmp.reserve(run.tmp_bytes ? run.tmp_bytes : 1));
    return DP_OK;
}

int decimate_scan(dp_ctx *c, const DecRun &run, int64_t seg, int64_t blocks, hipStream_t s)
{
    size_t b = run.tmp_bytes;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, run.a.bcount + seg, run.a.boff + seg, (int)blocks + 1, s));
    return DP_OK;
}

// queues the whole simplification, the counters zeroed first
int decimate_build(dp_ctx *c, DecRun &run, hipStream_t s)
{
    const DecArgs &a = run.a;
    const int64_t sc = 0, ss = a.nbv + 1, st = 2 * (a.nbv + 1);
    int rc;
    size_t b;
    DP_HIP(c, c->decimate.count.zero(s));
    DP_HIP(c, hipMemsetAsync(a.maxval, 0, sizeof(int32_t), s));
    if (a.nv > 0) {
        DP_HIP(c, hipMemsetAsync(a.used, 0, (size_t)a.nv, s));
        DP_HIP(c, hipMemsetAsync(a.surv, 0, (size_t)a.nv, s));
    }
    if (a.nt > 0)
        DP_HIP(c, hipMemsetAsync(a.tkeep, 0, (size_t)a.nt, s));
    // the word behind every segment's counts: the scan leaves the total there
    DP_HIP(c, hipMemsetAsync(a.bcount + sc + a.nbv, 0, sizeof(unsigned long long), s));
    DP_HIP(c, hipMemsetAsync(a.bcount + ss + a.nbv, 0, sizeof(unsigned long long), s));
    DP_HIP(c, hipMemsetAsync(a.bcount + st + a.nbt, 0, sizeof(unsigned long long), s));
    // the clusters
    DP_HIP(c, dpk::launch_over(dpk::dec_mark_kernel, a.nbt, a, s));
    DP_HIP(c, dpk::launch_over(dpk::dec_keys_kernel, a.nbv, a, s));
    if (a.nv > 0) {
        b = run.tmp_bytes;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.vkeys, a.vkeys_sorted, a.vidx, a.vidx_sorted,
                                                     (int)a.nv, 0, 64, s));
    }
    DP_HIP(c, dpk::launch_over(dpk::dec_vheads_kernel, a.nbv, a, s));
    if ((rc = decimate_scan(c, run, sc, a.nbv, s)) != DP_OK)
        return rc;
    DP_HIP(c, dpk::launch_over(dpk::dec_number_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::dec_clusters_kernel, a.nbv, a, s));
    // the triangles
    DP_HIP(c, dpk::launch_over(dpk::dec_tkeys_kernel, a.nbt, a, s));
    if (a.nt > 0) {
        b = run.tmp_bytes;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.tkeys, a.tkeys_sorted, a.tin, a.tmid, (int)a.nt, 0,
                                                     run.tri_end[0], s));
        if (a.wide) {
            DP_HIP(c, dpk::launch_over(dpk::dec_thigh_kernel, a.nbt, a, s));
            b = run.tmp_bytes;
            DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.tkeys, a.tkeys_sorted, a.tmid, a.tsorted,
                                                         (int)a.nt, 0, run.tri_end[1], s));
        }
    }
    DP_HIP(c, dpk::launch_over(dpk::dec_theads_kernel, a.nbt, a, s));
    DP_HIP(c, dpk::launch_over(dpk::dec_scount_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::dec_tcount_kernel, a.nbt, a, s));
    if ((rc = decimate_scan(c, run, ss, a.nbv, s)) != DP_OK || (rc = decimate_scan(c, run, st, a.nbt, s)) != DP_OK)
        return rc;
    // the output
    if (a.quadric && a.nt > 0) {
        DP_HIP(c, dpk::launch_over(dpk::dec_pairs_kernel, a.nbt, a, s));
        b = run.tmp_bytes;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.pkeys, a.pkeys_sorted, a.ptris, a.ptris_sorted,
                                                     (int)a.n3, 0, run.pair_end, s));
    }
    DP_HIP(c, dpk::launch_over(dpk::dec_walk_kernel, a.nbv, a, s));
    DP_HIP(c, dpk::launch_over(dpk::dec_temit_kernel, a.nbt, a, s));
    if (a.vmap_out)
        DP_HIP(c, dpk::launch_over(dpk::dec_vmap_kernel, a.nbv, a, s));
    return DP_OK;
}

// queues the copies of the counters and, behind them, K, the output totals and the largest cluster
int decimate_read(dp_ctx *c, const DecRun &run, hipStream_t s)
{
    const DecArgs &a = run.a;
    unsigned long long *h = c->decimate.count.extra();
    h[0] = h[1] = h[2] = h[3] = 0;
    DP_HIP(c, c->decimate.count.read(s));
    DP_HIP(c, hipMemcpyAsync(h, a.boff + a.nbv, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + 1, a.boff + (a.nbv + 1) + a.nbv, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + 2, a.boff + 2 * (a.nbv + 1) + a.nbt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + 3, a.maxval, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return DP_OK;
}

dp_mesh_decimate_stats decimate_stats(dp_ctx *c, const DecRun &run, double ms)
{
    const dpk::StripedCounters &k = c->decimate.count;
    const unsigned long long *h = c->decimate.count.extra();
    dp_mesh_decimate_stats r{};
    r.vertices_in = run.a.nv;
    r.triangles_in = run.a.nt;
    r.invalid_triangles = k.sum(0);
    r.degenerate_triangles = k.sum(1);
    r.unused_vertices = run.a.nv - k.sum(2);
    r.clamped_vertices = k.sum(3);
    r.clusters = (int64_t)h[0];
    r.vertices_out = (int64_t)h[1];
    r.triangles_out = (int64_t)h[2];
    r.orphan_clusters = r.clusters - r.vertices_out;
    r.max_cluster = (int64_t)(int32_t)(uint32_t)h[3];
    r.collapsed_triangles = k.sum(4);
    r.duplicate_triangles = k.sum(5);
    r.quadric_vertices = k.sum(6);
    r.mean_vertices = k.sum(7);
    r.decimate_ms = ms;
    return r;
}

// prepare, queue, read and the one wait; the outputs of run.a are the caller's to set before
int decimate_run(dp_ctx *c, DecRun &run, hipStream_t s, dp_mesh_decimate_stats &st)
{
    int rc;
    DP_HIP(c, c->decimate.time.begin(s));
    if ((rc = decimate_build(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->decimate.time.end(s));
    // the one wait: the counts and statistics
    if ((rc = decimate_read(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, hipStreamSynchronize(s));
    double ms = 0.0;
    DP_HIP(c, c->decimate.time.ms(ms));
    st = decimate_stats(c, run, ms);
    return DP_OK;
}

} // namespace

extern "C" int dp_mesh_decimate_device(dp_ctx *c, const dp_mesh_decimate_options *opts, const dp_mesh_vertex *d_vertices,
                                       int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                                       dp_mesh_vertex *d_vertices_out, int64_t vertex_cap, int64_t *n_vertices_out,
                                       int32_t *d_triangles_out, int64_t triangle_cap, int64_t *n_triangles_out,
                                       int32_t *d_vertex_map, int32_t *d_triangle_map, dp_mesh_decimate_stats *stats,
                                       void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_decimate_device";
    int rc = decimate_check(c, w, opts, d_vertices, n_vertices, d_triangles, n_triangles);
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
    DecRun run;
    if ((rc = decimate_prepare(c, *opts, d_vertices, n_vertices, d_triangles, n_triangles, s, run)) != DP_OK)
        return rc;
    run.a.vout = d_vertices_out;
    run.a.vcap = vertex_cap;
    run.a.tout = d_triangles_out;
    run.a.tcap = triangle_cap;
    run.a.vmap_out = d_vertex_map;
    run.a.tmap_out = d_triangle_map;
    dp_mesh_decimate_stats st;
    if ((rc = decimate_run(c, run, s, st)) != DP_OK)
        return rc;
    *n_vertices_out = st.vertices_out;
    *n_triangles_out = st.triangles_out;
    if (stats)
        *stats = st;
    return DP_OK;
}

extern "C" int dp_mesh_decimate(dp_ctx *c, const dp_mesh_decimate_options *opts, const dp_mesh_vertex *vertices,
                                int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                                const dp_mesh_vertex **vertices_out, int64_t *n_vertices_out,
                                const int32_t **triangles_out, int64_t *n_triangles_out, int32_t *vertex_map,
                                int32_t *triangle_map, dp_mesh_decimate_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_decimate";
    int rc = decimate_check(c, w, opts, vertices, n_vertices, triangles, n_triangles);
    if (rc == DP_OK && (!n_vertices_out || !n_triangles_out || !vertices_out || !triangles_out))
        rc = fail(c, DP_E_ARG, w + ": the result and count pointers must be given");
    if (rc == DP_OK)
        rc = mesh_check_alias(c, w, {vertex_map, triangle_map}, {vertices, triangles});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const int64_t nt = n_triangles, nv = n_vertices;
    dpk::MeshDecimateScratch &m = c->decimate;
    // staged inputs: the vertices (16 B each), then the triangles; the output is
    // no larger than the input, so the input's counts size the device results
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    DP_HIP(c, m.in.reserve(std::max<size_t>(vbytes + 12 * (size_t)nt, 1)));
    DP_HIP(c, m.maps.reserve((size_t)std::max<int64_t>(nv + nt, 1)));
    DP_HIP(c, m.verts.reserve((size_t)std::max<int64_t>(nv, 1)));
    DP_HIP(c, m.tris.reserve((size_t)std::max<int64_t>(3 * nt, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(m.in.p, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(m.in.p + vbytes, triangles, 12 * (size_t)nt, hipMemcpyHostToDevice, s));
    DecRun run;
    if ((rc = decimate_prepare(c, *opts, (const dp_mesh_vertex *)m.in.p, nv, (const int32_t *)(m.in.p + vbytes), nt, s,
                               run)) != DP_OK)
        return rc;
    run.a.vout = m.verts.p;
    run.a.vcap = nv;
    run.a.tout = m.tris.p;
    run.a.tcap = nt;
    run.a.vmap_out = vertex_map ? m.maps.p : nullptr;
    run.a.tmap_out = triangle_map ? m.maps.p + nv : nullptr;
    dp_mesh_decimate_stats st;
    if ((rc = decimate_run(c, run, s, st)) != DP_OK)
        return rc;
    const int64_t vo = st.vertices_out, to = st.triangles_out;
    if (vo > nv || to > nt)
        return fail(c, DP_E_STATE, w + ": the result is larger than the input");
    DP_HIP(c, m.hverts.resize((size_t)std::max<int64_t>(vo, 1)));
    DP_HIP(c, m.htris.resize((size_t)std::max<int64_t>(3 * to, 1)));
    if (vo > 0)
        DP_HIP(c, hipMemcpyAsync(m.hverts.data(), m.verts.p, sizeof(dp_mesh_vertex) * (size_t)vo, hipMemcpyDeviceToHost, s));
    if (to > 0)
        DP_HIP(c, hipMemcpyAsync(m.htris.data(), m.tris.p, 12 * (size_t)to, hipMemcpyDeviceToHost, s));
    if (vertex_map && nv > 0)
        DP_HIP(c, hipMemcpyAsync(vertex_map, run.a.vmap_out, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
    if (triangle_map && nt > 0)
        DP_HIP(c, hipMemcpyAsync(triangle_map, run.a.tmap_out, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    *vertices_out = vo > 0 ? m.hverts.data() : nullptr;
    *triangles_out = to > 0 ? m.htris.data() : nullptr;
    *n_vertices_out = vo;
    *n_triangles_out = to;
    if (stats)
        *stats = st;
    return DP_OK;
}
