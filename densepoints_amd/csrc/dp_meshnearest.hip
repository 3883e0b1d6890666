// dp_meshnearest.hip -- the gfx950 kernels of the nearest-triangle search from
// points to a mesh (spec in include/densepoints.h, dp_mesh_nearest) and its C
// ABI: a uniform grid over the box of the triangles taking part, every triangle
// registered in every cell its own box overlaps, every query walking the 3 x 3 x
// 3 cells around its own.
//
//   meshnear_box_kernel     the bounding box of the triangles taking part and
//                           their classes: a fixed number of blocks stride over
//                           the triangles, one box per block
//   meshnear_plan_kernel    one block: the boxes' box, the side of level 0 and
//                           the first level whose cells fit the cap
//   meshnear_levels_kernel  one lane per triangle: how many cells its box
//                           overlaps at every level from the first, until it is
//                           one cell (from there on it stays one); one integer
//                           atomic per wave and level on a small table
//   meshnear_pick_kernel    one lane: the lowest level whose registrations fit
//                           the bound, and its grid
//   meshnear_register_kernel<false>  one lane per triangle: +1 on every cell it
//                           overlaps
//   (one hipcub exclusive scan of the cells' counts: the cells' first entries)
//   meshnear_register_kernel<true>   one lane per triangle: its registrations,
//                           each with three bits saying whether the cell is the
//                           triangle's first on x, y and z.  The order inside a
//                           cell is the atomics': the minimum with its tie to the
//                           lowest index does not depend on it.
//   meshnear_maxcell_kernel the fullest cell and the number of registrations
//   meshnear_qkeys_kernel   one lane per query: the key of the cell nearest to it
//   (one stable hipcub radix sort of (key, query): neighbouring lanes walk the
//   same cells)
//   meshnear_query_kernel   one lane per cell-sorted query; the results are
//                           scattered to the queries' own positions
//
// The grid.  Level L has cubic cells of side side0 * 2^L, side0 = max_dist * (1 +
// 2^-19), from one origin (the box's low corner), n_k = floor(ext_k / side) + 1
// cells on axis k.  A coordinate x of axis k lies in cell floor(u), u = ((double)x
// - origin_k) / side: both operations are monotonic in x, so a triangle whose
// coordinates span [lo_k, hi_k] is registered in the cells C(lo_k) .. C(hi_k) of
// every axis, and a coordinate between lo_k and hi_k has its cell among them.
// Since 2^L scales u exactly, the cells of level L + 1 are pairs of level L's
// (floor(u / 2) = floor(floor(u) / 2)): a triangle's cell count never grows with
// the level, and one that is down to one cell stays there.
//
// Bounded tables.  The cap on cells is that of the cloud search (a power of two,
// 2 * n_triangles within 2^16 .. 2^24, known to the host); registrations are
// bounded by E = min(8 * n_triangles, 2^31 - 1), known to the host too.  The level
// taken is the lowest one from level_min whose exact registration count, summed
// by meshnear_levels_kernel, is at most E.  It exists: once the side reaches the
// largest triangle box every triangle overlaps at most 2 cells per axis, and at
// the last level there is one cell and one registration per triangle.  A coarser
// level is always correct, only slower.
//
// Why the margin suffices (for every candidate T of q some registered cell of T
// lies within +-1 of q's cell on every axis).  Take one axis.  If lo <= q <= hi,
// q's own cell is registered (monotonic).  Otherwise say q < lo; the box test of
// the spec passed, fl(lo - G) <= q, G = R * (1 + 2^-20).  q and lo are distinct
// floats, so lo - q >= 2^-24 * M, M = max(|lo|, |q|), while the rounding of lo - G
// is at most 2^-53 * (M + G): the test can pass only with M < 2^25 * G, and then
// the rounding is below 2^-28 * G, so the true lo - q <= G * (1 + 2^-28).
// With side >= R * (1 + 2^-19) * (1 - 2^-53) the true u of lo and q differ by at
// most (1 + 2^-20)(1 + 2^-28) / ((1 + 2^-19)(1 - 2^-53)) < 1 - 2^-21.  The computed
// u is the true one times (1 + e), |e| < 2^-52 (two roundings), and near the box
// |u| <= 2^24 + 2 (an axis has at most 2^24 cells, and q is within a cell of the
// box), so the computed u differ by less than 1 - 2^-21 + 2^-26 < 1 and their
// floors by at most 1: the registered cell C(lo) is in the walk.  q > hi is the
// mirror image with C(hi).  The three axes are independent and the registered
// cells are a box, so the cell made of the three choices is registered and walked.
// The clamp of a query's u to [-2, n + 1], done in fp64 before any conversion to
// an integer, is monotonic and leaves the registered range [0, n - 1] alone.
// The grid only bounds the walk: the spec's box test and d2 <= R2 decide.
//
// One evaluation per pair.  The walked cells [w0, w1] and the registered cells
// [t0, t1] of an axis overlap in [max(t0, w0), ...]; a registration is evaluated
// only from the cell that is, on every axis, max(t0, w0), i.e. the cell is the
// walk's first or the triangle's first there (the bit the fill kernel stored).
#include "dp_meshdev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

// triangles taking part, invalid, degenerate, non-finite; queries taking part, matched, unmatched
constexpr int kMeshNearCounters = 8;
constexpr int kMeshNearStripes = 64;
constexpr int kMeshNearBoxBlocks = 1024; // meshnear_box_kernel's blocks, at most
constexpr int kMeshNearCapMinBits = 16, kMeshNearCapMaxBits = 24;
// levels: a side of 2^-149 doubled 280 times exceeds any extent of floats
constexpr int kMeshNearLevels = 320;

struct MeshNearArgs {
    const char *queries;
    const dp_mesh_vertex *verts;
    const int32_t *tris;
    int64_t nq, qstride, nv, nt;
    int64_t entry_cap; // E, the entries' and the first bits' size
    int32_t cap, nboxes;
    int32_t bins, pad;
    double R, R2, G;
    float *boxes;
    MeshNearGrid *grid;
    unsigned long long *levels; // [kMeshNearLevels] cells of triangles above one cell, then [kMeshNearLevels] arrivals at one cell
    int32_t *cellcount, *begin, *entries;
    uint8_t *first;
    uint32_t *qkeys, *qkeys_sorted;
    int32_t *qidx, *qidx_sorted;
    int32_t *index;
    float *dist, *closest; // closest optional
    unsigned long long *hist; // optional
    unsigned long long *count; // kMeshNearStripes x kMeshNearCounters
};

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }

__device__ __forceinline__ uint32_t wave_stripe() { return blockIdx.x * (kMeshLanes / 64) + (threadIdx.x >> 6); }

// the class of triangle t: 0 takes part (p holds a, b, c), 1 invalid, 2 degenerate, 3 non-finite
__device__ __forceinline__ int load_triangle(const MeshNearArgs &a, int64_t t, float p[9])
{
    int32_t v[3];
    if (!load_valid_triangle(a.tris, a.nt, a.nv, t, v))
        return 1;
    if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2])
        return 2;
    bool fin = true;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            p[3 * i + k] = a.verts[v[i]].pos[k];
            fin = fin && finite_f32(p[3 * i + k]);
        }
    return fin ? 0 : 3;
}

__device__ __forceinline__ void triangle_box(const float p[9], float lo[3], float hi[3])
{
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(fminf(p[k], p[3 + k]), p[6 + k]);
        hi[k] = fmaxf(fmaxf(p[k], p[3 + k]), p[6 + k]);
    }
}

// the cells of an axis of `ext` at cells of `side`
__device__ __forceinline__ double axis_cells(double ext, double side) { return floor(dpg::dvdiv(ext, side)) + 1.0; }

// the cell coordinate of x, clamped to [lo, n + hi] in fp64 first: a coordinate
// of 1e30 must not reach the conversion
__device__ __forceinline__ int32_t cell_coord(double origin, double side, int32_t n, float x, double lo, double hi)
{
    double u = dpg::dvdiv((double)x - origin, side);
    u = fmin(fmax(u, lo), (double)n + hi);
    return (int32_t)floor(u);
}

// the cells [c0, c1] that the box [lo, hi] overlaps on every axis
__device__ __forceinline__ void box_cells(const double origin[3], double side, const int32_t n[3], const float lo[3],
                                          const float hi[3], int32_t c0[3], int32_t c1[3])
{
    for (int k = 0; k < 3; ++k) {
        c0[k] = cell_coord(origin[k], side, n[k], lo[k], 0.0, -1.0);
        c1[k] = max(c0[k], cell_coord(origin[k], side, n[k], hi[k], 0.0, -1.0));
    }
}

__device__ __forceinline__ void reduce_box(float lo[3], float hi[3], float (*part)[6])
{
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) {
            part[threadIdx.x >> 6][k] = lo[k];
            part[threadIdx.x >> 6][3 + k] = hi[k];
        }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kMeshLanes / 64; ++w)
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], part[w][k]);
                hi[k] = fmaxf(hi[k], part[w][3 + k]);
            }
}

__global__ __launch_bounds__(kMeshLanes) void meshnear_box_kernel(MeshNearArgs a)
{
    __shared__ float part[kMeshLanes / 64][6];
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    unsigned long long cls[4] = {0, 0, 0, 0};
    for (int64_t t = mesh_item(); t < a.nt; t += (int64_t)gridDim.x * kMeshLanes) {
        float p[9];
        const int c = load_triangle(a, t, p);
        for (int i = 0; i < 4; ++i)
            cls[i] += c == i ? 1ull : 0ull;
        if (c == 0) {
            float l[3], h[3];
            triangle_box(p, l, h);
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], l[k]);
                hi[k] = fmaxf(hi[k], h[k]);
            }
        }
    }
    reduce_box(lo, hi, part);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) {
            a.boxes[6 * blockIdx.x + k] = lo[k];
            a.boxes[6 * blockIdx.x + 3 + k] = hi[k];
        }
    const uint32_t stripe = wave_stripe();
    for (int i = 0; i < 4; ++i)
        wave_count<kMeshNearStripes, kMeshNearCounters>(a.count, i, cls[i], stripe);
}

// one block: the box of the boxes, level 0's side, the first level that fits the cap
__global__ __launch_bounds__(kMeshLanes) void meshnear_plan_kernel(MeshNearArgs a)
{
    __shared__ float part[kMeshLanes / 64][6];
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int b = threadIdx.x; b < a.nboxes; b += kMeshLanes)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], a.boxes[6 * b + k]);
            hi[k] = fmaxf(hi[k], a.boxes[6 * b + 3 + k]);
        }
    reduce_box(lo, hi, part);
    if (threadIdx.x != 0)
        return;
    MeshNearGrid g{};
    const bool none = !(lo[0] <= hi[0]); // no triangle takes part: one cell that nothing is registered in
    for (int k = 0; k < 3; ++k) {
        g.origin[k] = none ? 0.0 : (double)lo[k];
        g.ext[k] = none ? 0.0 : (double)hi[k] - (double)lo[k];
    }
    g.side0 = a.R * (1.0 + 0x1p-19);
    int L = 0;
    for (; L < kMeshNearLevels - 1; ++L) {
        const double side = ldexp(g.side0, L);
        if (axis_cells(g.ext[0], side) * axis_cells(g.ext[1], side) * axis_cells(g.ext[2], side) <= (double)a.cap)
            break;
    }
    g.level_min = L;
    *a.grid = g;
}

// The waves walk the levels in step: a lane leaves once its triangle is one cell.
__global__ __launch_bounds__(kMeshLanes) void meshnear_levels_kernel(MeshNearArgs a)
{
    const int64_t t = mesh_item();
    const MeshNearGrid &g = *a.grid;
    float p[9], lo[3], hi[3];
    bool act = t < a.nt && load_triangle(a, t, p) == 0;
    if (act)
        triangle_box(p, lo, hi);
    for (int L = g.level_min; L < kMeshNearLevels && __ballot(act) != 0; ++L) {
        const double side = ldexp(g.side0, L);
        unsigned long long c = 0, one = 0;
        if (act) {
            int32_t n[3], c0[3], c1[3];
            for (int k = 0; k < 3; ++k)
                n[k] = (int32_t)axis_cells(g.ext[k], side);
            box_cells(g.origin, side, n, lo, hi, c0, c1);
            // at most the level's cells, which fit the cap
            c = (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) *
                (unsigned long long)(c1[2] - c0[2] + 1);
            if (c == 1) {
                c = 0;
                one = 1;
                act = false;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o);
            one += __shfl_xor(one, o);
        }
        if ((threadIdx.x & 63) == 0) {
            if (c)
                atomicAdd(&a.levels[L], c);
            if (one)
                atomicAdd(&a.levels[kMeshNearLevels + L], one);
        }
    }
}

__global__ void meshnear_pick_kernel(MeshNearArgs a)
{
    MeshNearGrid g = *a.grid;
    unsigned long long ones = 0;
    int L = g.level_min;
    for (; L < kMeshNearLevels - 1; ++L) {
        ones += a.levels[kMeshNearLevels + L];
        if (a.levels[L] + ones <= (unsigned long long)a.entry_cap)
            break;
    }
    g.level = L;
    g.side = ldexp(g.side0, L);
    for (int k = 0; k < 3; ++k)
        g.n[k] = (int32_t)axis_cells(g.ext[k], g.side);
    g.cells = (int64_t)g.n[0] * g.n[1] * g.n[2];
    g.maxcell = 0;
    g.entries = 0;
    *a.grid = g;
}

template <bool Fill> __global__ __launch_bounds__(kMeshLanes) void meshnear_register_kernel(MeshNearArgs a)
{
    const int64_t t = mesh_item();
    float p[9], lo[3], hi[3];
    if (t >= a.nt || load_triangle(a, t, p) != 0)
        return;
    const MeshNearGrid &g = *a.grid;
    triangle_box(p, lo, hi);
    int32_t c0[3], c1[3];
    box_cells(g.origin, g.side, g.n, lo, hi, c0, c1);
    for (int32_t z = c0[2]; z <= c1[2]; ++z)
        for (int32_t y = c0[1]; y <= c1[1]; ++y)
            for (int32_t x = c0[0]; x <= c1[0]; ++x) {
                const int32_t key = (z * g.n[1] + y) * g.n[0] + x;
                if (!Fill) {
                    atomicAdd(&a.cellcount[key], 1);
                } else {
                    // the count runs back to 0: the cell's slots are handed out from its last
                    const int64_t at = (int64_t)a.begin[key] + (atomicSub(&a.cellcount[key], 1) - 1);
                    if (at >= 0 && at < a.entry_cap) {
                        a.entries[at] = (int32_t)t;
                        a.first[at] = (uint8_t)((x == c0[0] ? 1 : 0) | (y == c0[1] ? 2 : 0) | (z == c0[2] ? 4 : 0));
                    }
                }
            }
}

__global__ __launch_bounds__(kMeshLanes) void meshnear_maxcell_kernel(MeshNearArgs a)
{
    const int64_t k = mesh_item();
    int32_t v = k < a.cap ? a.begin[k + 1] - a.begin[k] : 0;
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0 && v)
        atomicMax(&a.grid->maxcell, v);
    if (k == 0)
        a.grid->entries = a.begin[a.cap];
}

// point i of the queries; false unless its three floats are finite
__device__ __forceinline__ bool load_query(const MeshNearArgs &a, int64_t i, float p[3])
{
    const float *f = (const float *)(a.queries + i * a.qstride);
    p[0] = f[0];
    p[1] = f[1];
    p[2] = f[2];
    return finite_f32(p[0]) && finite_f32(p[1]) && finite_f32(p[2]);
}

__global__ __launch_bounds__(kMeshLanes) void meshnear_qkeys_kernel(MeshNearArgs a)
{
    const int64_t i = mesh_item();
    if (i >= a.nq)
        return;
    const MeshNearGrid &g = *a.grid;
    float p[3];
    uint32_t key = (uint32_t)a.cap;
    if (load_query(a, i, p)) {
        const int32_t x = cell_coord(g.origin[0], g.side, g.n[0], p[0], 0.0, -1.0),
                      y = cell_coord(g.origin[1], g.side, g.n[1], p[1], 0.0, -1.0),
                      z = cell_coord(g.origin[2], g.side, g.n[2], p[2], 0.0, -1.0);
        key = (uint32_t)((z * g.n[1] + y) * g.n[0] + x);
    }
    a.qkeys[i] = key;
    a.qidx[i] = (int32_t)i;
}

__device__ __forceinline__ double dot3(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ void cross3(const double u[3], const double v[3], double w[3])
{
    w[0] = u[1] * v[2] - u[2] * v[1];
    w[1] = u[2] * v[0] - u[0] * v[2];
    w[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ void sub3(const double u[3], const double v[3], double w[3])
{
    for (int k = 0; k < 3; ++k)
        w[k] = u[k] - v[k];
}

// the segment from s along se, sp = q - s: replaces (d2, pt) when strictly nearer
__device__ __forceinline__ void segment_near(const double s[3], const double se[3], const double sp[3], double &d2, float pt[3])
{
    const double den = dot3(se, se);
    double t = den > 0.0 ? dpg::dvdiv(dot3(sp, se), den) : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    double r[3];
    for (int k = 0; k < 3; ++k)
        r[k] = sp[k] - t * se[k];
    const double e2 = dot3(r, r);
    if (e2 < d2) {
        d2 = e2;
        for (int k = 0; k < 3; ++k)
            pt[k] = (float)(s[k] + t * se[k]);
    }
}

// the spec's distance of q to (a, b, c): d2 and the point
__device__ __forceinline__ void triangle_near(const double q[3], const float p[9], double &d2, float pt[3])
{
    double a[3], b[3], c[3], ab[3], ac[3], bc[3], ca[3], ap[3], bp[3], cp[3], n[3], w[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)p[k];
        b[k] = (double)p[3 + k];
        c[k] = (double)p[6 + k];
    }
    sub3(b, a, ab);
    sub3(c, a, ac);
    sub3(c, b, bc);
    sub3(a, c, ca);
    sub3(q, a, ap);
    sub3(q, b, bp);
    sub3(q, c, cp);
    d2 = __builtin_huge_val();
    pt[0] = pt[1] = pt[2] = __builtin_huge_valf();
    cross3(ab, ac, n);
    const double nn = dot3(n, n);
    if (nn > (dot3(ab, ab) * dot3(ac, ac)) * 0x1p-40) {
        cross3(ab, ap, w);
        bool in = dot3(w, n) >= 0.0;
        cross3(bc, bp, w);
        in = in && dot3(w, n) >= 0.0;
        cross3(ca, cp, w);
        in = in && dot3(w, n) >= 0.0;
        if (in) {
            const double s = dpg::dvdiv(dot3(ap, n), nn);
            double r[3];
            for (int k = 0; k < 3; ++k)
                r[k] = s * n[k];
            d2 = dot3(r, r);
            for (int k = 0; k < 3; ++k)
                pt[k] = (float)(q[k] - r[k]);
        }
    }
    segment_near(a, ab, ap, d2, pt);
    segment_near(b, bc, bp, d2, pt);
    segment_near(c, ca, cp, d2, pt);
}

__global__ __launch_bounds__(kMeshLanes) void meshnear_query_kernel(MeshNearArgs a)
{
    const int64_t i = mesh_item();
    const bool in = i < a.nq;
    const MeshNearGrid &g = *a.grid;
    float p[3] = {0.0f, 0.0f, 0.0f};
    int64_t qi = 0;
    bool part = false;
    if (in) {
        qi = a.qidx_sorted[i];
        part = load_query(a, qi, p);
    }
    const float finf = __builtin_huge_valf();
    double best = __builtin_huge_val();
    int32_t who = -1;
    float where[3] = {finf, finf, finf};
    if (part) {
        const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
        int32_t w0[3], w1[3];
        for (int k = 0; k < 3; ++k) {
            const int32_t c = cell_coord(g.origin[k], g.side, g.n[k], p[k], -2.0, 1.0);
            w0[k] = max(c - 1, 0);
            w1[k] = min(c + 1, g.n[k] - 1);
        }
        for (int32_t z = w0[2]; z <= w1[2]; ++z)
            for (int32_t y = w0[1]; y <= w1[1]; ++y)
                for (int32_t x = w0[0]; x <= w1[0]; ++x) {
                    const int32_t key = (z * g.n[1] + y) * g.n[0] + x;
                    // a registration is taken from the walk's or the triangle's first cell of every axis
                    const uint32_t need = (x == w0[0] ? 0u : 1u) | (y == w0[1] ? 0u : 2u) | (z == w0[2] ? 0u : 4u);
                    const int32_t e = (int32_t)min((int64_t)a.begin[key + 1], a.entry_cap);
                    for (int32_t j = a.begin[key]; j < e; ++j) {
                        if ((a.first[j] & need) != need)
                            continue;
                        const int32_t t = a.entries[j];
                        float v[9], lo[3], hi[3];
                        for (int c = 0; c < 3; ++c) {
                            const float *f = a.verts[a.tris[3 * (int64_t)t + c]].pos; // registered: a triangle taking part
                            v[3 * c] = f[0];
                            v[3 * c + 1] = f[1];
                            v[3 * c + 2] = f[2];
                        }
                        triangle_box(v, lo, hi);
                        bool near = true;
                        for (int k = 0; k < 3; ++k)
                            near = near && (double)lo[k] - a.G <= q[k] && q[k] <= (double)hi[k] + a.G;
                        if (!near)
                            continue;
                        double d2;
                        float pt[3];
                        triangle_near(q, v, d2, pt);
                        if (d2 <= a.R2 && (d2 < best || (d2 == best && t < who))) {
                            best = d2;
                            who = t;
                            where[0] = pt[0];
                            where[1] = pt[1];
                            where[2] = pt[2];
                        }
                    }
                }
    }
    if (in) {
        const float d = who >= 0 ? (float)dpg::dvsqrt(best) : finf;
        a.index[qi] = who;
        a.dist[qi] = d;
        if (a.closest)
            for (int k = 0; k < 3; ++k)
                a.closest[3 * qi + k] = where[k];
        if (who >= 0 && a.hist) {
            const double b = floor(dpg::dvdiv((double)d, a.R) * (double)a.bins);
            const int64_t last = (int64_t)a.bins - 1, bin = (int64_t)b < last ? (int64_t)b : last;
            atomicAdd(&a.hist[bin], 1ull);
        }
    }
    const uint32_t stripe = wave_stripe();
    wave_count<kMeshNearStripes, kMeshNearCounters>(a.count, 4, part ? 1ull : 0ull, stripe);
    wave_count<kMeshNearStripes, kMeshNearCounters>(a.count, 5, part && who >= 0 ? 1ull : 0ull, stripe);
    wave_count<kMeshNearStripes, kMeshNearCounters>(a.count, 6, part && who < 0 ? 1ull : 0ull, stripe);
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

// argument checks shared by both forms (they need no device)
static int meshnear_check(dp_ctx *c, const std::string &w, const void *queries, int64_t nq, int64_t qstride,
                          const void *vertices, int64_t nv, const void *triangles, int64_t nt,
                          const dp_mesh_nearest_options *o)
{
    if (nq < 0 || nq > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n_queries must be in 0..2^31 - 1");
    if (nv < 0 || nv > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n_vertices must be in 0..2^31 - 1");
    if (nt < 0 || nt > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n_triangles must be in 0..2^31 - 1");
    if (nq > 0 && !queries)
        return fail(c, DP_E_ARG, w + ": queries must be given");
    if (nv > 0 && !vertices)
        return fail(c, DP_E_ARG, w + ": vertices must be given");
    if (nt > 0 && !triangles)
        return fail(c, DP_E_ARG, w + ": triangles must be given");
    if (qstride < 12 || qstride % 4)
        return fail(c, DP_E_ARG, w + ": query_stride must be a multiple of 4 and at least 12");
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if (!(o->max_dist > 0.0f) || !std::isfinite(o->max_dist))
        return fail(c, DP_E_ARG, w + ": max_dist must be finite and > 0");
    if (o->hist_bins < 0 || o->hist_bins > 65536)
        return fail(c, DP_E_ARG, w + ": hist_bins must be in 0..65536");
    if (o->flags)
        return fail(c, DP_E_ARG, w + ": unknown flags");
    return DP_OK;
}

// queues the search of a device mesh on s
static int meshnear_queue(dp_ctx *c, const dp_mesh_nearest_options &o, const void *d_queries, int64_t nq, int64_t qstride,
                          const dp_mesh_vertex *d_vertices, int64_t nv, const int32_t *d_triangles, int64_t nt,
                          int32_t *d_index, float *d_dist, float *d_closest, uint64_t *d_hist, hipStream_t s)
{
    dpk::MeshNearestScratch &r = c->meshnearest;
    // the cap: the power of two at or above 2 * n_triangles, within 2^16..2^24
    int cap_bits = dpk::kMeshNearCapMinBits;
    while (cap_bits < dpk::kMeshNearCapMaxBits && (1ll << cap_bits) < 2 * nt)
        ++cap_bits;
    const int32_t cap = 1 << cap_bits;
    const int end_bit = cap_bits + 1; // the key of a query that does not take part is cap itself
    const int64_t entry_cap = std::max<int64_t>(std::min<int64_t>(8 * nt, 0x7FFFFFFFll), 1);
    const int64_t box_blocks = std::min<int64_t>(dpk::mesh_blocks(nt), dpk::kMeshNearBoxBlocks);
    const size_t q = (size_t)std::max<int64_t>(nq, 1);
    DP_HIP(c, r.boxes.reserve(6 * (size_t)dpk::kMeshNearBoxBlocks));
    DP_HIP(c, r.grid.reserve(1));
    DP_HIP(c, r.levels.reserve(2 * (size_t)dpk::kMeshNearLevels));
    DP_HIP(c, r.cellcount.reserve((size_t)cap + 1));
    DP_HIP(c, r.begin.reserve((size_t)cap + 1));
    DP_HIP(c, r.entries.reserve((size_t)entry_cap));
    DP_HIP(c, r.first.reserve((size_t)entry_cap));
    DP_HIP(c, r.qkeys.reserve(q));
    DP_HIP(c, r.qkeys_sorted.reserve(q));
    DP_HIP(c, r.qidx.reserve(q));
    DP_HIP(c, r.qidx_sorted.reserve(q));
    DP_HIP(c, r.count.reserve(dpk::kMeshNearStripes, dpk::kMeshNearCounters, (sizeof(dpk::MeshNearGrid) + 7) / 8));

    dpk::MeshNearArgs a{};
    a.queries = (const char *)d_queries;
    a.verts = d_vertices;
    a.tris = d_triangles;
    a.nq = nq;
    a.qstride = qstride;
    a.nv = nv;
    a.nt = nt;
    a.entry_cap = entry_cap;
    a.cap = cap;
    a.nboxes = (int32_t)box_blocks;
    a.bins = o.hist_bins;
    a.R = (double)o.max_dist;
    a.R2 = a.R * a.R;
    a.G = a.R + a.R * 0x1p-20;
    a.boxes = r.boxes.p;
    a.grid = r.grid.p;
    a.levels = r.levels.p;
    a.cellcount = r.cellcount.p;
    a.begin = r.begin.p;
    a.entries = r.entries.p;
    a.first = r.first.p;
    a.qkeys = r.qkeys.p;
    a.qkeys_sorted = r.qkeys_sorted.p;
    a.qidx = r.qidx.p;
    a.qidx_sorted = r.qidx_sorted.p;
    a.index = d_index;
    a.dist = d_dist;
    a.closest = d_closest;
    a.hist = o.hist_bins > 0 ? (unsigned long long *)d_hist : nullptr;
    a.count = r.count.dev.p;

    size_t tmp = 0, b = 0;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, a.cellcount, a.begin, cap + 1, s));
    tmp = std::max(tmp, b);
    if (nq > 0) {
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, a.qkeys, a.qkeys_sorted, a.qidx, a.qidx_sorted, (int)nq, 0,
                                                     end_bit, s));
        tmp = std::max(tmp, b);
    }
    DP_HIP(c, c->scan_tmp.reserve(tmp ? tmp : 1));

    DP_HIP(c, r.count.zero(s));
    if (a.hist)
        DP_HIP(c, hipMemsetAsync(a.hist, 0, sizeof(unsigned long long) * (size_t)o.hist_bins, s));
    // the grid
    DP_HIP(c, r.time[0].begin(s));
    DP_HIP(c, hipMemsetAsync(a.levels, 0, sizeof(unsigned long long) * 2 * (size_t)dpk::kMeshNearLevels, s));
    DP_HIP(c, hipMemsetAsync(a.cellcount, 0, sizeof(int32_t) * ((size_t)cap + 1), s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_box_kernel, box_blocks, a, s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_plan_kernel, 1, a, s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_levels_kernel, dpk::mesh_blocks(nt), a, s));
    hipLaunchKernelGGL(dpk::meshnear_pick_kernel, dim3(1), dim3(1), 0, s, a);
    DP_HIP(c, hipGetLastError());
    DP_HIP(c, dpk::launch_over(dpk::meshnear_register_kernel<false>, dpk::mesh_blocks(nt), a, s));
    b = tmp;
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, b, a.cellcount, a.begin, cap + 1, s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_register_kernel<true>, dpk::mesh_blocks(nt), a, s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_maxcell_kernel, dpk::mesh_blocks(cap), a, s));
    DP_HIP(c, r.time[0].end(s));
    // the queries
    DP_HIP(c, r.time[1].begin(s));
    DP_HIP(c, dpk::launch_over(dpk::meshnear_qkeys_kernel, dpk::mesh_blocks(nq), a, s));
    if (nq > 0) {
        b = tmp;
        DP_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->scan_tmp.p, b, a.qkeys, a.qkeys_sorted, a.qidx, a.qidx_sorted,
                                                     (int)nq, 0, end_bit, s));
    }
    DP_HIP(c, dpk::launch_over(dpk::meshnear_query_kernel, dpk::mesh_blocks(nq), a, s));
    DP_HIP(c, r.time[1].end(s));
    return DP_OK;
}

// the statistics read and its wait
static int meshnear_stats(dp_ctx *c, int64_t nq, dp_mesh_nearest_stats *stats, hipStream_t s)
{
    dpk::MeshNearestScratch &r = c->meshnearest;
    DP_HIP(c, r.count.read(s));
    DP_HIP(c, hipMemcpyAsync(r.count.extra(), r.grid.p, sizeof(dpk::MeshNearGrid), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    const dpk::MeshNearGrid *g = (const dpk::MeshNearGrid *)r.count.extra();
    stats->triangles = r.count.sum(0);
    stats->invalid_triangles = r.count.sum(1);
    stats->degenerate_triangles = r.count.sum(2);
    stats->nonfinite_triangles = r.count.sum(3);
    stats->queries = r.count.sum(4);
    stats->skipped_queries = nq - stats->queries;
    stats->matched = r.count.sum(5);
    stats->unmatched = r.count.sum(6);
    stats->grid_cells = g->cells;
    stats->grid_entries = g->entries;
    stats->max_cell_entries = g->maxcell;
    DP_HIP(c, r.time[0].ms(stats->build_ms));
    DP_HIP(c, r.time[1].ms(stats->query_ms));
    return DP_OK;
}

extern "C" int dp_mesh_nearest_device(dp_ctx *c, const void *d_queries, int64_t n_queries, int64_t query_stride,
                                      const dp_mesh_vertex *d_vertices, int64_t n_vertices, const int32_t *d_triangles,
                                      int64_t n_triangles, const dp_mesh_nearest_options *opts, int32_t *d_index,
                                      float *d_dist, float *d_closest, uint64_t *d_hist, dp_mesh_nearest_stats *stats,
                                      void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_nearest_device";
    int rc = meshnear_check(c, w, d_queries, n_queries, query_stride, d_vertices, n_vertices, d_triangles, n_triangles, opts);
    if (rc != DP_OK)
        return rc;
    if (n_queries > 0 && !d_index)
        return fail(c, DP_E_ARG, w + ": d_index must be given");
    if (n_queries > 0 && !d_dist)
        return fail(c, DP_E_ARG, w + ": d_dist must be given");
    if ((rc = mesh_check_alias(c, w, {d_index, d_dist, d_closest, d_hist}, {d_queries, d_vertices, d_triangles})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = meshnear_queue(c, *opts, d_queries, n_queries, query_stride, d_vertices, n_vertices, d_triangles, n_triangles,
                             d_index, d_dist, d_closest, d_hist, s)) != DP_OK)
        return rc;
    return stats ? meshnear_stats(c, n_queries, stats, s) : DP_OK;
}

extern "C" int dp_mesh_nearest(dp_ctx *c, const void *queries, int64_t n_queries, int64_t query_stride,
                               const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                               int64_t n_triangles, const dp_mesh_nearest_options *opts, const int32_t **index,
                               const float **dist, const float **closest, const uint64_t **hist,
                               dp_mesh_nearest_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_nearest";
    int rc = meshnear_check(c, w, queries, n_queries, query_stride, vertices, n_vertices, triangles, n_triangles, opts);
    if (rc != DP_OK)
        return rc;
    if (!index)
        return fail(c, DP_E_ARG, w + ": index must be given");
    if (!dist)
        return fail(c, DP_E_ARG, w + ": dist must be given");
    if ((rc = mesh_check_alias(c, w, {index, dist, closest, hist}, {queries, vertices, triangles})) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::MeshNearestScratch &r = c->meshnearest;
    const int64_t nq = n_queries, nv = n_vertices, nt = n_triangles;
    const size_t bins = hist ? (size_t)opts->hist_bins : 0;
    // the queries are staged from the first point to the end of the last
    const size_t qbytes = nq > 0 ? (size_t)(nq - 1) * (size_t)query_stride + 12 : 0;
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv, tbytes = 12 * (size_t)nt;
    const size_t cbytes = closest ? 12 * (size_t)nq : 0;
    PlanePacker pin, pout;
    const size_t iq = pin.add(qbytes), iv = pin.add(vbytes), it = pin.add(tbytes);
    const size_t oi = pout.add(4 * (size_t)nq), od = pout.add(4 * (size_t)nq), oc = pout.add(cbytes),
                 oh = pout.add(8 * bins);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hindex.resize((size_t)std::max<int64_t>(nq, 1)));
    DP_HIP(c, r.hdist.resize((size_t)std::max<int64_t>(nq, 1)));
    DP_HIP(c, r.hclosest.resize(std::max<size_t>(cbytes / 4, 1)));
    DP_HIP(c, r.hhist.resize(std::max<size_t>(bins, 1)));
    if (nq > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + iq, queries, qbytes, hipMemcpyHostToDevice, s));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + iv, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + it, triangles, tbytes, hipMemcpyHostToDevice, s));
    if ((rc = meshnear_queue(c, *opts, r.in.p + iq, nq, query_stride, (const dp_mesh_vertex *)(r.in.p + iv), nv,
                             (const int32_t *)(r.in.p + it), nt, (int32_t *)(r.out.p + oi), (float *)(r.out.p + od),
                             cbytes ? (float *)(r.out.p + oc) : nullptr, bins ? (uint64_t *)(r.out.p + oh) : nullptr,
                             s)) != DP_OK)
        return rc;
    if (nq > 0) {
        DP_HIP(c, hipMemcpyAsync(r.hindex.data(), r.out.p + oi, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
        DP_HIP(c, hipMemcpyAsync(r.hdist.data(), r.out.p + od, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
        if (cbytes)
            DP_HIP(c, hipMemcpyAsync(r.hclosest.data(), r.out.p + oc, cbytes, hipMemcpyDeviceToHost, s));
    }
    if (bins)
        DP_HIP(c, hipMemcpyAsync(r.hhist.data(), r.out.p + oh, 8 * bins, hipMemcpyDeviceToHost, s));
    if (stats) {
        if ((rc = meshnear_stats(c, nq, stats, s)) != DP_OK)
            return rc;
    } else {
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *index = nq > 0 ? r.hindex.data() : nullptr;
    *dist = nq > 0 ? r.hdist.data() : nullptr;
    if (closest)
        *closest = nq > 0 ? r.hclosest.data() : nullptr;
    if (bins)
        *hist = r.hhist.data();
    return DP_OK;
}
