// dp_tsdf.hip -- gfx950 kernels of the TSDF volume and its mesh (spec in
// include/densepoints.h, dp_tsdf_integrate / dp_tsdf_mesh).
//
//   tsdf_integrate_kernel  one lane per voxel, a wave = 64 consecutive x of one
//                          (j, k) row, so its projections lie along one image
//                          line and the depth gathers stay close; the loop over
//                          the views is wave-uniform, so the view table (P, g,
//                          W, H, plane pointers) is read with scalar loads; a
//                          voxel's sums live in its lane's registers and are
//                          written once
//   mesh_count_kernel      one lane per lattice point p, which also names the
//                          cell with the low corner p: the cell's triangle
//                          count (a byte), the block's sum of them, and the
//                          edge bits of the cell's sign-changing edges OR-ed
//                          into the flag bytes of their origins (32-bit
//                          atomicOr: setting a bit is idempotent)
//   mesh_vcount_kernel     vertices per block = the set bits of its flag bytes
//   (two hipcub exclusive scans of the block counts; the last entry of each is
//   the total)
//   mesh_vertices_kernel   the first vertex number of every lattice point (the
//                          scanned offset plus the rank in the block) and the
//                          vertices themselves
//   mesh_triangles_kernel  the triangles of every cell at the scanned offset
//                          plus the rank in the block; a corner's number is its
//                          origin's first vertex plus the set bits below its
//                          direction
//
// Lattice points are linear in (k, j, i) and blocks are consecutive, so the
// vertices come out in (k, j, i, dir) order and the triangles in (cell,
// tetrahedron, triangle) order.  Nothing depends on the order in which lanes
// or blocks run.
#include "dp_ctx.h"
#include "dp_mapdev.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

namespace dpk {
namespace {

// corner codes of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Tetrahedron t
// (the permutations in lexicographic order) has the corners kTetQ[t][0..3];
// 021, 102 and 210 are odd.
__device__ const int8_t kTetQ[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ const int8_t kTetOdd[6] = {0, 1, 1, 0, 0, 1};
// edges 01 02 03 12 13 23 of a tetrahedron by their corner numbers
__device__ const int8_t kTetEdge[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// direction number of the bits dx | dy << 1 | dz << 2
__device__ const int8_t kDirOfBits[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// the header's triangle table of an even tetrahedron, as edge numbers
__device__ const int8_t kNTri[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__device__ const int8_t kTri[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {0, 0, 0}}, {{0, 5, 2}, {0, 3, 5}}, {{0, 4, 5}, {0, 5, 1}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{0, 1, 5}, {0, 5, 4}}, {{0, 5, 3}, {0, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{1, 3, 4}, {1, 4, 2}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};

__global__ __launch_bounds__(64 * kTsdfRows) void tsdf_integrate_kernel(TsdfArgs a)
{
    const TsdfVolume &g = a.vol;
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int j = (int)blockIdx.y * kTsdfRows + (int)threadIdx.y;
    const int k = (int)blockIdx.z;
    if (j >= g.ny) // the whole wave
        return;
    const bool in = i < g.nx;
    const double X[3] = {g.origin[0] + ((double)i + 0.5) * g.voxel, g.origin[1] + ((double)j + 0.5) * g.voxel,
                         g.origin[2] + ((double)k + 0.5) * g.voxel};
    double tsum = 0.0;
    int32_t w = 0;
    uint32_t sr = 0, sg = 0, sb = 0; // at most 64 x 255 each
    for (int kv = 0; kv < a.K; ++kv) {
        const TsdfView &s = a.tab[kv];
        double d;
        int32_t xi, yi;
        if (!in || !nearest_pixel(s.P, s.W, s.H, X, d, xi, yi))
            continue;
        const float z = s.depth[(int64_t)yi * s.W + xi];
        if (!is_depth(z))
            continue;
        const double sdf = ((double)z - d) / s.g;
        if (sdf < -a.trunc)
            continue;
        const double t = sdf >= a.trunc ? 1.0 : sdf / a.trunc;
        tsum = tsum + t;
        w += 1;
        const uint32_t px = s.img[(int64_t)yi * s.pitch + xi];
        sr += (px >> 16) & 255u;
        sg += (px >> 8) & 255u;
        sb += px & 255u;
    }
    float tsdf = 1.0f;
    uint32_t rgb = 0;
    if (w > 0) {
        const uint32_t uw = (uint32_t)w;
        tsdf = (float)(tsum / (double)w);
        rgb = (sr + uw / 2) / uw | ((sg + uw / 2) / uw) << 8 | ((sb + uw / 2) / uw) << 16;
    }
    if (in) {
        const int64_t at = ((int64_t)k * g.ny + j) * g.nx + i;
        if (a.tsdf)
            a.tsdf[at] = tsdf;
        if (a.weight)
            a.weight[at] = w;
        if (a.rgb)
            a.rgb[at] = rgb;
    }
    const uint32_t stripe = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kTsdfRows + threadIdx.y;
    wave_count<kTsdfStripes, kTsdfCounters>(a.count, 0, in ? 1ull : 0ull, stripe);
    wave_count<kTsdfStripes, kTsdfCounters>(a.count, 1, (unsigned long long)w, stripe);
    wave_count<kTsdfStripes, kTsdfCounters>(a.count, 2, w > 0 ? 1ull : 0ull, stripe);
    wave_count<kTsdfStripes, kTsdfCounters>(a.count, 3, w > 0 && fabsf(tsdf) < 1.0f ? 1ull : 0ull, stripe);
}

// ---- mesh ---------------------------------------------------------------------

struct Lattice {
    int64_t L;
    int i, j, k;
    bool point, cell;
};

__device__ __forceinline__ Lattice lattice_of(const MeshArgs &a)
{
    Lattice p;
    p.L = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    p.point = p.L < a.points;
    const int64_t row = p.L / a.vol.nx;
    p.i = (int)(p.L - row * a.vol.nx);
    p.j = (int)(row % a.vol.ny);
    p.k = (int)(row / a.vol.ny);
    p.cell = p.point && p.i < a.vol.nx - 1 && p.j < a.vol.ny - 1 && p.k < a.vol.nz - 1;
    return p;
}

// the lattice point at corner `code` of the cell whose low corner is L
__device__ __forceinline__ int64_t corner_at(const MeshArgs &a, int64_t L, int code)
{
    return L + (code & 1) + (int64_t)((code >> 1) & 1) * a.vol.nx + (int64_t)((code >> 2) & 1) * a.vol.nx * a.vol.ny;
}

__device__ __forceinline__ uint32_t flag_byte(const MeshArgs &a, int64_t L)
{
    return (a.flags[L >> 2] >> ((uint32_t)(L & 3) * 8u)) & 0x7Fu;
}

// bit `code` set iff the cell's corner is INSIDE; a cell only (all corners exist)
__device__ __forceinline__ uint32_t inside_bits(const MeshArgs &a, int64_t L)
{
    uint32_t in8 = 0;
#pragma unroll
    for (int code = 0; code < 8; ++code)
        in8 |= (a.tsdf[corner_at(a, L, code)] < 0.0f ? 1u : 0u) << code;
    return in8;
}

__device__ __forceinline__ uint32_t tet_mask(uint32_t in8, int t)
{
    return ((in8 >> kTetQ[t][0]) & 1u) | ((in8 >> kTetQ[t][1]) & 1u) << 1 | ((in8 >> kTetQ[t][2]) & 1u) << 2 |
           ((in8 >> kTetQ[t][3]) & 1u) << 3;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_count_kernel(MeshArgs a)
{
    __shared__ uint32_t wsum[kMeshBlock / 64];
    const Lattice p = lattice_of(a);
    uint32_t nt = 0;
    bool active = false;
    if (p.cell) {
        active = true;
#pragma unroll
        for (int code = 0; code < 8; ++code)
            active = active && a.weight[corner_at(a, p.L, code)] >= a.min_weight;
    }
    if (active) {
        const uint32_t in8 = inside_bits(a, p.L);
        if (in8 != 0u && in8 != 0xFFu) {
#pragma unroll
            for (int t = 0; t < 6; ++t)
                nt += (uint32_t)kNTri[tet_mask(in8, t)];
            // the cell's edges are the pairs lo < hi of corner codes with lo a
            // subset of hi: every one of them is an edge of a Kuhn tetrahedron
#pragma unroll
            for (int lo = 0; lo < 7; ++lo) {
                uint32_t f = 0;
#pragma unroll
                for (int hi = lo + 1; hi < 8; ++hi)
                    if ((lo & hi) == lo)
                        f |= (((in8 >> lo) ^ (in8 >> hi)) & 1u) << kDirOfBits[lo ^ hi];
                if (f) {
                    const int64_t at = corner_at(a, p.L, lo);
                    atomicOr(&a.flags[at >> 2], f << ((uint32_t)(at & 3) * 8u));
                }
            }
        }
    }
    if (p.point)
        a.tcount[p.L] = (uint8_t)nt;
    const uint32_t total = block_sum<kMeshBlock>(nt, wsum);
    if (threadIdx.x == 0)
        a.bcount[a.blocks + 1 + blockIdx.x] = total;
    wave_count<kTsdfStripes, 1>(a.active, 0, active ? 1ull : 0ull, blockIdx.x * (kMeshBlock / 64) + (threadIdx.x >> 6));
}

__global__ __launch_bounds__(kMeshBlock) void mesh_vcount_kernel(MeshArgs a)
{
    __shared__ uint32_t wsum[kMeshBlock / 64];
    const Lattice p = lattice_of(a);
    const uint32_t total = block_sum<kMeshBlock>(p.point ? (uint32_t)__popc(flag_byte(a, p.L)) : 0u, wsum);
    if (threadIdx.x == 0)
        a.bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_vertices_kernel(MeshArgs a)
{
    __shared__ uint32_t wsum[kMeshBlock / 64];
    const Lattice p = lattice_of(a);
    const uint32_t f = p.point ? flag_byte(a, p.L) : 0u;
    const int64_t base = (int64_t)a.boff[blockIdx.x] + block_exclusive((uint32_t)__popc(f), wsum);
    if (p.point)
        a.vbase[p.L] = (uint32_t)base;
    if (!f || base >= a.vcap)
        return;
    const TsdfVolume &g = a.vol;
    const double av = (double)a.tsdf[p.L];
    const uint32_t wa = a.rgb ? a.rgb[p.L] : 0u;
    const int idx[3] = {p.i, p.j, p.k};
    int64_t id = base;
    for (int dir = 0; dir < 7; ++dir) {
        if (!((f >> dir) & 1u))
            continue;
        if (id >= a.vcap)
            break;
        // the direction's bits: 0, 1, 2 are the axes, then xy, xz, yz, xyz
        const int bits = dir < 3 ? 1 << dir : dir == 3 ? 3 : dir == 4 ? 5 : dir == 5 ? 6 : 7;
        const int64_t B = corner_at(a, p.L, bits); // a set bit's edge lies in a cell, so B exists
        const double bv = (double)a.tsdf[B];
        const double s = av / (av - bv);
        dp_mesh_vertex vtx;
        for (int c = 0; c < 3; ++c) {
            const double XA = g.origin[c] + ((double)idx[c] + 0.5) * g.voxel;
            const double XB = g.origin[c] + ((double)(idx[c] + ((bits >> c) & 1)) + 0.5) * g.voxel;
            vtx.pos[c] = (float)(XA + s * (XB - XA));
        }
        const uint32_t wb = a.rgb ? a.rgb[B] : 0u;
        for (int c = 0; c < 3; ++c) {
            const double ca = (double)((wa >> (8 * c)) & 255u), cb = (double)((wb >> (8 * c)) & 255u);
            vtx.rgb[c] = (uint8_t)(int32_t)rint(ca + s * (cb - ca));
        }
        vtx.pad = 0;
        a.verts[id] = vtx;
        ++id;
    }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_triangles_kernel(MeshArgs a)
{
    __shared__ uint32_t wsum[kMeshBlock / 64];
    const Lattice p = lattice_of(a);
    const uint32_t nt = p.point ? (uint32_t)a.tcount[p.L] : 0u;
    int64_t id = (int64_t)a.boff[a.blocks + 1 + blockIdx.x] + block_exclusive(nt, wsum);
    if (!nt || id >= a.tcap)
        return;
    // nt > 0: an active cell
    const uint32_t in8 = inside_bits(a, p.L);
    for (int t = 0; t < 6; ++t) {
        const uint32_t m = tet_mask(in8, t);
        for (int r = 0; r < kNTri[m]; ++r, ++id) {
            if (id >= a.tcap)
                return;
            int32_t v[3];
            for (int c = 0; c < 3; ++c) {
                const int e = kTri[m][r][c];
                const int lo = kTetQ[t][kTetEdge[e][0]], hi = kTetQ[t][kTetEdge[e][1]];
                const int64_t at = corner_at(a, p.L, lo);
                const uint32_t below = (1u << kDirOfBits[lo ^ hi]) - 1u;
                v[c] = (int32_t)(a.vbase[at] + (uint32_t)__popc(flag_byte(a, at) & below));
            }
            const bool odd = kTetOdd[t] != 0;
            a.tris[3 * id] = v[0];
            a.tris[3 * id + 1] = odd ? v[2] : v[1];
            a.tris[3 * id + 2] = odd ? v[1] : v[2];
        }
    }
}

} // namespace

hipError_t launch_tsdf_integrate(const TsdfArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)((a.vol.nx + 63) / 64), (unsigned)((a.vol.ny + kTsdfRows - 1) / kTsdfRows),
                    (unsigned)a.vol.nz);
    hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(64, kTsdfRows), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mesh_count(const MeshArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mesh_vcount(const MeshArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_vcount_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mesh_vertices(const MeshArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mesh_triangles(const MeshArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    return hipGetLastError();
}

} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_tsdf_options(dp_tsdf_options *to)
{
    if (!to)
        return;
    *to = dp_tsdf_options{};
    to->min_weight = 1;
}

// the option ranges shared by all four calls (they need no device)
static int tsdf_check_options(dp_ctx *c, const char *who, const dp_tsdf_options *o)
{
    if (!c)
        return DP_E_ARG;
    const std::string w(who);
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(o->origin[a]))
            return fail(c, DP_E_ARG, w + ": origin must be finite");
    if (!(o->voxel > 0.0f) || !std::isfinite(o->voxel))
        return fail(c, DP_E_ARG, w + ": voxel must be finite and > 0");
    if (!(o->trunc > 0.0f) || !std::isfinite(o->trunc))
        return fail(c, DP_E_ARG, w + ": trunc must be finite and > 0");
    int64_t points = 1;
    for (int a = 0; a < 3; ++a) {
        if (o->dim[a] < 2 || o->dim[a] > 1024)
            return fail(c, DP_E_ARG, w + ": every dim must be in 2..1024");
        points *= o->dim[a];
    }
    if (points > (1ll << 30))
        return fail(c, DP_E_ARG, w + ": at most 2^30 voxels");
    if (o->min_weight < 1 || o->min_weight > 64)
        return fail(c, DP_E_ARG, w + ": min_weight must be in 1..64");
    if (o->flags != 0)
        return fail(c, DP_E_ARG, w + ": unknown flag bits");
    return DP_OK;
}

static dpk::TsdfVolume tsdf_volume(const dp_tsdf_options &o)
{
    dpk::TsdfVolume g{};
    for (int a = 0; a < 3; ++a)
        g.origin[a] = (double)o.origin[a];
    g.voxel = (double)o.voxel;
    g.nx = o.dim[0];
    g.ny = o.dim[1];
    g.nz = o.dim[2];
    return g;
}

static int64_t tsdf_points(const dp_tsdf_options &o) { return (int64_t)o.dim[0] * o.dim[1] * o.dim[2]; }

// the integration's argument checks (they need no device)
static int tsdf_check_views(dp_ctx *c, const int32_t *views, int n_views, const float *const *depth)
{
    const int rc = check_view_list(c, "dp_tsdf_integrate", views, n_views, 64);
    if (rc != DP_OK)
        return rc;
    if (!depth)
        return fail(c, DP_E_ARG, "dp_tsdf_integrate: depth planes must be given");
    for (int k = 0; k < n_views; ++k)
        if (!depth[k])
            return fail(c, DP_E_ARG, "dp_tsdf_integrate: a plane pointer is NULL");
    return DP_OK;
}

extern "C" int dp_tsdf_integrate_device(dp_ctx *c, const int32_t *views, int n_views, const dp_tsdf_options *opts,
                                        const float *const *d_depth, float *d_tsdf, int32_t *d_weight,
                                        uint32_t *d_rgb, dp_tsdf_stats *stats, void *stream)
{
    int rc = tsdf_check_options(c, "dp_tsdf_integrate", opts);
    if (rc != DP_OK)
        return rc;
    rc = tsdf_check_views(c, views, n_views, d_depth);
    if (rc != DP_OK)
        return rc;
    std::vector<dpk::TsdfView> tab((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const dpg::ViewDev &v = c->hv[views[k]];
        dpk::TsdfView &t = tab[(size_t)k];
        for (int j = 0; j < 12; ++j)
            t.P[j] = v.P[j];
        const double m2[3] = {v.P[8], v.P[9], v.P[10]};
        t.g = std::sqrt(dpg::dot3(m2, m2));
        if (!(t.g > 0.0) || !std::isfinite(t.g))
            return fail(c, DP_E_ARG, "dp_tsdf_integrate: a requested view's third row has no finite, positive length");
        t.depth = d_depth[k];
        t.img = v.img;
        t.W = v.W;
        t.H = v.H;
        t.pitch = v.pitch;
        t.view = views[k];
    }
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    StripedCounters &n = c->tsdf.count;
    DP_HIP(c, c->tsdf.tab.reserve((size_t)n_views));
    DP_HIP(c, n.reserve(dpk::kTsdfStripes, dpk::kTsdfCounters));

    dpk::TsdfArgs a{};
    a.tab = c->tsdf.tab.p;
    a.K = n_views;
    a.vol = tsdf_volume(*opts);
    a.trunc = (double)opts->trunc;
    a.tsdf = d_tsdf;
    a.weight = d_weight;
    a.rgb = d_rgb;
    a.count = n.dev.p;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the table is read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(c->tsdf.tab.p, tab.data(), sizeof(dpk::TsdfView) * tab.size(), hipMemcpyHostToDevice, s));
    DP_HIP(c, n.zero(s));
    DP_HIP(c, c->tsdf.time[0].begin(s));
    DP_HIP(c, dpk::launch_tsdf_integrate(a, s));
    DP_HIP(c, c->tsdf.time[0].end(s));
    if (!stats)
        return DP_OK;
    DP_HIP(c, n.read(s));
    DP_HIP(c, hipStreamSynchronize(s));
    stats->voxels = n.sum(0);
    stats->observations = n.sum(1);
    stats->observed_voxels = n.sum(2);
    stats->near_voxels = n.sum(3);
    DP_HIP(c, c->tsdf.time[0].ms(stats->integrate_ms));
    return DP_OK;
}

extern "C" int dp_tsdf_integrate(dp_ctx *c, const int32_t *views, int n_views, const dp_tsdf_options *opts,
                                 const float *const *depth, float *tsdf, int32_t *weight, uint32_t *rgb,
                                 dp_tsdf_stats *stats)
{
    int rc = tsdf_check_options(c, "dp_tsdf_integrate", opts);
    if (rc != DP_OK)
        return rc;
    rc = tsdf_check_views(c, views, n_views, depth);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // device copies of the planes, 256-B aligned, in one buffer; the three
    // output volumes in another
    std::vector<size_t> od((size_t)n_views);
    PlanePacker pack;
    for (int k = 0; k < n_views; ++k)
        od[(size_t)k] = pack.add(4 * view_pixels(c, views[k]));
    const size_t vol = 4 * (size_t)tsdf_points(*opts);
    DP_HIP(c, c->tsdf.in.reserve(pack.total ? pack.total : 1));
    DP_HIP(c, c->tsdf.vol.reserve(3 * vol));
    std::vector<const float *> dd((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        dd[(size_t)k] = (const float *)(c->tsdf.in.p + od[(size_t)k]);
        DP_HIP(c, hipMemcpyAsync(c->tsdf.in.p + od[(size_t)k], depth[k], 4 * view_pixels(c, views[k]),
                                 hipMemcpyHostToDevice, s));
    }
    unsigned char *o = c->tsdf.vol.p;
    rc = dp_tsdf_integrate_device(c, views, n_views, opts, dd.data(), tsdf ? (float *)o : nullptr,
                                  weight ? (int32_t *)(o + vol) : nullptr, rgb ? (uint32_t *)(o + 2 * vol) : nullptr,
                                  stats, s);
    if (rc != DP_OK)
        return rc;
    if (tsdf)
        DP_HIP(c, hipMemcpyAsync(tsdf, o, vol, hipMemcpyDeviceToHost, s));
    if (weight)
        DP_HIP(c, hipMemcpyAsync(weight, o + vol, vol, hipMemcpyDeviceToHost, s));
    if (rgb)
        DP_HIP(c, hipMemcpyAsync(rgb, o + 2 * vol, vol, hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}

namespace {

// The mesh in two queued phases: the counts and their scans, then the emission
// into buffers of a known capacity.  The device form queues both and waits once;
// the host form reads the totals in between to size its buffers.
struct MeshRun {
    dpk::MeshArgs a{};
    size_t scan_bytes = 0;
};

int mesh_prepare(dp_ctx *c, const dp_tsdf_options &o, const float *d_tsdf, const int32_t *d_weight,
                 const uint32_t *d_rgb, hipStream_t s, MeshRun &run)
{
    dpk::MeshArgs &a = run.a;
    a.vol = tsdf_volume(o);
    a.min_weight = o.min_weight;
    a.points = tsdf_points(o);
    a.blocks = (a.points + dpk::kMeshBlock - 1) / dpk::kMeshBlock;
    const size_t words = (size_t)(a.points / 4 + 1), nb = (size_t)a.blocks + 1;
    DP_HIP(c, c->tsdf.flags.reserve(words));
    DP_HIP(c, c->tsdf.tcount.reserve((size_t)a.points));
    DP_HIP(c, c->tsdf.vbase.reserve((size_t)a.points));
    DP_HIP(c, c->tsdf.bcount.reserve(2 * nb));
    DP_HIP(c, c->tsdf.boff.reserve(2 * nb));
    DP_HIP(c, c->tsdf.count.reserve(dpk::kTsdfStripes, 1, 2));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, run.scan_bytes, c->tsdf.bcount.p, c->tsdf.boff.p, (int)nb, s));
    DP_HIP(c, c->scan_tmp.reserve(run.scan_bytes ? run.scan_bytes : 1));
    a.tsdf = d_tsdf;
    a.weight = d_weight;
    a.rgb = d_rgb;
    a.flags = c->tsdf.flags.p;
    a.tcount = c->tsdf.tcount.p;
    a.vbase = c->tsdf.vbase.p;
    a.bcount = c->tsdf.bcount.p;
    a.boff = c->tsdf.boff.p;
    a.active = c->tsdf.count.dev.p;
    return DP_OK;
}

// phase 1
int mesh_count(dp_ctx *c, MeshRun &run, hipStream_t s)
{
    const dpk::MeshArgs &a = run.a;
    const size_t nb = (size_t)a.blocks + 1;
    DP_HIP(c, hipMemsetAsync(c->tsdf.flags.p, 0, sizeof(uint32_t) * (size_t)(a.points / 4 + 1), s));
    DP_HIP(c, c->tsdf.count.zero(s));
    DP_HIP(c, hipMemsetAsync(c->tsdf.bcount.p + a.blocks, 0, sizeof(unsigned long long), s));
    DP_HIP(c, hipMemsetAsync(c->tsdf.bcount.p + nb + a.blocks, 0, sizeof(unsigned long long), s));
    DP_HIP(c, dpk::launch_mesh_count(a, s));
    DP_HIP(c, dpk::launch_mesh_vcount(a, s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, run.scan_bytes, c->tsdf.bcount.p, c->tsdf.boff.p, (int)nb,
                                               s));
    DP_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, run.scan_bytes, c->tsdf.bcount.p + nb, c->tsdf.boff.p + nb,
                                               (int)nb, s));
    return DP_OK;
}

// the active cells' stripes and, behind them, the vertex and the triangle total; waits
int mesh_read_totals(dp_ctx *c, const MeshRun &run, hipStream_t s)
{
    const dpk::MeshArgs &a = run.a;
    const size_t nb = (size_t)a.blocks + 1;
    unsigned long long *h = c->tsdf.count.extra();
    DP_HIP(c, c->tsdf.count.read(s));
    DP_HIP(c, hipMemcpyAsync(h, c->tsdf.boff.p + a.blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipMemcpyAsync(h + 1, c->tsdf.boff.p + nb + a.blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             s));
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}

int mesh_emit(dp_ctx *c, MeshRun &run, dp_mesh_vertex *d_vertices, int64_t vcap, int32_t *d_triangles, int64_t tcap,
              hipStream_t s)
{
    dpk::MeshArgs &a = run.a;
    a.verts = d_vertices;
    a.vcap = vcap;
    a.tris = d_triangles;
    a.tcap = tcap;
    DP_HIP(c, dpk::launch_mesh_vertices(a, s));
    DP_HIP(c, dpk::launch_mesh_triangles(a, s));
    return DP_OK;
}

// the totals read into the caller's counts and statistics
int mesh_finish(dp_ctx *c, double ms, int64_t *n_vertices, int64_t *n_triangles, dp_mesh_stats *stats)
{
    *n_vertices = (int64_t)c->tsdf.count.extra()[0];
    *n_triangles = (int64_t)c->tsdf.count.extra()[1];
    if (stats) {
        stats->active_cells = c->tsdf.count.sum(0);
        stats->vertices = *n_vertices;
        stats->triangles = *n_triangles;
        stats->mesh_ms = ms;
    }
    if (*n_vertices > 0x7FFFFFFFll || *n_triangles > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, "dp_tsdf_mesh: more than 2^31 - 1 vertices or triangles");
    return DP_OK;
}

int mesh_check(dp_ctx *c, const dp_tsdf_options *opts, const void *tsdf, const void *weight, const void *nv,
               const void *nt)
{
    const int rc = tsdf_check_options(c, "dp_tsdf_mesh", opts);
    if (rc != DP_OK)
        return rc;
    if (!tsdf || !weight)
        return fail(c, DP_E_ARG, "dp_tsdf_mesh: the tsdf and weight planes must be given");
    if (!nv || !nt)
        return fail(c, DP_E_ARG, "dp_tsdf_mesh: n_vertices and n_triangles must be given");
    return DP_OK;
}

} // namespace

extern "C" int dp_tsdf_mesh_device(dp_ctx *c, const dp_tsdf_options *opts, const float *d_tsdf,
                                   const int32_t *d_weight, const uint32_t *d_rgb, dp_mesh_vertex *d_vertices,
                                   int64_t vertex_cap, int64_t *n_vertices, int32_t *d_triangles,
                                   int64_t triangle_cap, int64_t *n_triangles, dp_mesh_stats *stats, void *stream)
{
    int rc = mesh_check(c, opts, d_tsdf, d_weight, n_vertices, n_triangles);
    if (rc != DP_OK)
        return rc;
    if (vertex_cap < 0 || triangle_cap < 0 || (vertex_cap > 0 && !d_vertices) || (triangle_cap > 0 && !d_triangles))
        return fail(c, DP_E_ARG, "dp_tsdf_mesh_device: a cap must be >= 0, with its buffer given when > 0");
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    MeshRun run;
    if ((rc = mesh_prepare(c, *opts, d_tsdf, d_weight, d_rgb, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.time[0].begin(s));
    if ((rc = mesh_count(c, run, s)) != DP_OK)
        return rc;
    if ((rc = mesh_emit(c, run, d_vertices, vertex_cap, d_triangles, triangle_cap, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.time[0].end(s));
    // the one wait: the totals
    if ((rc = mesh_read_totals(c, run, s)) != DP_OK)
        return rc;
    double ms = 0.0;
    DP_HIP(c, c->tsdf.time[0].ms(ms));
    return mesh_finish(c, ms, n_vertices, n_triangles, stats);
}

extern "C" int dp_tsdf_mesh(dp_ctx *c, const dp_tsdf_options *opts, const float *tsdf, const int32_t *weight,
                            const uint32_t *rgb, const dp_mesh_vertex **vertices, int64_t *n_vertices,
                            const int32_t **triangles, int64_t *n_triangles, dp_mesh_stats *stats)
{
    int rc = mesh_check(c, opts, tsdf, weight, n_vertices, n_triangles);
    if (rc != DP_OK)
        return rc;
    if (!vertices || !triangles)
        return fail(c, DP_E_ARG, "dp_tsdf_mesh: vertices and triangles must be given");
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    const size_t vol = 4 * (size_t)tsdf_points(*opts);
    DP_HIP(c, c->tsdf.in.reserve(3 * vol));
    unsigned char *in = c->tsdf.in.p;
    DP_HIP(c, hipMemcpyAsync(in, tsdf, vol, hipMemcpyHostToDevice, s));
    DP_HIP(c, hipMemcpyAsync(in + vol, weight, vol, hipMemcpyHostToDevice, s));
    if (rgb)
        DP_HIP(c, hipMemcpyAsync(in + 2 * vol, rgb, vol, hipMemcpyHostToDevice, s));
    MeshRun run;
    if ((rc = mesh_prepare(c, *opts, (const float *)in, (const int32_t *)(in + vol),
                           rgb ? (const uint32_t *)(in + 2 * vol) : nullptr, s, run)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.time[0].begin(s));
    if ((rc = mesh_count(c, run, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.time[0].end(s));
    if ((rc = mesh_read_totals(c, run, s)) != DP_OK)
        return rc;
    double ms0 = 0.0, ms1 = 0.0;
    DP_HIP(c, c->tsdf.time[0].ms(ms0));
    int64_t nv = 0, nt = 0;
    if ((rc = mesh_finish(c, 0.0, &nv, &nt, nullptr)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.verts.reserve((size_t)std::max<int64_t>(nv, 1)));
    DP_HIP(c, c->tsdf.tris.reserve((size_t)std::max<int64_t>(3 * nt, 1)));
    DP_HIP(c, c->tsdf.hverts.resize((size_t)std::max<int64_t>(nv, 1)));
    DP_HIP(c, c->tsdf.htris.resize((size_t)std::max<int64_t>(3 * nt, 1)));
    DP_HIP(c, c->tsdf.time[1].begin(s));
    if ((rc = mesh_emit(c, run, c->tsdf.verts.p, nv, c->tsdf.tris.p, nt, s)) != DP_OK)
        return rc;
    DP_HIP(c, c->tsdf.time[1].end(s));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(c->tsdf.hverts.data(), c->tsdf.verts.p, sizeof(dp_mesh_vertex) * (size_t)nv,
                                 hipMemcpyDeviceToHost, s));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(c->tsdf.htris.data(), c->tsdf.tris.p, sizeof(int32_t) * 3 * (size_t)nt,
                                 hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    DP_HIP(c, c->tsdf.time[1].ms(ms1));
    *vertices = nv > 0 ? c->tsdf.hverts.data() : nullptr;
    *triangles = nt > 0 ? c->tsdf.htris.data() : nullptr;
    return mesh_finish(c, ms0 + ms1, n_vertices, n_triangles, stats);
}
