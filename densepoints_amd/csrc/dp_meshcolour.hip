// dp_meshcolour.hip -- the gfx950 kernel of the mesh's vertex colours (spec in
// include/densepoints.h, dp_mesh_colour) and its C ABI: every vertex is
// projected into the requested views, a depth plane of the mesh per view decides
// which of them see it, and its colour becomes the weighted mean of their texels.
//
//   mesh_colour_kernel   one lane per vertex, a wave = 64 consecutive vertices
//                        (dp_tsdf_mesh numbers them in (k, j, i) order, so
//                        neighbouring lanes gather neighbouring texels); the
//                        loop over the views is the outer, wave-uniform one, so
//                        the view table (P, C, sizes, plane pointers) is read
//                        with scalar loads; one 16-byte record in, one out
//
// A vertex's sums are its own and run over the views in order: nothing is
// shared between lanes but the statistics, which go through striped counters
// (wave_count) that the host sums.
#include "dp_meshdev.h"

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

constexpr int kMeshColourCounters = 7; // vertices, projected, occluded, grazing, visible pairs, coloured, unseen
constexpr int kMeshColourStripes = 64; // each counter kept kMeshColourStripes times (summed by the host)

struct MeshColourArgs {
    const MeshColourView *tab;
    int32_t K, bilinear, clear_unseen, pad;
    double tol, min_cos; // (double)depth_tol, (double)min_cos
    const dp_mesh_vertex *verts;
    const float *normals; // 3 per vertex, or null
    int64_t nv;
    dp_mesh_vertex *out;
    unsigned long long *seen; // optional
    int32_t *best;            // optional
    unsigned long long *count; // kMeshColourStripes x kMeshColourCounters
};

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }

// the R, G, B bytes of a BGRA8 texel as fp64
__device__ __forceinline__ void texel_rgb(uint32_t px, double *t)
{
    t[0] = (double)((px >> 16) & 255u);
    t[1] = (double)((px >> 8) & 255u);
    t[2] = (double)(px & 255u);
}

// step 5 with DP_MESH_COLOUR_BILINEAR: the four clamped taps around (u, v)
__device__ __forceinline__ void sample_bilinear(const MeshColourView &s, double u, double v, double *val)
{
    const double fu = floor(u), fv = floor(v);
    const int32_t x0 = (int32_t)fu, y0 = (int32_t)fv;
    const double fx = u - fu, fy = v - fv;
    const int32_t xa = dpg::clampi(x0, 0, s.W - 1), xb = dpg::clampi(x0 + 1, 0, s.W - 1);
    const int32_t ya = dpg::clampi(y0, 0, s.H - 1), yb = dpg::clampi(y0 + 1, 0, s.H - 1);
    const uint32_t *ra = s.img + (int64_t)ya * s.pitch, *rb = s.img + (int64_t)yb * s.pitch;
    double taa[3], tba[3], tab[3], tbb[3];
    texel_rgb(ra[xa], taa);
    texel_rgb(ra[xb], tba);
    texel_rgb(rb[xa], tab);
    texel_rgb(rb[xb], tbb);
    for (int ch = 0; ch < 3; ++ch) {
        const double top = (1.0 - fx) * taa[ch] + fx * tba[ch];
        const double bot = (1.0 - fx) * tab[ch] + fx * tbb[ch];
        val[ch] = (1.0 - fy) * top + fy * bot;
    }
}

__global__ __launch_bounds__(kMeshLanes) void mesh_colour_kernel(MeshColourArgs a)
{
    const int64_t i = mesh_item();
    const bool in = i < a.nv;
    dp_mesh_vertex vx{};
    if (in)
        vx = a.verts[i];
    const bool part = in && finite_f32(vx.pos[0]) && finite_f32(vx.pos[1]) && finite_f32(vx.pos[2]);
    const double X[3] = {(double)vx.pos[0], (double)vx.pos[1], (double)vx.pos[2]};
    double n[3] = {0.0, 0.0, 0.0}, l2 = 0.0;
    bool has_normal = false;
    if (part && a.normals) {
        for (int j = 0; j < 3; ++j)
            n[j] = (double)a.normals[3 * i + j];
        l2 = dpg::dot3(n, n);
        has_normal = l2 > 0.0 && l2 <= 1.7976931348623157e308;
    }
    double wsum = 0.0, sum[3] = {0.0, 0.0, 0.0}, bw = 0.0;
    unsigned long long mask = 0;
    int32_t best = -1;
    uint32_t projected = 0, occluded = 0, grazing = 0;
    if (__any(part)) {
        for (int k = 0; k < a.K; ++k) {
            const MeshColourView &s = a.tab[k];
            double d;
            int32_t xi, yi;
            if (!part || !nearest_pixel(s.P, s.W, s.H, X, d, xi, yi))
                continue;
            const float z = s.depth[(int64_t)yi * s.W + xi];
            if (!is_depth(z))
                continue;
            ++projected;
            if (!(d - (double)z <= a.tol * d)) {
                ++occluded;
                continue;
            }
            double wgt = 1.0;
            if (has_normal) {
                const double ray[3] = {X[0] - s.C[0], X[1] - s.C[1], X[2] - s.C[2]};
                const double q = dpg::dot3(ray, ray) * l2;
                bool faces = q > 0.0 && q <= 1.7976931348623157e308;
                if (faces) {
                    wgt = dpg::dvdiv(0.0 - dpg::dot3(n, ray), dpg::dvsqrt(q));
                    faces = wgt > 0.0 && wgt >= a.min_cos;
                }
                if (!faces) {
                    ++grazing;
                    continue;
                }
            }
            double val[3];
            if (a.bilinear) {
                // u, v as nearest_pixel divided them
                double u, v;
                dpg::div2(row_of(s.P, 0, X), row_of(s.P, 1, X), d, u, v);
                sample_bilinear(s, u, v, val);
            } else {
                texel_rgb(s.img[(int64_t)yi * s.pitch + xi], val);
            }
            for (int ch = 0; ch < 3; ++ch)
                sum[ch] = sum[ch] + wgt * val[ch];
            wsum = wsum + wgt;
            mask |= 1ull << k;
            if (wgt > bw) {
                bw = wgt;
                best = k;
            }
        }
    }
    if (in) {
        dp_mesh_vertex o = vx;
        if (mask) {
            for (int ch = 0; ch < 3; ++ch)
                o.rgb[ch] = (uint8_t)(int32_t)fmin(255.0, rint(dpg::dvdiv(sum[ch], wsum)));
        } else if (part && a.clear_unseen) {
            o.rgb[0] = o.rgb[1] = o.rgb[2] = 0;
        }
        a.out[i] = o;
        if (a.seen)
            a.seen[i] = mask;
        if (a.best)
            a.best[i] = best;
    }
    const uint32_t stripe = blockIdx.x * (kMeshLanes / 64) + (threadIdx.x >> 6);
    const uint32_t visible = (uint32_t)__popcll(mask);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 0, part ? 1ull : 0ull, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 1, (unsigned long long)projected, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 2, (unsigned long long)occluded, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 3, (unsigned long long)grazing, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 4, (unsigned long long)visible, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 5, part && mask ? 1ull : 0ull, stripe);
    wave_count<kMeshColourStripes, kMeshColourCounters>(a.count, 6, part && !mask ? 1ull : 0ull, stripe);
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mesh_colour_options(dp_mesh_colour_options *mco)
{
    if (!mco)
        return;
    mco->depth_tol = 0.01f;
    mco->min_cos = 0.2f;
    mco->flags = 0;
}

// argument checks shared by both forms (they need no device); fills the view
// table but for its depth planes
static int meshcolour_check(dp_ctx *c, const std::string &w, const void *vertices, int64_t nv, const int32_t *views,
                            int n_views, const dp_mesh_colour_options &o, const float *const *depth,
                            std::vector<dpk::MeshColourView> &tab)
{
    int rc = mesh_check_counts(c, w, nullptr, 0, nv);
    if (rc != DP_OK)
        return rc;
    if (nv > 0 && !vertices)
        return fail(c, DP_E_ARG, w + ": vertices must be given");
    if (!(o.depth_tol >= 0.0f) || !std::isfinite(o.depth_tol))
        return fail(c, DP_E_ARG, w + ": depth_tol must be finite and >= 0");
    if (!(o.min_cos >= 0.0f && o.min_cos <= 1.0f))
        return fail(c, DP_E_ARG, w + ": min_cos must be in 0..1");
    if (o.flags & ~(DP_MESH_COLOUR_BILINEAR | DP_MESH_COLOUR_CLEAR_UNSEEN))
        return fail(c, DP_E_ARG, w + ": unknown flags");
    if ((rc = check_view_list(c, w.c_str(), views, n_views, 64)) != DP_OK)
        return rc;
    if (!depth)
        return fail(c, DP_E_ARG, w + ": depth planes must be given");
    tab.resize((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        if (!depth[k])
            return fail(c, DP_E_ARG, w + ": a plane pointer is NULL");
        const dpg::ViewDev &v = c->hv[views[k]];
        dpk::MeshColourView &t = tab[(size_t)k];
        dpk::ViewInv inv;
        if (!view_inverse(v, inv))
            return fail(c, DP_E_ARG, w + ": a requested view's left 3x3 is singular");
        const double *P = inv.P, *A = inv.A;
        for (int j = 0; j < 12; ++j)
            t.P[j] = P[j];
        for (int j = 0; j < 3; ++j) {
            t.C[j] = ((A[3 * j] * (0.0 - P[3]) + A[3 * j + 1] * (0.0 - P[7])) + A[3 * j + 2] * (0.0 - P[11])) / inv.det;
            if (!std::isfinite(t.C[j]))
                return fail(c, DP_E_ARG, w + ": a requested view's camera centre is not finite");
        }
        if ((int64_t)v.W * v.H > 0x7FFFFFFFll)
            return fail(c, DP_E_ARG, w + ": view too large");
        t.depth = nullptr;
        t.img = v.img;
        t.W = v.W;
        t.H = v.H;
        t.pitch = v.pitch;
        t.view = views[k];
    }
    return DP_OK;
}

// queues the colouring of device vertices on s
static int meshcolour_queue(dp_ctx *c, std::vector<dpk::MeshColourView> &tab, const dp_mesh_colour_options &o,
                            const dp_mesh_vertex *d_vertices, int64_t nv, const float *d_normals,
                            const float *const *d_depth, dp_mesh_vertex *d_out, uint64_t *d_seen, int32_t *d_best,
                            hipStream_t s)
{
    dpk::MeshColourScratch &r = c->meshcolour;
    for (size_t k = 0; k < tab.size(); ++k)
        tab[k].depth = d_depth[k];
    DP_HIP(c, r.tab.reserve(tab.size()));
    DP_HIP(c, r.count.reserve(dpk::kMeshColourStripes, dpk::kMeshColourCounters));

    dpk::MeshColourArgs a{};
    a.tab = r.tab.p;
    a.K = (int32_t)tab.size();
    a.bilinear = (o.flags & DP_MESH_COLOUR_BILINEAR) ? 1 : 0;
    a.clear_unseen = (o.flags & DP_MESH_COLOUR_CLEAR_UNSEEN) ? 1 : 0;
    a.tol = (double)o.depth_tol;
    a.min_cos = (double)o.min_cos;
    a.verts = d_vertices;
    a.normals = d_normals;
    a.nv = nv;
    a.out = d_out;
    a.seen = (unsigned long long *)d_seen;
    a.best = d_best;
    a.count = r.count.dev.p;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the table is read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(r.tab.p, tab.data(), sizeof(dpk::MeshColourView) * tab.size(), hipMemcpyHostToDevice, s));
    DP_HIP(c, r.count.zero(s));
    DP_HIP(c, r.time.begin(s));
    DP_HIP(c, dpk::launch_over(dpk::mesh_colour_kernel, dpk::mesh_blocks(nv), a, s));
    DP_HIP(c, r.time.end(s));
    return DP_OK;
}

// the statistics read and its wait
static int meshcolour_stats(dp_ctx *c, dp_mesh_colour_stats *stats, hipStream_t s)
{
    StripedCounters &n = c->meshcolour.count;
    DP_HIP(c, n.read(s));
    DP_HIP(c, hipStreamSynchronize(s));
    stats->vertices = n.sum(0);
    stats->projected_pairs = n.sum(1);
    stats->occluded_pairs = n.sum(2);
    stats->grazing_pairs = n.sum(3);
    stats->visible_pairs = n.sum(4);
    stats->coloured_vertices = n.sum(5);
    stats->unseen_vertices = n.sum(6);
    DP_HIP(c, c->meshcolour.time.ms(stats->colour_ms));
    return DP_OK;
}

extern "C" int dp_mesh_colour_device(dp_ctx *c, const dp_mesh_vertex *d_vertices, int64_t n_vertices,
                                     const float *d_normals, const int32_t *views, int n_views,
                                     const dp_mesh_colour_options *mco, const float *const *d_depth,
                                     dp_mesh_vertex *d_vertices_out, uint64_t *d_seen, int32_t *d_best,
                                     dp_mesh_colour_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_colour_device";
    dp_mesh_colour_options o;
    dp_default_mesh_colour_options(&o);
    if (mco)
        o = *mco;
    std::vector<dpk::MeshColourView> tab;
    int rc = meshcolour_check(c, w, d_vertices, n_vertices, views, n_views, o, d_depth, tab);
    if (rc != DP_OK)
        return rc;
    if (n_vertices > 0 && !d_vertices_out)
        return fail(c, DP_E_ARG, w + ": vertices_out must be given");
    for (int k = 0; k < n_views && rc == DP_OK; ++k)
        rc = mesh_check_alias(c, w, {d_vertices_out, d_seen, d_best}, {d_vertices, d_normals, d_depth[k]});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = meshcolour_queue(c, tab, o, d_vertices, n_vertices, d_normals, d_depth, d_vertices_out, d_seen, d_best,
                               s)) != DP_OK)
        return rc;
    return stats ? meshcolour_stats(c, stats, s) : DP_OK;
}

extern "C" int dp_mesh_colour(dp_ctx *c, const dp_mesh_vertex *vertices, int64_t n_vertices, const float *normals,
                              const int32_t *views, int n_views, const dp_mesh_colour_options *mco,
                              const float *const *depth, const dp_mesh_vertex **vertices_out, uint64_t *seen,
                              int32_t *best, dp_mesh_colour_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_mesh_colour";
    dp_mesh_colour_options o;
    dp_default_mesh_colour_options(&o);
    if (mco)
        o = *mco;
    std::vector<dpk::MeshColourView> tab;
    int rc = meshcolour_check(c, w, vertices, n_vertices, views, n_views, o, depth, tab);
    if (rc != DP_OK)
        return rc;
    if (!vertices_out)
        return fail(c, DP_E_ARG, w + ": vertices_out must be given");
    for (int k = 0; k < n_views && rc == DP_OK; ++k)
        rc = mesh_check_alias(c, w, {seen, best}, {vertices, normals, depth[k]});
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::MeshColourScratch &r = c->meshcolour;
    const int64_t nv = n_vertices;
    // staged inputs, 256-B aligned, in one buffer: the vertices (16 B each), the
    // normals, the depth planes; the results in another: vertices, seen, best
    const size_t vbytes = sizeof(dp_mesh_vertex) * (size_t)nv;
    PlanePacker pin, pout;
    const size_t iv = pin.add(vbytes), in = pin.add(normals ? 12 * (size_t)nv : 0);
    std::vector<size_t> id((size_t)n_views);
    for (int k = 0; k < n_views; ++k)
        id[(size_t)k] = pin.add(4 * view_pixels(c, views[k]));
    const size_t ov = pout.add(vbytes), os = pout.add(seen ? 8 * (size_t)nv : 0), ob = pout.add(best ? 4 * (size_t)nv : 0);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hverts.resize((size_t)std::max<int64_t>(nv, 1)));
    if (nv > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + iv, vertices, vbytes, hipMemcpyHostToDevice, s));
    if (nv > 0 && normals)
        DP_HIP(c, hipMemcpyAsync(r.in.p + in, normals, 12 * (size_t)nv, hipMemcpyHostToDevice, s));
    std::vector<const float *> dd((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const size_t bytes = 4 * view_pixels(c, views[k]);
        dd[(size_t)k] = (const float *)(r.in.p + id[(size_t)k]);
        if (bytes)
            DP_HIP(c, hipMemcpyAsync(r.in.p + id[(size_t)k], depth[k], bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = meshcolour_queue(c, tab, o, (const dp_mesh_vertex *)(r.in.p + iv), nv,
                               normals ? (const float *)(r.in.p + in) : nullptr, dd.data(),
                               (dp_mesh_vertex *)(r.out.p + ov), seen ? (uint64_t *)(r.out.p + os) : nullptr,
                               best ? (int32_t *)(r.out.p + ob) : nullptr, s)) != DP_OK)
        return rc;
    if (nv > 0) {
        DP_HIP(c, hipMemcpyAsync(r.hverts.data(), r.out.p + ov, vbytes, hipMemcpyDeviceToHost, s));
        if (seen)
            DP_HIP(c, hipMemcpyAsync(seen, r.out.p + os, 8 * (size_t)nv, hipMemcpyDeviceToHost, s));
        if (best)
            DP_HIP(c, hipMemcpyAsync(best, r.out.p + ob, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
    }
    if (stats) {
        if ((rc = meshcolour_stats(c, stats, s)) != DP_OK)
            return rc;
    } else {
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *vertices_out = nv > 0 ? r.hverts.data() : nullptr;
    return DP_OK;
}
