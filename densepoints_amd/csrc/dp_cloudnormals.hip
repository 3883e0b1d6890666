// dp_cloudnormals.hip -- the gfx950 kernel of the PCA normals and the surface
// variation of a point cloud (spec in include/densepoints.h, dp_cloud_normals),
// and its C ABI.
//
// The neighbourhoods are dp_cloud_knn's own rows of the cloud against itself
// (knn_queue, dp_clouddev.h) in the rows and counts of c->cloudknn, which
// dp_cloud_clean fills the same way: the calls never overlap on a context.
//
//   normals_kernel  one lane per point.  It reads its row of caller indices and
//                   gathers the neighbours with load_point twice: once for the
//                   mean, once for the six sums of the centred scatter (the
//                   second gather finds the lines of the first in the cache;
//                   keeping 32 points in registers instead would cost 96 VGPRs).
//                   The cyclic Jacobi is dp_cloud_align's jacobi_rotate with every
//                   matrix index a template argument, so the 3 x 3 N and V (15
//                   doubles) stay in registers; the sweeps are one rolled loop of
//                   three rotations.  The eigenvector of the smallest diagonal
//                   entry is normalised, given the canonical sign, oriented by
//                   `toward` when asked, and written with the variation: 16 bytes.
//                   The classes and the orientation's outcomes go through the
//                   striped integer counters.
#include "dp_clouddev.h"

#include <algorithm>
#include <cmath>

namespace dpk {
namespace {

// points (taking part), estimated, sparse, degenerate, flipped, unoriented
constexpr int kNormalsCounters = 6;
constexpr int kNormalsStripes = 64;

struct NormalsArgs {
    const char *points;
    int64_t n, stride;
    int32_t k, min_nb;
    int32_t orient; // 0, DP_CLOUD_NORMALS_ORIENT_VIEWPOINT or DP_CLOUD_NORMALS_ORIENT_DIRECTION
    int32_t pad;
    const int32_t *rows, *rowcount;
    const char *toward; // entry i at toward + i * toward_stride (NULL without a flag)
    int64_t toward_stride;
    float *normal;
    float *variation; // optional
    unsigned long long *count; // kNormalsStripes x kNormalsCounters
};

__global__ __launch_bounds__(kMeshLanes) void normals_kernel(NormalsArgs a)
{
    const int64_t i = mesh_item();
    bool part = false, sparse = false, degenerate = false, estimated = false, flipped = false, unoriented = false;
    if (i < a.n) {
        float x[3];
        part = load_point(a.points, a.stride, i, x);
        float out[3] = {0.0f, 0.0f, 0.0f};
        float var = __builtin_huge_valf();
        const int32_t c = part ? a.rowcount[i] : 0;
        sparse = part && c < a.min_nb;
        if (part && !sparse) {
            const int32_t *row = a.rows + i * a.k;
            float p[3];
            double m[3] = {0.0, 0.0, 0.0};
            for (int32_t j = 0; j < c; ++j) {
                load_point(a.points, a.stride, row[j], p);
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    m[r] = j ? m[r] + (double)p[r] : (double)p[r];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
                m[r] = dpg::dvdiv(m[r], (double)c);
            double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
            for (int32_t j = 0; j < c; ++j) {
                load_point(a.points, a.stride, row[j], p);
                const double dx = (double)p[0] - m[0], dy = (double)p[1] - m[1], dz = (double)p[2] - m[2];
                const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
                cxx = j ? cxx + xx : xx;
                cxy = j ? cxy + xy : xy;
                cxz = j ? cxz + xz : xz;
                cyy = j ? cyy + yy : yy;
                cyz = j ? cyz + yz : yz;
                czz = j ? czz + zz : zz;
            }
            const double T = (cxx + cyy) + czz;
            degenerate = T == 0.0;
            estimated = !degenerate;
            if (estimated) {
                double N[3][3], V[3][3];
                N[0][0] = cxx;
                N[1][1] = cyy;
                N[2][2] = czz;
                N[0][1] = N[1][0] = cxy;
                N[0][2] = N[2][0] = cxz;
                N[1][2] = N[2][1] = cyz;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        V[r][k] = r == k ? 1.0 : 0.0;
#pragma unroll 1
                for (int sweep = 0; sweep < DP_CLOUD_NORMALS_SWEEPS; ++sweep) {
                    jacobi_rotate<0, 1>(N, V);
                    jacobi_rotate<0, 2>(N, V);
                    jacobi_rotate<1, 2>(N, V);
                }
                int j = 0;
                double low = N[0][0];
                if (N[1][1] < low) {
                    low = N[1][1];
                    j = 1;
                }
                if (N[2][2] < low) {
                    low = N[2][2];
                    j = 2;
                }
                double v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    v[k] = j == 0 ? V[k][0] : (j == 1 ? V[k][1] : V[k][2]);
                const double len = dpg::dvsqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                double u[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    u[k] = dpg::dvdiv(v[k], len);
                var = (float)dpg::dvdiv(low > 0.0 ? low : 0.0, T); // fmax(low, 0.0), +0.0 for a -0.0
                // the canonical sign: the largest component (the lowest on ties) is positive
                double big = fabs(u[0]), lead = u[0];
                if (fabs(u[1]) > big) {
                    big = fabs(u[1]);
                    lead = u[1];
                }
                if (fabs(u[2]) > big)
                    lead = u[2];
                bool neg = lead < 0.0;
                if (a.orient) {
                    float w[3];
                    const bool wfinite = load_point(a.toward, a.toward_stride, i, w);
                    const double sg = neg ? -1.0 : 1.0;
                    const double ux = sg * u[0], uy = sg * u[1], uz = sg * u[2]; // exact: a sign change
                    double s;
                    if (a.orient == DP_CLOUD_NORMALS_ORIENT_VIEWPOINT)
                        s = (((double)w[0] - (double)x[0]) * ux + ((double)w[1] - (double)x[1]) * uy) +
                            ((double)w[2] - (double)x[2]) * uz;
                    else
                        s = ((double)w[0] * ux + (double)w[1] * uy) + (double)w[2] * uz;
                    if (wfinite && s < 0.0) {
                        neg = !neg;
                        flipped = true;
                    } else if (!wfinite || !(s > 0.0)) {
                        unoriented = true;
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    out[k] = (float)(neg ? -u[k] : u[k]);
            }
        }
        float *o = a.normal + 3 * i;
        o[0] = out[0];
        o[1] = out[1];
        o[2] = out[2];
        if (a.variation)
            a.variation[i] = var;
    }
    const uint32_t stripe = wave_stripe();
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 0, part ? 1ull : 0ull, stripe);
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 1, estimated ? 1ull : 0ull, stripe);
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 2, sparse ? 1ull : 0ull, stripe);
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 3, degenerate ? 1ull : 0ull, stripe);
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 4, flipped ? 1ull : 0ull, stripe);
    wave_count<kNormalsStripes, kNormalsCounters>(a.count, 5, unoriented ? 1ull : 0ull, stripe);
}

} // namespace
} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI: dp_cloud_normals
// ---------------------------------------------------------------------------

static int normals_check(dp_ctx *c, const std::string &w, const void *points, int64_t n, int64_t stride,
                         const dp_cloud_normals_options *o, const void *toward, int64_t toward_stride)
{
    if (n < 0 || n > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": n must be in 0..2^31 - 1");
    if (n > 0 && !points)
        return fail(c, DP_E_ARG, w + ": points must be given");
    if (stride < 12 || stride % 4)
        return fail(c, DP_E_ARG, w + ": stride must be a multiple of 4 and at least 12");
    if (!o)
        return fail(c, DP_E_ARG, w + ": opts must be given");
    if (!(o->max_dist > 0.0f) || !std::isfinite(o->max_dist))
        return fail(c, DP_E_ARG, w + ": max_dist must be finite and > 0");
    if (o->k < 3 || o->k > 32)
        return fail(c, DP_E_ARG, w + ": k must be in 3..32");
    if (o->min_neighbours < 3 || o->min_neighbours > o->k)
        return fail(c, DP_E_ARG, w + ": min_neighbours must be in 3..k");
    if (o->flags != 0 && o->flags != DP_CLOUD_NORMALS_ORIENT_VIEWPOINT &&
        o->flags != DP_CLOUD_NORMALS_ORIENT_DIRECTION)
        return fail(c, DP_E_ARG, w + ": flags must be 0 or one of the two ORIENT flags");
    if (o->flags) {
        if (!toward)
            return fail(c, DP_E_ARG, w + ": an ORIENT flag needs toward");
        if (toward_stride != 0 && (toward_stride < 12 || toward_stride % 4))
            return fail(c, DP_E_ARG, w + ": toward_stride must be 0 or a multiple of 4 and at least 12");
    } else if (toward || toward_stride != 0) {
        return fail(c, DP_E_ARG, w + ": toward and toward_stride must be NULL and 0 without an ORIENT flag");
    }
    return DP_OK;
}

// an output may be neither an input nor another output
static int normals_check_alias(dp_ctx *c, const std::string &w, const void *points, const void *toward,
                               const void *normal, const void *variation, const void *count)
{
    const void *o[3] = {normal, variation, count};
    for (int i = 0; i < 3; ++i) {
        if (!o[i])
            continue;
        if (o[i] == points || o[i] == toward)
            return fail(c, DP_E_ARG, w + ": an output pointer equals an input pointer");
        for (int j = 0; j < i; ++j)
            if (o[i] == o[j])
                return fail(c, DP_E_ARG, w + ": two output pointers are equal");
    }
    return DP_OK;
}

// queues the search and the estimate of a device cloud on s
static int normals_queue(dp_ctx *c, const dp_cloud_normals_options &o, const void *d_points, int64_t n, int64_t stride,
                         const void *d_toward, int64_t toward_stride, float *d_normal, float *d_variation,
                         int32_t *d_count, hipStream_t s)
{
    dpk::CloudKnnScratch &r = c->cloudknn;
    dpk::CloudNormalsScratch &m = c->cloudnormals;
    DP_HIP(c, r.rows.reserve(std::max<size_t>((size_t)n * (size_t)o.k, 1)));
    DP_HIP(c, r.rowcount.reserve((size_t)n + 1));
    DP_HIP(c, m.count.reserve(dpk::kNormalsStripes, dpk::kNormalsCounters, (sizeof(dpk::CloudGrid) + 7) / 8));

    // the counts are the search's own output: into the caller's buffer when it wants them
    int32_t *rowcount = d_count ? d_count : r.rowcount.p;
    DP_HIP(c, m.time[0].begin(s));
    dp_cloud_knn_options ko{o.max_dist, o.k, 0};
    const int rc = knn_queue(c, ko, d_points, n, stride, d_points, n, stride, r.rows.p, nullptr, rowcount, s);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, m.time[0].end(s));

    dpk::NormalsArgs a{};
    a.points = (const char *)d_points;
    a.n = n;
    a.stride = stride;
    a.k = o.k;
    a.min_nb = o.min_neighbours;
    a.orient = o.flags;
    a.rows = r.rows.p;
    a.rowcount = rowcount;
    a.toward = (const char *)d_toward;
    a.toward_stride = toward_stride;
    a.normal = d_normal;
    a.variation = d_variation;
    a.count = m.count.dev.p;
    DP_HIP(c, m.time[1].begin(s));
    DP_HIP(c, m.count.zero(s));
    DP_HIP(c, dpk::launch_over(dpk::normals_kernel, dpk::mesh_blocks(n), a, s));
    DP_HIP(c, m.time[1].end(s));
    return DP_OK;
}

// the statistics read and its wait
static int normals_stats(dp_ctx *c, int64_t n, dp_cloud_normals_stats *stats, hipStream_t s)
{
    dpk::CloudNormalsScratch &m = c->cloudnormals;
    DP_HIP(c, m.count.read(s));
    DP_HIP(c, hipMemcpyAsync(m.count.extra(), c->cloudnearest.grid.p, sizeof(dpk::CloudGrid), hipMemcpyDeviceToHost, s));
    DP_HIP(c, hipStreamSynchronize(s));
    const dpk::CloudGrid *g = (const dpk::CloudGrid *)m.count.extra();
    stats->points = m.count.sum(0);
    stats->skipped = n - stats->points;
    stats->estimated = m.count.sum(1);
    stats->sparse = m.count.sum(2);
    stats->degenerate = m.count.sum(3);
    stats->flipped = m.count.sum(4);
    stats->unoriented = m.count.sum(5);
    stats->grid_cells = g->cells;
    stats->max_cell_targets = g->maxcell;
    DP_HIP(c, m.time[0].ms(stats->knn_ms));
    DP_HIP(c, m.time[1].ms(stats->normals_ms));
    return DP_OK;
}

extern "C" int dp_cloud_normals_device(dp_ctx *c, const void *d_points, int64_t n, int64_t stride,
                                       const dp_cloud_normals_options *opts, const void *d_toward,
                                       int64_t toward_stride, float *d_normal, float *d_variation, int32_t *d_count,
                                       dp_cloud_normals_stats *stats, void *stream)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_normals_device";
    int rc = normals_check(c, w, d_points, n, stride, opts, d_toward, toward_stride);
    if (rc != DP_OK)
        return rc;
    if (n > 0 && !d_normal)
        return fail(c, DP_E_ARG, w + ": d_normal must be given");
    if ((rc = normals_check_alias(c, w, d_points, d_toward, d_normal, d_variation, d_count)) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = normals_queue(c, *opts, d_points, n, stride, d_toward, toward_stride, d_normal, d_variation, d_count,
                            s)) != DP_OK)
        return rc;
    return stats ? normals_stats(c, n, stats, s) : DP_OK;
}

extern "C" int dp_cloud_normals(dp_ctx *c, const void *points, int64_t n, int64_t stride,
                                const dp_cloud_normals_options *opts, const void *toward, int64_t toward_stride,
                                const float **normal, const float **variation, const int32_t **count,
                                dp_cloud_normals_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    const std::string w = "dp_cloud_normals";
    int rc = normals_check(c, w, points, n, stride, opts, toward, toward_stride);
    if (rc != DP_OK)
        return rc;
    if (!normal)
        return fail(c, DP_E_ARG, w + ": normal must be given");
    if ((rc = normals_check_alias(c, w, points, toward, normal, variation, count)) != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    dpk::CloudKnnScratch &r = c->cloudknn;
    // the records are staged from the first point to the end of the last; toward
    // entries that start inside them are read from the staged copy (which then
    // reaches to the end of the last entry), others are staged behind it
    const size_t pbytes = n > 0 ? (size_t)(n - 1) * (size_t)stride + 12 : 0;
    const size_t tbytes = toward && n > 0 ? (size_t)(n - 1) * (size_t)toward_stride + 12 : 0;
    const char *pb = (const char *)points, *tb = (const char *)toward;
    const bool inside = tbytes && tb >= pb && tb < pb + pbytes;
    const size_t rbytes = inside ? std::max(pbytes, (size_t)(tb - pb) + tbytes) : pbytes;
    PlanePacker pin, pout;
    const size_t ip = pin.add(rbytes), it = pin.add(inside ? 0 : tbytes);
    const size_t on = pout.add(12 * (size_t)n), ov = pout.add(variation ? 4 * (size_t)n : 0),
                 oc = pout.add(count ? 4 * (size_t)n : 0);
    DP_HIP(c, r.in.reserve(std::max<size_t>(pin.total, 1)));
    DP_HIP(c, r.out.reserve(std::max<size_t>(pout.total, 1)));
    DP_HIP(c, r.hout.resize(std::max<size_t>(pout.total, 1)));
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.in.p + ip, points, rbytes, hipMemcpyHostToDevice, s));
    if (tbytes && !inside)
        DP_HIP(c, hipMemcpyAsync(r.in.p + it, toward, tbytes, hipMemcpyHostToDevice, s));
    const void *d_toward = !tbytes ? nullptr : (inside ? r.in.p + ip + (tb - pb) : r.in.p + it);
    if ((rc = normals_queue(c, *opts, r.in.p + ip, n, stride, d_toward, toward_stride, (float *)(r.out.p + on),
                            variation ? (float *)(r.out.p + ov) : nullptr, count ? (int32_t *)(r.out.p + oc) : nullptr,
                            s)) != DP_OK)
        return rc;
    if (n > 0)
        DP_HIP(c, hipMemcpyAsync(r.hout.data(), r.out.p, pout.total, hipMemcpyDeviceToHost, s));
    if (stats) {
        if ((rc = normals_stats(c, n, stats, s)) != DP_OK)
            return rc;
    } else {
        DP_HIP(c, hipStreamSynchronize(s));
    }
    *normal = n > 0 ? (const float *)(r.hout.data() + on) : nullptr;
    if (variation)
        *variation = n > 0 ? (const float *)(r.hout.data() + ov) : nullptr;
    if (count)
        *count = n > 0 ? (const int32_t *)(r.hout.data() + oc) : nullptr;
    return DP_OK;
}
