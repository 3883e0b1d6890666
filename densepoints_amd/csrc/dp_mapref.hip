// dp_mapref.hip -- depth-map refinement (spec in include/densepoints.h,
// dp_refine_maps): every pixel of the requested views scores a short list of
// candidate planes (its own, a depth sweep of it, its neighbours') against a few
// source views through the performance mode's sampler and keeps the best.
//
//   mapref_kernel<WIN>  one lane per pixel; a 256-thread block owns a 16 x 16
//                       tile of one view (blockIdx.y = the view's rank), so a
//                       wave is a 16 x 4 strip and neighbouring lanes gather
//                       neighbouring source texels.  The block stages 16 x the
//                       reference grays of its tile plus the window apron in LDS
//                       once; the reference moments are per pixel, not per
//                       candidate.  The candidate and source loops are
//                       wave-uniform with per-lane void flags: the source's
//                       table row is read with scalar loads, a candidate or a
//                       source that no lane of the wave can use is skipped, and a
//                       wave without any plane runs neither loop.  Per (candidate,
//                       source) the fp64 set-up runs once; per sample two fmaf
//                       pairs, the 2^23 add, the clamp and two 4-byte gathers
//                       (the tap pair of each row); all gathers of a window row
//                       are issued before any is blended.  The top-k scores live
//                       in fixed, fully unrolled registers.
//
// The kernel reads the input planes and writes the output planes only, so its
// result is a function of the planes alone.  Neighbour planes (the reach
// offsets) are read from global memory: eight pixels per lane, against
// thousands of gathers.
#include "dp_fast.h"
#include "dp_mapdev.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace dpk {
namespace {

// the input pixel (px, py) of view r: true iff it is inside the image and has
// a plane (z a depth, dot(n, n) > 0)
__device__ __forceinline__ bool load_plane(const MaprefView &r, int px, int py, float &z, float *n)
{
    if (px < 0 || py < 0 || px >= r.W || py >= r.H)
        return false;
    const int64_t i = (int64_t)py * r.W + px;
    z = r.depth[i];
    if (!is_depth(z))
        return false;
    n[0] = r.normal[3 * i];
    n[1] = r.normal[3 * i + 1];
    n[2] = r.normal[3 * i + 2];
    const double d[3] = {(double)n[0], (double)n[1], (double)n[2]};
    return dpg::dot3(d, d) > 0.0;
}

// the (x, x + 1) tap pair of a gray row: two u16, the low one first
__device__ __forceinline__ uint32_t load_pair(const uint16_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

template <int WIN> __global__ __launch_bounds__(256) void mapref_kernel(MaprefArgs a)
{
    constexpr int HW = (WIN - 1) / 2, TS = 16 + 2 * HW, N = WIN * WIN;
    __shared__ uint16_t tile[TS * TS];
    const int k = blockIdx.y;
    const MaprefView &r = a.tab[k];
    const double *rP = r.inv.P;
    const int tiles_x = (r.W + 15) >> 4;
    if ((int)blockIdx.x >= tiles_x * ((r.H + 15) >> 4))
        return;
    const int tx0 = ((int)blockIdx.x % tiles_x) << 4, ty0 = ((int)blockIdx.x / tiles_x) << 4;
    for (int t = threadIdx.x; t < TS * TS; t += 256) {
        const int yy = min(max(ty0 - HW + t / TS, 0), r.H - 1), xx = min(max(tx0 - HW + t % TS, 0), r.W - 1);
        tile[t] = (uint16_t)((r.gray[(int64_t)yy * r.gpitch + xx] & 0xFFu) << 4);
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = tx0 + lx, y = ty0 + ly;
    const bool in = x < r.W && y < r.H;
    const int64_t at = in ? (int64_t)y * r.W + x : 0;
    const uint16_t *tw = tile + ly * TS + lx; // the window's top-left sample

    // the pixel's own plane and which of its neighbours have one
    float z = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    uint32_t vmask = 0;
    bool own_depth = false;
    if (in) {
        own_depth = is_depth(r.depth[at]);
        if (load_plane(r, x, y, z, n))
            vmask |= 1u;
        for (int e = 0; e < 4 * a.nreach; ++e) {
            const int d = a.reach[e >> 2];
            float zz, nn[3];
            if (load_plane(r, x + ((e & 2) ? 0 : (e & 1) ? d : -d), y + ((e & 2) ? ((e & 1) ? d : -d) : 0), zz, nn))
                vmask |= 2u << e;
        }
    }

    double best = 0.0;
    int choice = -1;
    float wz = 0.0f, wn[3] = {0.0f, 0.0f, 0.0f};
    uint32_t ncand = 0, nscored = 0;
    if (__any(vmask != 0)) {
        // the reference moments: the same window for every candidate
        uint32_t Sa = 0, Saa = 0;
        for (int j = 0; j < WIN; ++j)
#pragma unroll
            for (int i = 0; i < WIN; ++i) {
                const uint32_t v = tw[j * TS + i];
                Sa += v;
                Saa += v * v;
            }
        const double va = (double)N * (double)Saa - (double)Sa * (double)Sa;
        // the own point, its ray and its pixel footprint (the sweep's step)
        const double xd = (double)x, yd = (double)y;
        double Xo[3] = {0.0, 0.0, 0.0}, ray[3] = {0.0, 0.0, 0.0}, dx = 0.0, len = 0.0;
        if (vmask & 1u) {
            backproject(r.inv, xd, yd, (double)z, Xo);
            if (a.sweep > 0) {
                const double d0 = row_of(rP, 2, Xo);
                const double cu = row_of(rP, 0, Xo) / d0, cv = row_of(rP, 1, Xo) / d0;
                const double Xq[3] = {Xo[0] + r.xr[0], Xo[1] + r.xr[1], Xo[2] + r.xr[2]};
                const double d1 = row_of(rP, 2, Xq);
                const double du = row_of(rP, 0, Xq) / d1 - cu, dv = row_of(rP, 1, Xq) / d1 - cv;
                dx = sqrt(du * du + dv * dv);
                for (int j = 0; j < 3; ++j)
                    ray[j] = Xo[j] - r.C[j];
                len = sqrt(dpg::dot3(ray, ray));
            }
        }
        const int ncands = 1 + 2 * a.sweep + 4 * a.nreach;
        for (int ci = 0; ci < ncands; ++ci) {
            bool live;
            double X0[3] = {Xo[0], Xo[1], Xo[2]};
            float cn[3] = {n[0], n[1], n[2]};
            if (ci <= 2 * a.sweep) {
                live = vmask & 1u;
                if (ci > 0) {
                    const int h = ci <= a.sweep ? ci - 1 - a.sweep : ci - a.sweep;
                    live = live && dx > 0.0 && len > 0.0;
                    const double t = ((double)h * a.step) / dx;
                    for (int j = 0; j < 3; ++j)
                        X0[j] = Xo[j] + (t * ray[j]) / len;
                }
            } else {
                const int e = ci - 1 - 2 * a.sweep, d = a.reach[e >> 2];
                const int px = x + ((e & 2) ? 0 : (e & 1) ? d : -d), py = y + ((e & 2) ? ((e & 1) ? d : -d) : 0);
                live = (vmask >> (1 + e)) & 1u;
                float zz = 0.0f;
                if (live) {
                    load_plane(r, px, py, zz, cn);
                    backproject(r.inv, (double)px, (double)py, (double)zz, X0);
                }
            }
            if (!__any(live))
                continue;
            // the plane as seen from r, its depth at the pixel and the two next to it
            const double nd[3] = {(double)cn[0], (double)cn[1], (double)cn[2]};
            double m[3];
            for (int j = 0; j < 3; ++j)
                m[j] = (r.inv.A[j] * nd[0] + r.inv.A[3 + j] * nd[1]) + r.inv.A[6 + j] * nd[2];
            const double p4[3] = {rP[3], rP[7], rP[11]};
            const double c = r.inv.det * dpg::dot3(nd, X0) + dpg::dot3(m, p4);
            const double zc = c / ((m[0] * xd + m[1] * yd) + m[2]);
            const float zf = (float)zc;
            live = live && is_depth(zf);
            if (!__any(live))
                continue;
            const double zi = c / ((m[0] * (xd + 1.0) + m[1] * yd) + m[2]);
            const double zj = c / ((m[0] * xd + m[1] * (yd + 1.0)) + m[2]);
            double Xc[3], Xi[3], Xj[3];
            backproject(r.inv, xd, yd, zc, Xc);
            backproject(r.inv, xd + 1.0, yd, zi, Xi);
            backproject(r.inv, xd, yd + 1.0, zj, Xj);

            // the valid sources' scores, sorted descending in fixed registers
            double top[kMaprefMaxSources];
#pragma unroll
            for (int t = 0; t < kMaprefMaxSources; ++t)
                top[t] = -INFINITY;
            int nvalid = 0;
            for (int si = 0; si < r.nsrc; ++si) {
                const MaprefView &s = a.tab[r.src[si]];
                float U0 = 0.0f, V0 = 0.0f, Ui = 0.0f, Vi = 0.0f, Uj = 0.0f, Vj = 0.0f;
                bool ok = live;
                if (ok) {
                    const double dc = row_of(s.inv.P, 2, Xc), di = row_of(s.inv.P, 2, Xi), dj = row_of(s.inv.P, 2, Xj);
                    ok = dc > 0.0 && di > 0.0 && dj > 0.0;
                    if (ok) {
                        const double uc = row_of(s.inv.P, 0, Xc) / dc, vc = row_of(s.inv.P, 1, Xc) / dc;
                        const double ui = row_of(s.inv.P, 0, Xi) / di, vi = row_of(s.inv.P, 1, Xi) / di;
                        const double uj = row_of(s.inv.P, 0, Xj) / dj, vj = row_of(s.inv.P, 1, Xj) / dj;
                        U0 = (float)(32.0 * uc);
                        V0 = (float)(32.0 * vc);
                        Ui = (float)(32.0 * (ui - uc));
                        Vi = (float)(32.0 * (vi - vc));
                        Uj = (float)(32.0 * (uj - uc));
                        Vj = (float)(32.0 * (vj - vc));
                        const double umax = 32.0 * (double)(s.W - 1), vmax = 32.0 * (double)(s.H - 1);
                        for (int q = 0; q < 4; ++q) {
                            const double ci2 = (q & 1) ? (double)HW : -(double)HW;
                            const double cj2 = (q & 2) ? (double)HW : -(double)HW;
                            const double ca = ((double)U0 + ci2 * (double)Ui) + cj2 * (double)Uj;
                            const double cb = ((double)V0 + ci2 * (double)Vi) + cj2 * (double)Vj;
                            ok = ok && ca >= 0.0 && ca <= umax && cb >= 0.0 && cb <= vmax;
                        }
                    }
                }
                if (!__any(ok))
                    continue;
                if (!ok) // a lane that sits the source out samples texel (0, 0)
                    U0 = V0 = Ui = Vi = Uj = Vj = 0.0f;
                const float ulim = 8388608.0f + (float)(32 * (s.W - 1)), vlim = 8388608.0f + (float)(32 * (s.H - 1));
                const uint16_t *g = s.gray;
                const int gp = s.gpitch, hmax = s.H - 1;
                uint32_t Sb = 0, Sbb = 0, Sab = 0;
#pragma unroll 1
                for (int j = 0; j < WIN; ++j) {
                    const float tj = (float)(j - HW);
                    uint32_t r0[WIN], r1[WIN], fr[WIN];
#pragma unroll
                    for (int i = 0; i < WIN; ++i) {
                        const float ti = (float)(i - HW);
                        float U = __builtin_fmaf(tj, Uj, __builtin_fmaf(ti, Ui, U0)) + 8388608.0f;
                        float V = __builtin_fmaf(tj, Vj, __builtin_fmaf(ti, Vi, V0)) + 8388608.0f;
                        U = fminf(fmaxf(U, 8388608.0f), ulim);
                        V = fminf(fmaxf(V, 8388608.0f), vlim);
                        const int iu = (int)(U - 8388608.0f), iv = (int)(V - 8388608.0f);
                        const int xs = iu >> 5, yv = iv >> 5;
                        fr[i] = (uint32_t)(iu & 31) | ((uint32_t)(iv & 31) << 8);
                        r0[i] = load_pair(g + ((int64_t)yv * gp + xs));
                        r1[i] = load_pair(g + ((int64_t)min(yv + 1, hmax) * gp + xs));
                    }
#pragma unroll
                    for (int i = 0; i < WIN; ++i) {
                        const uint32_t fx = fr[i] & 31u, fy = fr[i] >> 8;
                        const uint32_t p00 = r0[i] & 0xFFu, p01 = (r0[i] >> 16) & 0xFFu;
                        const uint32_t p10 = r1[i] & 0xFFu, p11 = (r1[i] >> 16) & 0xFFu;
                        const uint32_t b = ((32u - fx) * ((32u - fy) * p00 + fy * p10) +
                                            fx * ((32u - fy) * p01 + fy * p11) + 32u) >> 6;
                        const uint32_t av = tw[j * TS + i];
                        Sb += b;
                        Sbb += b * b;
                        Sab += av * b;
                    }
                }
                if (ok) {
                    const double num = (double)N * (double)Sab - (double)Sa * (double)Sb;
                    const double vb = (double)N * (double)Sbb - (double)Sb * (double)Sb;
                    const double den = sqrt(va * vb);
                    double v = num / (den > a.dmin ? den : a.dmin);
                    ++nvalid;
                    ++nscored;
#pragma unroll
                    for (int t = 0; t < kMaprefMaxSources; ++t)
                        if (v > top[t]) {
                            const double o = top[t];
                            top[t] = v;
                            v = o;
                        }
                }
            }
            if (live && nvalid >= a.top_k) {
                double S = top[0];
#pragma unroll
                for (int t = 1; t < kMaprefMaxSources; ++t)
                    if (t < a.top_k)
                        S = S + top[t];
                const double score = S / (double)a.top_k;
                ++ncand;
                if (choice < 0 || score > best) {
                    best = score;
                    choice = ci;
                    wz = zf;
                    wn[0] = cn[0], wn[1] = cn[1], wn[2] = cn[2];
                }
            }
        }
    }

    const bool scored = choice >= 0;
    const bool kept = scored && best >= a.min_ncc;
    float oz = 0.0f, on[3] = {0.0f, 0.0f, 0.0f}, os = 0.0f;
    int oc = -1;
    if (kept) {
        oz = wz;
        on[0] = wn[0], on[1] = wn[1], on[2] = wn[2];
        os = (float)best;
        oc = choice;
    } else if (!scored && own_depth && a.keep_unscored) {
        oz = r.depth[at];
        on[0] = r.normal[3 * at], on[1] = r.normal[3 * at + 1], on[2] = r.normal[3 * at + 2];
        oc = -2;
    }
    if (in) {
        if (r.odepth)
            r.odepth[at] = oz;
        if (r.onormal) {
            r.onormal[3 * at] = on[0];
            r.onormal[3 * at + 1] = on[1];
            r.onormal[3 * at + 2] = on[2];
        }
        if (r.oscore)
            r.oscore[at] = os;
        if (r.ochoice)
            r.ochoice[at] = oc;
    }
    const uint32_t stripe = blockIdx.x * 4u + (threadIdx.x >> 6);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 0, own_depth ? 1ull : 0ull, stripe);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 1, (unsigned long long)ncand, stripe);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 2, (unsigned long long)nscored, stripe);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 3, kept ? 1ull : 0ull, stripe);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 4, kept && !own_depth ? 1ull : 0ull, stripe);
    wave_count<kMaprefStripes, kMaprefCounters>(a.count, 5, kept && choice != 0 ? 1ull : 0ull, stripe);
}

} // namespace

hipError_t launch_mapref(const MaprefArgs &a, unsigned gx, hipStream_t s)
{
    const dim3 grid(gx, (unsigned)a.K), block(256);
    switch (a.window) {
    case 3: hipLaunchKernelGGL(mapref_kernel<3>, grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL(mapref_kernel<5>, grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL(mapref_kernel<7>, grid, block, 0, s, a); break;
    case 9: hipLaunchKernelGGL(mapref_kernel<9>, grid, block, 0, s, a); break;
    case 11: hipLaunchKernelGGL(mapref_kernel<11>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace dpk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void dp_default_mapref_options(dp_mapref_options *mo)
{
    if (!mo)
        return;
    mo->window = 7;
    mo->sweep = 2;
    mo->step_px = 1.0f;
    mo->reach[0] = 1;
    mo->reach[1] = 4;
    mo->max_sources = 4;
    mo->top_k = 2;
    mo->min_ncc = 0.5f;
    mo->flags = 0;
}

// argument checks shared by both forms (they need no device)
static int mapref_check(dp_ctx *c, const int32_t *views, int n_views, const dp_mapref_options &o,
                        const int32_t *sources, const float *const *depth, const float *const *normal,
                        float *const *od, float *const *on, float *const *os, int32_t *const *oc)
{
    if (!c)
        return DP_E_ARG;
    if (o.window < 3 || o.window > 11 || !(o.window & 1))
        return fail(c, DP_E_ARG, "dp_refine_maps: window must be odd and in 3..11");
    if (o.sweep < 0 || o.sweep > 8)
        return fail(c, DP_E_ARG, "dp_refine_maps: sweep must be in 0..8");
    if (!(o.step_px > 0.0f) || !std::isfinite(o.step_px))
        return fail(c, DP_E_ARG, "dp_refine_maps: step_px must be finite and > 0");
    for (int i = 0; i < 2; ++i)
        if (o.reach[i] < 0 || o.reach[i] > 16)
            return fail(c, DP_E_ARG, "dp_refine_maps: a reach must be in 0..16");
    if (o.max_sources < 1 || o.max_sources > dpk::kMaprefMaxSources)
        return fail(c, DP_E_ARG, "dp_refine_maps: max_sources must be in 1..8");
    if (o.top_k < 1 || o.top_k > o.max_sources)
        return fail(c, DP_E_ARG, "dp_refine_maps: top_k must be in 1..max_sources");
    if (!(o.min_ncc >= -1.0f && o.min_ncc <= 1.0f))
        return fail(c, DP_E_ARG, "dp_refine_maps: min_ncc must be in -1..1");
    if (o.flags & ~DP_MAPREF_KEEP_UNSCORED)
        return fail(c, DP_E_ARG, "dp_refine_maps: unknown flag bits");
    const int rc = check_view_list(c, "dp_refine_maps", views, n_views, 64);
    if (rc != DP_OK)
        return rc;
    uint64_t seen[2] = {0, 0}; // the requested views, for the sources' rows
    for (int k = 0; k < n_views; ++k)
        seen[views[k] >> 6] |= 1ull << (views[k] & 63);
    if (sources)
        for (int k = 0; k < n_views; ++k) {
            uint64_t row[2] = {0, 0};
            bool ended = false;
            for (int j = 0; j < o.max_sources; ++j) {
                const int32_t v = sources[(size_t)k * o.max_sources + j];
                if (v == -1) {
                    ended = true;
                    continue;
                }
                if (ended || v < 0 || v >= c->V || v == views[k] || !((seen[v >> 6] >> (v & 63)) & 1ull) ||
                    ((row[v >> 6] >> (v & 63)) & 1ull))
                    return fail(c, DP_E_ARG, "dp_refine_maps: a sources row must hold requested views other than "
                                             "its own, without repeats, -1 padded at the end");
                row[v >> 6] |= 1ull << (v & 63);
            }
        }
    if (!depth || !normal)
        return fail(c, DP_E_ARG, "dp_refine_maps: depth and normal planes must be given");
    for (int k = 0; k < n_views; ++k)
        if (!depth[k] || !normal[k])
            return fail(c, DP_E_ARG, "dp_refine_maps: a plane pointer is NULL");
    for (int k = 0; k < n_views; ++k) {
        const void *outs[4] = {od ? od[k] : nullptr, on ? on[k] : nullptr, os ? os[k] : nullptr, oc ? oc[k] : nullptr};
        for (const void *p : outs)
            for (int j = 0; p && j < n_views; ++j)
                if (p == depth[j] || p == normal[j])
                    return fail(c, DP_E_ARG, "dp_refine_maps: an output plane is an input plane");
    }
    return DP_OK;
}

extern "C" int dp_refine_maps_device(dp_ctx *c, const int32_t *views, int n_views, const dp_mapref_options *mo,
                                     const int32_t *sources, const float *const *d_depth,
                                     const float *const *d_normal, float *const *d_depth_out,
                                     float *const *d_normal_out, float *const *d_score_out,
                                     int32_t *const *d_choice_out, dp_mapref_stats *stats, void *stream)
{
    dp_mapref_options o;
    dp_default_mapref_options(&o);
    if (mo)
        o = *mo;
    int rc = mapref_check(c, views, n_views, o, sources, d_depth, d_normal, d_depth_out, d_normal_out, d_score_out,
                          d_choice_out);
    if (rc != DP_OK)
        return rc;
    int rank[DP_MAX_VIEWS];
    for (int v = 0; v < DP_MAX_VIEWS; ++v)
        rank[v] = -1;
    for (int k = 0; k < n_views; ++k)
        rank[views[k]] = k;
    std::vector<dpk::MaprefView> tab((size_t)n_views);
    int64_t max_tiles = 1;
    for (int k = 0; k < n_views; ++k) {
        dpk::MaprefView &t = tab[(size_t)k];
        const dpg::ViewDev &v = c->hv[views[k]];
        if (!view_inverse(v, t.inv))
            return fail(c, DP_E_ARG, "dp_refine_maps: a requested view's left 3x3 is singular");
        for (int j = 0; j < 3; ++j) {
            t.C[j] = v.C[j];
            t.xr[j] = v.xr[j];
        }
        t.depth = d_depth[k];
        t.normal = d_normal[k];
        t.odepth = d_depth_out ? d_depth_out[k] : nullptr;
        t.onormal = d_normal_out ? d_normal_out[k] : nullptr;
        t.oscore = d_score_out ? d_score_out[k] : nullptr;
        t.ochoice = d_choice_out ? d_choice_out[k] : nullptr;
        t.W = v.W;
        t.H = v.H;
        if ((int64_t)v.W * v.H > 0x7FFFFFFFll)
            return fail(c, DP_E_ARG, "dp_refine_maps: view too large");
        max_tiles = std::max<int64_t>(max_tiles, (int64_t)((v.W + 15) >> 4) * ((v.H + 15) >> 4));
        t.nsrc = 0;
        for (int j = 0; j < dpk::kMaprefMaxSources; ++j)
            t.src[j] = 0;
        if (sources) {
            for (int j = 0; j < o.max_sources; ++j) {
                const int32_t sv = sources[(size_t)k * o.max_sources + j];
                if (sv >= 0)
                    t.src[t.nsrc++] = rank[sv];
            }
        } else {
            // the other requested views by ascending squared centre distance, ties to the lower id
            std::vector<std::pair<double, int32_t>> near;
            for (int kp = 0; kp < n_views; ++kp) {
                if (kp == k)
                    continue;
                const double *Cs = c->hv[views[kp]].C;
                const double e[3] = {Cs[0] - v.C[0], Cs[1] - v.C[1], Cs[2] - v.C[2]};
                near.emplace_back(dpg::dot3(e, e), views[kp]);
            }
            std::sort(near.begin(), near.end());
            for (size_t j = 0; j < near.size() && (int)j < o.max_sources; ++j)
                t.src[t.nsrc++] = rank[near[j].second];
        }
    }
    std::vector<dpk::GrayPlane> gray;
    rc = dp_gray_planes(c, gray);
    if (rc != DP_OK)
        return rc;
    for (int k = 0; k < n_views; ++k) {
        tab[(size_t)k].gray = (const uint16_t *)gray[(size_t)views[k]].p;
        tab[(size_t)k].gpitch = gray[(size_t)views[k]].pitch;
    }
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    StripedCounters &n = c->mapref.count;
    DP_HIP(c, c->mapref.tab.reserve((size_t)n_views));
    DP_HIP(c, n.reserve(dpk::kMaprefStripes, dpk::kMaprefCounters));

    dpk::MaprefArgs a{};
    a.tab = c->mapref.tab.p;
    a.K = n_views;
    a.window = o.window;
    a.sweep = o.sweep;
    a.nreach = 0;
    for (int i = 0; i < 2; ++i)
        if (o.reach[i] > 0)
            a.reach[a.nreach++] = o.reach[i];
    a.top_k = o.top_k;
    a.keep_unscored = (o.flags & DP_MAPREF_KEEP_UNSCORED) ? 1 : 0;
    a.step = (double)o.step_px;
    a.min_ncc = (double)o.min_ncc;
    {
        const double N = (double)(o.window * o.window);
        a.dmin = ((c->opt.ncc_denom_min * 256.0) * N) * N;
    }
    a.count = n.dev.p;

    // A pageable source: hip_runtime_api.h on hipMemcpyAsync, "If host or dst are not pinned, the memory
    // copy will be performed synchronously" -- the table is read before the call returns and may be freed then.
    // The runtime stages so small a copy without waiting for the stream: a call made behind 120 ms of
    // pending work returns in 0.1 ms, and two calls queued back to back each see their own table
    // (tests/test_gpu_caller_stream.py).
    DP_HIP(c, hipMemcpyAsync(c->mapref.tab.p, tab.data(), sizeof(dpk::MaprefView) * tab.size(), hipMemcpyHostToDevice, s));
    DP_HIP(c, n.zero(s));
    DP_HIP(c, c->mapref.time.begin(s));
    DP_HIP(c, dpk::launch_mapref(a, (unsigned)max_tiles, s));
    DP_HIP(c, c->mapref.time.end(s));
    if (!stats)
        return DP_OK;
    // the one wait: the counters
    DP_HIP(c, n.read(s));
    DP_HIP(c, hipStreamSynchronize(s));
    stats->depth_pixels_in = n.sum(0);
    stats->candidates = n.sum(1);
    stats->source_scores = n.sum(2);
    stats->kept = n.sum(3);
    stats->filled = n.sum(4);
    stats->moved = n.sum(5);
    DP_HIP(c, c->mapref.time.ms(stats->refine_ms));
    return DP_OK;
}

extern "C" int dp_refine_maps(dp_ctx *c, const int32_t *views, int n_views, const dp_mapref_options *mo,
                              const int32_t *sources, const float *const *depth, const float *const *normal,
                              float *const *depth_out, float *const *normal_out, float *const *score_out,
                              int32_t *const *choice_out, dp_mapref_stats *stats)
{
    dp_mapref_options o;
    dp_default_mapref_options(&o);
    if (mo)
        o = *mo;
    int rc = mapref_check(c, views, n_views, o, sources, depth, normal, depth_out, normal_out, score_out, choice_out);
    if (rc != DP_OK)
        return rc;
    hipSetDevice(c->device);
    hipStream_t s = c->stream;
    // device copies of the input planes and the wanted output planes, 256-B
    // aligned, in one buffer: per view depth, normal, then depth, normal, score,
    // choice out
    const size_t words[6] = {1, 3, 1, 3, 1, 1};
    std::vector<size_t> off((size_t)n_views * 6);
    PlanePacker pack;
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        const bool want[6] = {true, true, depth_out && depth_out[k], normal_out && normal_out[k],
                              score_out && score_out[k], choice_out && choice_out[k]};
        for (int j = 0; j < 6; ++j)
            off[(size_t)k * 6 + j] = want[j] ? pack.add(4 * words[j] * px) : 0;
    }
    DP_HIP(c, c->mapref.io.reserve(pack.total ? pack.total : 1));
    std::vector<const float *> dd((size_t)n_views), dn((size_t)n_views);
    std::vector<float *> od((size_t)n_views), on((size_t)n_views), os((size_t)n_views);
    std::vector<int32_t *> oc((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        unsigned char *b = c->mapref.io.p;
        const size_t *f = &off[(size_t)k * 6];
        dd[(size_t)k] = (const float *)(b + f[0]);
        dn[(size_t)k] = (const float *)(b + f[1]);
        od[(size_t)k] = depth_out && depth_out[k] ? (float *)(b + f[2]) : nullptr;
        on[(size_t)k] = normal_out && normal_out[k] ? (float *)(b + f[3]) : nullptr;
        os[(size_t)k] = score_out && score_out[k] ? (float *)(b + f[4]) : nullptr;
        oc[(size_t)k] = choice_out && choice_out[k] ? (int32_t *)(b + f[5]) : nullptr;
        DP_HIP(c, hipMemcpyAsync(b + f[0], depth[k], 4 * px, hipMemcpyHostToDevice, s));
        DP_HIP(c, hipMemcpyAsync(b + f[1], normal[k], 12 * px, hipMemcpyHostToDevice, s));
    }
    rc = dp_refine_maps_device(c, views, n_views, &o, sources, dd.data(), dn.data(), od.data(), on.data(), os.data(),
                               oc.data(), stats, s);
    if (rc != DP_OK)
        return rc;
    for (int k = 0; k < n_views; ++k) {
        const size_t px = view_pixels(c, views[k]);
        if (od[(size_t)k])
            DP_HIP(c, hipMemcpyAsync(depth_out[k], od[(size_t)k], 4 * px, hipMemcpyDeviceToHost, s));
        if (on[(size_t)k])
            DP_HIP(c, hipMemcpyAsync(normal_out[k], on[(size_t)k], 12 * px, hipMemcpyDeviceToHost, s));
        if (os[(size_t)k])
            DP_HIP(c, hipMemcpyAsync(score_out[k], os[(size_t)k], 4 * px, hipMemcpyDeviceToHost, s));
        if (oc[(size_t)k])
            DP_HIP(c, hipMemcpyAsync(choice_out[k], oc[(size_t)k], 4 * px, hipMemcpyDeviceToHost, s));
    }
    DP_HIP(c, hipStreamSynchronize(s));
    return DP_OK;
}
