// dp_synth.hip -- C ABI: the synthetic-scene API (include/densepoints.h,
// dp_synth_*; the scene itself is dp_synth.h) and the host/device probes of
// include/densepoints_probe.h that belong to no other translation unit.
#include "dp_ctx.h"
#include "../../include/densepoints_probe.h"
#include "dp_synth.h"

#include <cmath>
#include <cstring>
#include <random>

// ---------------------------------------------------------------------------
// synthetic scenes
// ---------------------------------------------------------------------------

extern "C" void dp_synth_default(dp_synth_config *cfg)
{
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_views = 8;
    cfg->width = 640;
    cfg->height = 480;
    cfg->kind = 1;
    cfg->seed = 20261015ull;
    cfg->spread_deg = 35.0;
    cfg->seed_stride_px = 32.0;
    cfg->depth_noise = 0.005;
}

static const double kSynthDistance = 1.8;

extern "C" int dp_synth_cameras(const dp_synth_config *cfg, double *P)
{
    if (!cfg || !P || cfg->n_views <= 0 || cfg->n_views > DP_MAX_VIEWS || cfg->width <= 0 || cfg->height <= 0)
        return DP_E_ARG;
    const int V = cfg->n_views;
    const double spread = cfg->spread_deg * 3.14159265358979323846 / 180.0;
    const double golden = 2.39996322972865332;
    const double f = 0.8 * cfg->width, cx = 0.5 * cfg->width, cy = 0.5 * cfg->height;
    for (int v = 0; v < V; ++v) {
        const double th = spread * std::sqrt((v + 0.5) / V);
        const double ph = golden * v;
        const double C[3] = {kSynthDistance * std::sin(th) * std::cos(ph),
                             kSynthDistance * std::sin(th) * std::sin(ph), kSynthDistance * std::cos(th)};
        double z[3] = {-C[0] / kSynthDistance, -C[1] / kSynthDistance, -C[2] / kSynthDistance};
        const double down[3] = {0.0, -1.0, 0.0};
        double x[3], y[3];
        dpg::cross3(down, z, x);
        const double xn = std::sqrt(dpg::dot3(x, x));
        for (int i = 0; i < 3; ++i)
            x[i] /= xn;
        dpg::cross3(z, x, y);
        const double *R[3] = {x, y, z};
        const double K[3][3] = {{f, 0.0, cx}, {0.0, f, cy}, {0.0, 0.0, 1.0}};
        double Rt[3][4];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)
                Rt[r][k] = R[r][k];
            Rt[r][3] = -dpg::dot3(R[r], C);
        }
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k)
                P[12 * v + 4 * r + k] = (K[r][0] * Rt[0][k] + K[r][1] * Rt[1][k]) + K[r][2] * Rt[2][k];
    }
    return DP_OK;
}

static int render_cam(const dp_synth_config *cfg, const double *P, int v, dps::RenderCam &rc)
{
    double C[3], K[9], E[12];
    if (dp_view_geometry(P + 12 * v, C, K, E, nullptr) != DP_OK)
        return DP_E_ARG;
    std::memset(&rc, 0, sizeof(rc));
    for (int i = 0; i < 3; ++i) {
        rc.C[i] = C[i];
        for (int j = 0; j < 3; ++j)
            rc.Rt[3 * i + j] = E[4 * j + i];
    }
    rc.f = K[0];
    rc.cx = K[2];
    rc.cy = K[5];
    rc.W = cfg->width;
    rc.H = cfg->height;
    rc.kind = cfg->kind;
    rc.seed = cfg->seed;
    rc.px_world = kSynthDistance / (0.8 * cfg->width);
    return DP_OK;
}

extern "C" int dp_synth_render_host(const dp_synth_config *cfg, const double *P, int v, uint8_t *bgr)
{
    if (!cfg || !P || !bgr || v < 0 || v >= cfg->n_views)
        return DP_E_ARG;
    dps::RenderCam rc;
    if (render_cam(cfg, P, v, rc) != DP_OK)
        return DP_E_ARG;
    parallel_for(rc.H, [&](int64_t y) {
        for (int x = 0; x < rc.W; ++x) {
            const uint32_t px = dps::render_pixel(rc, x, (int)y);
            uint8_t *o = bgr + ((size_t)y * rc.W + x) * 3;
            o[0] = (uint8_t)(px & 255u);
            o[1] = (uint8_t)((px >> 8) & 255u);
            o[2] = (uint8_t)((px >> 16) & 255u);
        }
    });
    return DP_OK;
}

namespace {
__global__ void render_kernel(dps::RenderCam rc, uint32_t *out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x < rc.W)
        out[(size_t)y * rc.W + x] = dps::render_pixel(rc, x, y);
}
} // namespace

extern "C" int dp_synth_render_device(dp_ctx *c, const dp_synth_config *cfg, const double *P, int v,
                                      void *d_bgra, void *stream)
{
    if (!c || !cfg || !P || !d_bgra || v < 0 || v >= cfg->n_views)
        return fail(c, DP_E_ARG, "render: bad arguments");
    dps::RenderCam rc;
    if (render_cam(cfg, P, v, rc) != DP_OK)
        return fail(c, DP_E_ARG, "render: singular camera");
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    hipLaunchKernelGGL(render_kernel, dim3((rc.W + 255) / 256, rc.H), dim3(256), 0, s, rc, (uint32_t *)d_bgra);
    DP_HIP(c, hipGetLastError());
    return DP_OK;
}

extern "C" int64_t dp_synth_seeds(const dp_synth_config *cfg, const double *P, double *xyz, int64_t cap)
{
    if (!cfg || !P)
        return DP_E_ARG;
    std::mt19937_64 rng(cfg->seed);
    const double two53 = 1.0 / 9007199254740992.0;
    int64_t cnt = 0;
    const double stride = cfg->seed_stride_px > 0 ? cfg->seed_stride_px : 32.0;
    for (int v = 0; v < cfg->n_views; ++v) {
        dps::RenderCam rc;
        if (render_cam(cfg, P, v, rc) != DP_OK)
            return DP_E_ARG;
        for (double y = 0.5 * stride; y < rc.H; y += stride)
            for (double x = 0.5 * stride; x < rc.W; x += stride) {
                const double u1 = ((double)(rng() >> 11) + 0.5) * two53;
                const double u2 = ((double)(rng() >> 11) + 0.5) * two53;
                const double eps = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
                double d[3], X[3];
                dps::ray_dir(rc, x, y, d);
                if (!dps::intersect(rc, d, X))
                    continue;
                const double k = 1.0 + cfg->depth_noise * eps;
                if (xyz && cnt < cap)
                    for (int i = 0; i < 3; ++i)
                        xyz[3 * cnt + i] = rc.C[i] + (X[i] - rc.C[i]) * k;
                ++cnt;
            }
    }
    return cnt;
}

extern "C" int dp_synth_surface(const dp_synth_config *cfg, int64_t n, const double *xy, double *z_out,
                                double *normal_out)
{
    if (!cfg || n < 0 || (n > 0 && (!xy || !z_out)))
        return DP_E_ARG;
    for (int64_t q = 0; q < n; ++q) {
        const double x = xy[2 * q], y = xy[2 * q + 1];
        double z = 0.0, nx = 0.0, ny = 0.0, nz = 1.0;
        if (cfg->kind != 0) {
            double h, a, b, cx, cy;
            dps::facet(cfg->seed, dps::facet_index(x), dps::facet_index(y), h, a, b, cx, cy);
            z = (h + a * (x - cx)) + b * (y - cy);
            const double l = std::sqrt((a * a + b * b) + 1.0);
            nx = -a / l;
            ny = -b / l;
            nz = 1.0 / l;
        }
        z_out[q] = z;
        if (normal_out) {
            normal_out[3 * q] = nx;
            normal_out[3 * q + 1] = ny;
            normal_out[3 * q + 2] = nz;
        }
    }
    return DP_OK;
}

// ---------------------------------------------------------------------------
// probes (densepoints_probe.h)
// ---------------------------------------------------------------------------

extern "C" int dp_debug_stamps(uint64_t *out8)
{
    if (!out8)
        return DP_E_ARG;
    return dpk::read_stamps((unsigned long long *)out8);
}

extern "C" void dp_probe_sincos(double x, double *s, double *c) { dpm::sincos(x, *s, *c); }
extern "C" double dp_probe_acos(double x) { return dpm::acos(x); }

extern "C" int dp_probe_texture(const double P[12], int32_t W, int32_t H, const uint8_t *bgr,
                                const double corners[12], int cell, int32_t *gray)
{
    dpg::ViewDev v;
    if (view_from_P(P, W, H, 8, v) != DP_OK)
        return -1;
    dpg::TexMap tm;
    if (!dpg::texture_map(v, corners, cell, tm))
        return 0;
    auto px = [&](int x, int y) {
        const uint8_t *p = bgr + ((size_t)(tm.tly + y) * W + (size_t)(tm.tlx + x)) * 3;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    };
    for (int py = 0; py < cell; ++py)
        for (int pxx = 0; pxx < cell; ++pxx) {
            const dpg::Tap t = dpg::window_tap(tm, pxx, py);
            gray[py * cell + pxx] = dpg::blend_gray(px(t.x0, t.y0), px(t.x1, t.y0), px(t.x0, t.y1),
                                                    px(t.x1, t.y1), t.fx, t.fy);
        }
    return 1;
}

extern "C" double dp_probe_ncc(int32_t N, int32_t Sa, int32_t Saa, int32_t Sb, int32_t Sbb, int32_t Sab,
                               double denom_min)
{
    return dpg::ncc_finish(N, Sa, Saa, Sb, Sbb, Sab, denom_min);
}

namespace {
__global__ void probe_math_kernel(const double *x, int n, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    double s, c;
    dpm::sincos(x[i], s, c);
    out[4 * i + 0] = s;
    out[4 * i + 1] = c;
    out[4 * i + 2] = dpm::acos(x[i]);
    out[4 * i + 3] = sqrt(fabs(x[i]));
    // exact shortcuts of the texel loop vs the plain expressions (0 = equal)
    const double w = 1e-3 + fabs(x[i]) * 7.0;
    const double q = 32.0 / w;
    const double v = x[i] * 3.0e4;
    const double na = x[i] * 1234.567 + 0.25, nb = x[i] * -0.0071 + 1.5;
    // each shortcut only inside its documented range
    int ok = 1;
    if (w < 1e6)
        ok = ok && __double_as_longlong(dpk::div32_safe(w)) == __double_as_longlong(q);
    if (fabs(v) < 2147483647.0)
        ok = ok && dpk::rint_i32(v) == (int32_t)rint(v);
    ok = ok && __double_as_longlong(dpk::div_rn(na, nb)) == __double_as_longlong(na / nb);
    ok = ok && __double_as_longlong(dpk::recip_safe(w * 0.03125)) == __double_as_longlong(q);
    // sqrt_rn vs the library sqrt over several magnitudes of each input
    {
        const double ax = fabs(x[i]);
        const double sv[4] = {ax, ax * 1.0e6 + 1.0, ax * 1.0e-6, ax * ax * 14641.0};
        for (int k = 0; k < 4; ++k)
            ok = ok && __double_as_longlong(dpk::sqrt_rn(sv[k])) == __double_as_longlong(sqrt(sv[k]));
    }
    // a sweep of nearby denominators per input (stress the final rounding)
    for (int k = 1; k <= 16 && ok; ++k) {
        const double wk = w * (1.0 + k * 1.1102230246251565e-16 * (double)(i % 7 + 1));
        if (wk < 1e6)
            ok = __double_as_longlong(dpk::div32_safe(wk)) == __double_as_longlong(32.0 / wk);
        const double bk = nb + k * 3.3e-5;
        ok = ok && __double_as_longlong(dpk::div_rn(na, bk)) == __double_as_longlong(na / bk);
        const double sk = fabs(na) * (1.0 + k * 2.220446049250313e-16);
        ok = ok && __double_as_longlong(dpk::sqrt_rn(sk)) == __double_as_longlong(sqrt(sk));
    }
    if (!ok)
        out[4 * i + 3] = -1.0;
}
} // namespace

extern "C" int dp_probe_texel_device(const uint64_t *taps_a, const uint64_t *taps_b, const uint32_t *fxy, int n,
                                     int32_t *gray)
{
    if (n <= 0 || !taps_a || !taps_b || !fxy || !gray)
        return DP_E_ARG;
    void *d = nullptr;
    const size_t nb = (size_t)n;
    if (hipMalloc(&d, nb * (8 + 8 + 4 + 4)) != hipSuccess)
        return DP_E_HIP;
    unsigned long long *da = (unsigned long long *)d, *db = da + nb;
    uint32_t *df = (uint32_t *)(db + nb);
    int32_t *dg = (int32_t *)(df + nb);
    hipMemcpy(da, taps_a, nb * 8, hipMemcpyHostToDevice);
    hipMemcpy(db, taps_b, nb * 8, hipMemcpyHostToDevice);
    hipMemcpy(df, fxy, nb * 4, hipMemcpyHostToDevice);
    hipError_t e = dpk::launch_probe_texel(da, db, df, n, dg);
    if (e == hipSuccess)
        e = hipMemcpy(gray, dg, nb * 4, hipMemcpyDeviceToHost);
    hipFree(d);
    return e == hipSuccess ? DP_OK : DP_E_HIP;
}

extern "C" int dp_probe_math_device(const double *x, int n, double *out)
{
    if (n <= 0 || !x || !out)
        return DP_E_ARG;
    double *dx = nullptr, *dout = nullptr;
    if (hipMalloc(&dx, sizeof(double) * n) != hipSuccess)
        return DP_E_HIP;
    if (hipMalloc(&dout, sizeof(double) * 4 * n) != hipSuccess) {
        hipFree(dx);
        return DP_E_HIP;
    }
    hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, dout);
    hipError_t e = hipMemcpy(out, dout, sizeof(double) * 4 * n, hipMemcpyDeviceToHost);
    hipFree(dx);
    hipFree(dout);
    return e == hipSuccess ? DP_OK : DP_E_HIP;
}
