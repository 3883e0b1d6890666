// dp_fast.hip -- host side of the performance mode of the patch refine: its
// options, the fp16 gray planes and fp32 cameras of the current level, the
// launch of a refine job (dp_fast_launch) and the C ABI.  The device code is
// dp_fast_kernel.hip; dp_fast.h is what the two share.  Spec:
// include/densepoints.h (dp_fast_options) and oracle/or_fast.c.
#include "dp_fast.h"

#include <cmath>

namespace {

// gray plane pitch (pixels): a tile row may read two pixels past the image
// edge (a whole 32-bit pair after the right tap), 128-B aligned rows
inline int gray_pitch(int W) { return (W + 2 + 63) & ~63; }

int fast_check_options(dp_ctx *c, const dp_fast_options &f)
{
    if (f.iters < 0 || f.iters > 64 || f.margin < 0 || f.margin > dpk::kFastMaxMargin || f.tile_budget < 64 ||
        f.tile_budget > dpk::kFastBudget || f.max_views < 2 || f.max_views > dpk::kFastMaxV ||
        !(f.fd_step >= 0x1p-20f && f.fd_step <= 0x1p+20f) || !(f.ls_step > 0.0f && f.ls_step <= 0x1p+20f) ||
        (f.densify != 0 && f.densify != 1) || (f.gradient != 0 && f.gradient != 1) ||
        (f.filter_max_views != 0 && (f.filter_max_views < 2 || f.filter_max_views > dpk::kFastMaxV)))
        return fail(c, DP_E_ARG, "dp_fast_options out of range (margin <= 7, tile_budget <= 16384, 2 <= max_views "
                                 "<= 32, fd_step in [2^-20, 2^20], 0 < ls_step <= 2^20, gradient 0 or 1, "
                                 "filter_max_views 0 or 2..32)");
    return DP_OK;
}

// byte offset of the FastCam table in the d_gray allocation
inline size_t fast_cam_offset(int V) { return (sizeof(dpk::GrayPlane) * (size_t)V + 255) & ~(size_t)255; }

int ensure_gray(dp_ctx *c)
{
    if (!c->V)
        return fail(c, DP_E_STATE, "no views set");
    if (c->gray_ready && c->gray_level == c->level && c->gray_V == c->V)
        return DP_OK;
    hipSetDevice(c->device);
    // a fast kernel launched on a caller's stream may still read the old
    // planes and tables: let the device drain before they are rewritten
    DP_HIP(c, hipDeviceSynchronize());
    std::vector<dpk::GrayPlane> gp(c->V);
    size_t total = 0;
    std::vector<size_t> off(c->V);
    for (int v = 0; v < c->V; ++v) {
        const int pitch = gray_pitch(c->hv[v].W);
        off[v] = total;
        total += (size_t)pitch * (size_t)c->hv[v].H;
        gp[v].w = c->hv[v].W;
        gp[v].h = c->hv[v].H;
        gp[v].pitch = pitch;
        gp[v].pad = 0;
    }
    if (total > c->gray_cap) {
        c->gray_cap = 0;
        DP_HIP(c, c->gray_pool.alloc(total * sizeof(__half)));
        c->gray_cap = total;
    }
    for (int v = 0; v < c->V; ++v)
        gp[v].p = (const __half *)c->gray_pool.p + off[v];
    std::vector<dpk::PyrPlane> src(c->V);
    int mw = 0, mh = 0;
    for (int v = 0; v < c->V; ++v) {
        src[v] = dpk::PyrPlane{(uint32_t *)c->hv[v].img, c->hv[v].W, c->hv[v].H, c->hv[v].pitch, 0};
        mw = c->hv[v].W > mw ? c->hv[v].W : mw;
        mh = c->hv[v].H > mh ? c->hv[v].H : mh;
    }
    // fp32 cameras of the level (or_fast.c fcam_of): rows 0-1 of P times 32,
    // row 2, centre and unit x-axis, each rounded once
    std::vector<dpk::FastCam> fc(c->V);
    for (int v = 0; v < c->V; ++v) {
        const dpg::ViewDev &h = c->hv[v];
        for (int k = 0; k < 12; ++k)
            fc[v].Q[k] = (float)(k < 8 ? 32.0 * h.P[k] : h.P[k]);
        for (int k = 0; k < 3; ++k) {
            fc[v].C[k] = (float)h.C[k];
            fc[v].xr[k] = (float)h.xr[k];
        }
        fc[v].W = h.W;
        fc[v].H = h.H;
    }
    dpk::PyrPlane *d_src = nullptr;
    // one table: GrayPlane[V], then FastCam[V] at fast_cam_offset(V)
    DP_HIP(c, c->d_gray.alloc(fast_cam_offset(c->V) + sizeof(dpk::FastCam) * c->V));
    DP_HIP(c, hipMalloc(&d_src, sizeof(dpk::PyrPlane) * c->V));
    DP_HIP(c, hipMemcpy(c->d_gray.p, gp.data(), sizeof(dpk::GrayPlane) * c->V, hipMemcpyHostToDevice));
    DP_HIP(c, hipMemcpy((char *)c->d_gray.p + fast_cam_offset(c->V), fc.data(), sizeof(dpk::FastCam) * c->V,
                        hipMemcpyHostToDevice));
    DP_HIP(c, hipMemcpy(d_src, src.data(), sizeof(dpk::PyrPlane) * c->V, hipMemcpyHostToDevice));
    hipError_t e = dpk::launch_gray(d_src, (const dpk::GrayPlane *)c->d_gray.p, c->V, gray_pitch(mw), mh, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    hipFree(d_src);
    DP_HIP(c, e);
    c->gray_ready = true;
    c->gray_level = c->level;
    c->gray_V = c->V;
    return DP_OK;
}

} // namespace

int dp_gray_planes(dp_ctx *c, std::vector<dpk::GrayPlane> &out)
{
    int rc = ensure_gray(c);
    if (rc != DP_OK)
        return rc;
    out.resize((size_t)c->V);
    size_t off = 0;
    for (int v = 0; v < c->V; ++v) {
        const int pitch = gray_pitch(c->hv[v].W);
        out[(size_t)v] = dpk::GrayPlane{(const __half *)c->gray_pool.p + off, c->hv[v].W, c->hv[v].H, pitch, 0};
        off += (size_t)pitch * (size_t)c->hv[v].H;
    }
    return DP_OK;
}

int dp_fast_launch(dp_ctx *c, const dpk::RefineJob &job, hipStream_t s)
{
    int rc = ensure_gray(c);
    if (rc != DP_OK)
        return rc;
    const int cell = job.cell;
    const dpk::GenDev *gen = job.gen;
    dpk::FastArgs a{};
    a.views = c->d_views;
    a.gray = (const dpk::GrayPlane *)c->d_gray.p;
    a.cams = (const dpk::FastCam *)((const char *)c->d_gray.p + fast_cam_offset(c->V));
    a.V = c->V;
    a.cell = cell;
    a.mode = job.mode;
    // a device-resident generation is sized on the device: its launch is laid
    // out as for n = 0 (one candidate per dequeue), whatever the buffers hold
    a.n = gen ? 0 : job.n;
    a.opt = c->opt;
    a.fo = c->fopt;
    a.patches = job.patches;
    a.accept = job.accept;
    a.work = c->d_work.p;
    a.evals = c->d_evals.p;
    a.parents = job.parents;
    a.parent0 = job.parent0;
    a.items = job.items;
    a.max_pops = job.max_pops;
    a.gen = gen;
    a.epi = job.epi;
    a.seq0 = job.seq0;
    a.claim_grid = c->grid.p;
    a.grid_scale = (double)c->opt.grid_scale;
    // the InitRelatedImages thresholds as cosines, by the host libm (the
    // spec's), rounded to fp32, and their fp32 squares
    a.cvis = (float)std::cos(c->opt.visible_angle);
    a.ccand = (float)std::cos(c->opt.candidate_angle);
    a.cvis2 = a.cvis * a.cvis;
    a.ccand2 = a.ccand * a.ccand;
    {
        const int N = cell * cell;
        a.dmin = ((c->opt.ncc_denom_min * 256.0) * (double)N) * (double)N;
        a.dminf = (float)a.dmin;
        a.gs = (1.0f / c->fopt.fd_step) * 0x1p-24f;
    }
    DP_HIP(c, c->d_fstats.reserve(8));
    a.stats = c->d_fstats.p;
    if (!gen) {
        // a device-resident generation's counters are zeroed by the previous
        // organizer (dp_bfs.hip) and its statistics by its batch (run_generations)
        DP_HIP(c, hipMemsetAsync(c->d_fstats.p, 0, 8 * sizeof(unsigned long long), s));
        DP_HIP(c, hipMemsetAsync(c->d_work.p, 0, sizeof(uint32_t), s));
    }
    DP_HIP(c, hipEventRecord(c->e0, s));
    DP_HIP(c, dpk::launch_fast(a, c->fopt.tile_budget, s));
    DP_HIP(c, hipEventRecord(c->e1, s));
    c->timed = true;
    return DP_OK;
}

extern "C" void dp_default_fast_options(dp_fast_options *f)
{
    if (!f)
        return;
    *f = dp_fast_options{};
    f->iters = 4;
    f->margin = 2;
    f->tile_budget = 6656; // 4 waves per SIMD (the 6.5 KiB arena); up to kFastBudget
    f->max_views = 8; // spec v5 (r05): the refine's views keep their tile margin (was 32)
    f->fd_step = 0.5f;
    f->ls_step = 1.0f;
    f->densify = 0;
    f->gradient = 0;
    f->filter_max_views = dpk::kFastMaxV; // the filter scores every view that fits the budget
}

extern "C" int dp_set_fast_options(dp_ctx *c, const dp_fast_options *f)
{
    if (!c || !f)
        return DP_E_ARG;
    int rc = fast_check_options(c, *f);
    if (rc != DP_OK)
        return rc;
    c->fopt = *f;
    return DP_OK;
}

extern "C" int dp_build_gray(dp_ctx *c)
{
    if (!c)
        return DP_E_ARG;
    c->gray_ready = false;
    return ensure_gray(c);
}

extern "C" int dp_read_gray(dp_ctx *c, int view, uint16_t *out)
{
    if (!c || !out)
        return DP_E_ARG;
    if (view < 0 || view >= c->V)
        return fail(c, DP_E_ARG, "dp_read_gray: bad view");
    int rc = ensure_gray(c);
    if (rc != DP_OK)
        return rc;
    const int W = c->hv[view].W, H = c->hv[view].H, pitch = gray_pitch(W);
    size_t off = 0;
    for (int v = 0; v < view; ++v)
        off += (size_t)gray_pitch(c->hv[v].W) * (size_t)c->hv[v].H;
    DP_HIP(c, hipMemcpy2D(out, (size_t)W * 2, (const __half *)c->gray_pool.p + off, (size_t)pitch * 2, (size_t)W * 2,
                          (size_t)H, hipMemcpyDeviceToHost));
    return DP_OK;
}

extern "C" int dp_probe_recip_f32_device(const float *x, int n, float *out)
{
    if (n < 0 || (n > 0 && (!x || !out)))
        return DP_E_ARG;
    if (n == 0)
        return DP_OK;
    float *dx = nullptr, *dy = nullptr;
    if (hipMalloc(&dx, sizeof(float) * n) != hipSuccess)
        return DP_E_OOM;
    if (hipMalloc(&dy, sizeof(float) * n) != hipSuccess) {
        hipFree(dx);
        return DP_E_OOM;
    }
    hipError_t e = hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = dpk::launch_recip_probe(dx, n, dy);
    if (e == hipSuccess)
        e = hipMemcpy(out, dy, sizeof(float) * n, hipMemcpyDeviceToHost);
    hipFree(dx);
    hipFree(dy);
    return e == hipSuccess ? DP_OK : DP_E_HIP;
}

extern "C" int dp_probe_grad_q24_device(const double *dncc, int n, int32_t *out)
{
    if (n < 0 || (n > 0 && (!dncc || !out)))
        return DP_E_ARG;
    if (n == 0)
        return DP_OK;
    double *dx = nullptr;
    int32_t *dy = nullptr;
    if (hipMalloc(&dx, sizeof(double) * n) != hipSuccess)
        return DP_E_OOM;
    if (hipMalloc(&dy, sizeof(int32_t) * n) != hipSuccess) {
        hipFree(dx);
        return DP_E_OOM;
    }
    hipError_t e = hipMemcpy(dx, dncc, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = dpk::launch_grad_q24_probe(dx, n, dy);
    if (e == hipSuccess)
        e = hipMemcpy(out, dy, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    hipFree(dx);
    hipFree(dy);
    return e == hipSuccess ? DP_OK : DP_E_HIP;
}

extern "C" int dp_fast_last_stats(dp_ctx *c, dp_fast_stats *out)
{
    if (!c || !out)
        return DP_E_ARG;
    *out = dp_fast_stats{};
    if (!c->d_fstats.p)
        return DP_OK;
    unsigned long long v[5];
    DP_HIP(c, hipDeviceSynchronize());
    DP_HIP(c, hipMemcpy(v, c->d_fstats.p, sizeof(v), hipMemcpyDeviceToHost));
    out->clipped_stagings = (int64_t)v[4];
    out->patches = (int64_t)v[0];
    out->evals = (int64_t)v[1];
    out->view_evals = (int64_t)v[2];
    out->staged_bytes = (int64_t)v[3];
    return DP_OK;
}

extern "C" int dp_probe_lds_unaligned_device(uint32_t *out256)
{
    if (!out256)
        return DP_E_ARG;
    uint32_t *d = nullptr;
    if (hipMalloc(&d, 256 * sizeof(uint32_t)) != hipSuccess)
        return DP_E_OOM;
    hipError_t e = dpk::launch_lds_probe(d);
    if (e == hipSuccess)
        e = hipMemcpy(out256, d, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    hipFree(d);
    return e == hipSuccess ? DP_OK : DP_E_HIP;
}
