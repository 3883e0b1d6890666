// dp_capi.hip -- C ABI (include/densepoints.h): contexts and options, view
// upload, pyramids, the patch filter's entry points, and the batch
// refine/expand/eval API with the one launcher (launch_job) every refine of
// the library goes through.  The densify engine is dp_densify.hip.
#include "dp_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>


// ---------------------------------------------------------------------------
// geometry (product implementation of View::SetProjectionMatrix)
// ---------------------------------------------------------------------------

static double det_cols(const double *a, const double *b, const double *c)
{
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1])) +
           c[0] * (a[1] * b[2] - a[2] * b[1]);
}

extern "C" int dp_view_geometry(const double P[12], double C[3], double K[9], double E[12],
                                double xaxis[3])
{
    // camera centre: cofactor null vector of P (types.cpp:34-37 uses SVD)
    double col[4][3];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            col[c][r] = P[r * 4 + c];
    const double cx = det_cols(col[1], col[2], col[3]);
    const double cy = -det_cols(col[0], col[2], col[3]);
    const double cz = det_cols(col[0], col[1], col[3]);
    const double cw = -det_cols(col[0], col[1], col[2]);
    if (cw == 0.0 || !std::isfinite(cw))
        return DP_E_ARG;
    const double Cc[3] = {cx / cw, cy / cw, cz / cw};
    // RQ with positive K diagonal (types.cpp:39-67): bottom-up Gram-Schmidt
    const double *m0 = P, *m1 = P + 4, *m2 = P + 8;
    double q2[3], q1[3], q0[3], t[3];
    const double l2 = std::sqrt(dpg::dot3(m2, m2));
    for (int i = 0; i < 3; ++i)
        q2[i] = m2[i] / l2;
    const double p12 = dpg::dot3(m1, q2);
    for (int i = 0; i < 3; ++i)
        t[i] = m1[i] - p12 * q2[i];
    const double l1 = std::sqrt(dpg::dot3(t, t));
    for (int i = 0; i < 3; ++i)
        q1[i] = t[i] / l1;
    const double p02 = dpg::dot3(m0, q2), p01 = dpg::dot3(m0, q1);
    for (int i = 0; i < 3; ++i)
        t[i] = (m0[i] - p02 * q2[i]) - p01 * q1[i];
    const double l0 = std::sqrt(dpg::dot3(t, t));
    for (int i = 0; i < 3; ++i)
        q0[i] = t[i] / l0;
    if (C)
        std::memcpy(C, Cc, sizeof(Cc));
    if (xaxis)
        std::memcpy(xaxis, q0, sizeof(q0));
    if (K) {
        const double k22 = dpg::dot3(m2, q2);
        const double k[9] = {dpg::dot3(m0, q0) / k22, dpg::dot3(m0, q1) / k22, dpg::dot3(m0, q2) / k22,
                             0.0, dpg::dot3(m1, q1) / k22, dpg::dot3(m1, q2) / k22,
                             0.0, 0.0, 1.0};
        std::memcpy(K, k, sizeof(k));
    }
    if (E) {
        const double *R[3] = {q0, q1, q2};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                E[r * 4 + c] = R[r][c];
            E[r * 4 + 3] = -dpg::dot3(R[r], Cc);
        }
    }
    return DP_OK;
}

int view_from_P(const double *P, int W, int H, int gs, dpg::ViewDev &v)
{
    std::memset(&v, 0, sizeof(v));
    std::memcpy(v.P, P, sizeof(v.P));
    double xa[3];
    int rc = dp_view_geometry(P, v.C, nullptr, nullptr, xa);
    if (rc != DP_OK)
        return rc;
    const double nx = std::sqrt(dpg::dot3(xa, xa));
    for (int i = 0; i < 3; ++i)
        v.xr[i] = xa[i] / nx; // GetXAxis().normalized() (patch.cpp:95)
    v.W = W;
    v.H = H;
    v.pitch = W;
    v.gw = W / gs; // PatchOrganizer::AllocateViews (patch_organizer.cpp:35-36)
    v.gh = H / gs;
    return DP_OK;
}

// ---------------------------------------------------------------------------
// options / context
// ---------------------------------------------------------------------------

extern "C" void dp_default_options(dp_options *o)
{
    std::memset(o, 0, sizeof(*o));
    o->seed_cell_size = 16;
    o->expand_cell_size = 11;
    o->grid_scale = 8;
    o->max_patches_per_cell = 1;
    o->min_visible = 3;
    o->min_expand_visible = 2;
    o->nm_max_evals = 500;
    o->ncc_threshold = 0.6;
    o->visible_angle = 0.78;
    o->candidate_angle = 1.04;
    o->nm_step[0] = 0.02;
    o->nm_step[1] = 0.2;
    o->nm_step[2] = 0.2;
    o->nm_eps = 0.0001;
    o->ncc_denom_min = 0.1;
    o->max_pops = 10000000;
}

extern "C" int dp_abi_version(void) { return DP_ABI_VERSION; }

static int check_options(dp_ctx *c, const dp_options &o)
{
    if (o.seed_cell_size < 2 || o.seed_cell_size > DP_MAX_CELL || o.expand_cell_size < 2 ||
        o.expand_cell_size > DP_MAX_CELL)
        return fail(c, DP_E_ARG, "cell sizes must be in [2, 16]");
    if (o.grid_scale <= 0)
        return fail(c, DP_E_ARG, "grid_scale must be > 0");
    if (o.max_patches_per_cell < 1 || o.max_patches_per_cell > 64)
        return fail(c, DP_E_ARG, "max_patches_per_cell must be in [1, 64]");
    if (o.nm_max_evals < 1)
        return fail(c, DP_E_ARG, "nm_max_evals must be >= 1");
    return DP_OK;
}

extern "C" int dp_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int dp_ctx_create(const dp_options *opt, int device, dp_ctx **out)
{
    if (!out)
        return DP_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return DP_E_NODEVICE;
    if (device < 0 || device >= ndev)
        return DP_E_ARG;
    dp_ctx *c = new (std::nothrow) dp_ctx();
    if (!c)
        return DP_E_OOM;
    c->device = device;
    {
        const char *e = getenv("DP_NO_LPT");
        c->lpt_off = e && e[0] == '1';
        const char *g = getenv("DP_GEN_CAP");
        c->gen_cap_test = g ? std::atoll(g) : 0;
    }
    if (opt)
        c->opt = *opt;
    else
        dp_default_options(&c->opt);
    dp_default_fast_options(&c->fopt);
    int rc = check_options(c, c->opt);
    if (rc != DP_OK) {
        delete c;
        return rc;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        c->d_work.reserve(1) != hipSuccess || c->d_evals.reserve(1) != hipSuccess ||
        c->e0.create() != hipSuccess || c->e1.create() != hipSuccess ||
        c->ej.create(hipEventDisableTiming) != hipSuccess || c->mbox.reserve(8) != hipSuccess ||
        hipMemset(c->mbox.p, 0, 8 * sizeof(unsigned long long)) != hipSuccess) {
        dp_ctx_destroy(c);
        return DP_E_HIP;
    }
    *out = c;
    return DP_OK;
}

static void free_pyramid(dp_ctx *c)
{
    for (uint32_t *p : c->pyr_pool)
        hipFree(p);
    c->pyr_pool.clear();
    if (c->planes.size() > 1)
        c->planes.resize(1);
    c->level = 0;
}

static void free_views(dp_ctx *c)
{
    free_pyramid(c);
    c->planes.clear();
    c->P0.clear();
    for (uint32_t *p : c->own_img)
        hipFree(p);
    c->own_img.clear();
    if (c->d_views)
        hipFree(c->d_views);
    c->d_views = nullptr;
    c->hv.clear();
    c->V = 0;
}

extern "C" int dp_ctx_destroy(dp_ctx *c)
{
    if (!c)
        return DP_OK;
    hipSetDevice(c->device);
    if (c->stream)
        hipStreamSynchronize(c->stream);
    free_views(c);
    // the members free themselves (dp_buf.h); the stream outlives them all
    const hipStream_t stream = c->stream;
    delete c;
    if (stream)
        hipStreamDestroy(stream);
    return DP_OK;
}

extern "C" const char *dp_last_error(const dp_ctx *c) { return c ? c->err.c_str() : "null context"; }

extern "C" int dp_set_options(dp_ctx *c, const dp_options *opt)
{
    if (!c || !opt)
        return DP_E_ARG;
    int rc = check_options(c, *opt);
    if (rc != DP_OK)
        return rc;
    c->opt = *opt;
    // grid geometry depends on grid_scale
    for (auto &v : c->hv) {
        v.gw = v.W / opt->grid_scale;
        v.gh = v.H / opt->grid_scale;
    }
    if (c->V) {
        hipSetDevice(c->device);
        DP_HIP(c, hipMemcpy(c->d_views, c->hv.data(), sizeof(dpg::ViewDev) * c->V, hipMemcpyHostToDevice));
    }
    return DP_OK;
}

static int upload_view_table(dp_ctx *c)
{
    int64_t off = 0;
    for (auto &v : c->hv) {
        v.grid_off = off;
        off += (int64_t)v.gw * v.gh;
    }
    c->grid_cells = off;
    // narrow addressing when every plane ends within 4 GiB of the lowest one
    // and the 24-bit row multiply holds (pitch * 4 < 2^24, H < 2^24)
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    bool fits = true;
    for (auto &v : c->hv) {
        const uintptr_t b = (uintptr_t)v.img;
        lo = b < lo ? b : lo;
        const uintptr_t e = b + (uintptr_t)v.pitch * (uintptr_t)v.H * 4u;
        hi = e > hi ? e : hi;
        fits = fits && (int64_t)v.pitch * 4 < (1 << 24) && v.H < (1 << 24);
    }
    // DP_WIDE_ADDRESSING=1 forces 64-bit tap addresses (tests cover both paths)
    const char *wide = getenv("DP_WIDE_ADDRESSING");
    c->narrow = fits && hi - lo <= 0xFFFFFFF0ull && !(wide && wide[0] == '1');
    c->img_base = (const char *)lo;
    for (auto &v : c->hv)
        v.img_off = c->narrow ? (uint32_t)((uintptr_t)v.img - lo) : 0u;
    DP_HIP(c, hipMalloc(&c->d_views, sizeof(dpg::ViewDev) * c->V));
    DP_HIP(c, hipMemcpy(c->d_views, c->hv.data(), sizeof(dpg::ViewDev) * c->V, hipMemcpyHostToDevice));
    return DP_OK;
}

static void record_level0(dp_ctx *c, const double *P)
{
    c->gray_ready = false; // performance-mode gray planes follow the views
    c->P0.assign(P, P + 12 * (size_t)c->V);
    c->planes.assign(1, std::vector<dpk::PyrPlane>(c->V));
    for (int v = 0; v < c->V; ++v)
        c->planes[0][v] = dpk::PyrPlane{(uint32_t *)c->hv[v].img, c->hv[v].W, c->hv[v].H, c->hv[v].pitch, 0};
    c->level = 0;
}

extern "C" int dp_set_views(dp_ctx *c, int V, const double *P, const dp_image *images)
{
    if (!c || V <= 0 || V > DP_MAX_VIEWS || !P || !images)
        return fail(c, DP_E_ARG, "dp_set_views: bad arguments (1 <= V <= 128)");
    hipSetDevice(c->device);
    DP_HIP(c, hipStreamSynchronize(c->stream));
    free_views(c);
    c->hv.resize(V);
    // one pool for all planes (narrow addressing whenever it is < 4 GiB)
    size_t total = 0;
    for (int v = 0; v < V; ++v) {
        const dp_image &im = images[v];
        if (im.width <= 0 || im.height <= 0 || !im.bgr)
            return fail(c, DP_E_ARG, "dp_set_views: empty image");
        total += (size_t)im.width * (size_t)im.height;
    }
    uint32_t *pool = nullptr;
    DP_HIP(c, hipMalloc(&pool, total * sizeof(uint32_t)));
    c->own_img.push_back(pool);
    std::vector<uint32_t> tmp;
    size_t at = 0;
    for (int v = 0; v < V; ++v) {
        const dp_image &im = images[v];
        if (view_from_P(P + 12 * v, im.width, im.height, c->opt.grid_scale, c->hv[v]) != DP_OK)
            return fail(c, DP_E_ARG, "dp_set_views: singular projection matrix");
        const size_t stride = im.stride ? (size_t)im.stride : (size_t)im.width * 3;
        tmp.resize((size_t)im.width * im.height);
        parallel_for(im.height, [&](int64_t y) {
            const uint8_t *row = im.bgr + (size_t)y * stride;
            uint32_t *o = tmp.data() + (size_t)y * im.width;
            for (int x = 0; x < im.width; ++x)
                o[x] = (uint32_t)row[3 * x] | ((uint32_t)row[3 * x + 1] << 8) |
                       ((uint32_t)row[3 * x + 2] << 16) | 0xFF000000u;
        });
        uint32_t *d = pool + at;
        at += tmp.size();
        DP_HIP(c, hipMemcpy(d, tmp.data(), tmp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->hv[v].img = d;
    }
    c->V = V;
    record_level0(c, P);
    return upload_view_table(c);
}

extern "C" int dp_set_views_device(dp_ctx *c, int V, const double *P, const int32_t *W, const int32_t *H,
                                   const int32_t *pitch, const void *const *dev_bgra)
{
    if (!c || V <= 0 || V > DP_MAX_VIEWS || !P || !W || !H || !dev_bgra)
        return fail(c, DP_E_ARG, "dp_set_views_device: bad arguments");
    hipSetDevice(c->device);
    DP_HIP(c, hipStreamSynchronize(c->stream));
    free_views(c);
    c->hv.resize(V);
    for (int v = 0; v < V; ++v) {
        if (W[v] <= 0 || H[v] <= 0 || !dev_bgra[v])
            return fail(c, DP_E_ARG, "dp_set_views_device: empty image");
        if (view_from_P(P + 12 * v, W[v], H[v], c->opt.grid_scale, c->hv[v]) != DP_OK)
            return fail(c, DP_E_ARG, "dp_set_views_device: singular projection matrix");
        c->hv[v].pitch = pitch ? pitch[v] : W[v];
        c->hv[v].img = (const uint32_t *)dev_bgra[v];
    }
    c->V = V;
    record_level0(c, P);
    return upload_view_table(c);
}

// ---------------------------------------------------------------------------
// image pyramids
// ---------------------------------------------------------------------------

extern "C" int dp_build_pyramid(dp_ctx *c, int levels)
{
    if (!c || levels < 1 || levels > DP_MAX_LEVELS)
        return fail(c, DP_E_ARG, "dp_build_pyramid: levels must be in [1, DP_MAX_LEVELS]");
    if (c->V <= 0 || c->planes.empty())
        return fail(c, DP_E_STATE, "dp_build_pyramid: no views set");
    c->gray_ready = false;
    hipSetDevice(c->device);
    DP_HIP(c, hipStreamSynchronize(c->stream));
    if (c->level != 0) {
        int rc = dp_set_level(c, 0);
        if (rc != DP_OK)
            return rc;
    }
    free_pyramid(c);
    const int V = c->V;
    dpk::PyrPlane *d_tab = nullptr;
    DP_HIP(c, hipMalloc(&d_tab, sizeof(dpk::PyrPlane) * 2 * V));
    int rc = DP_OK;
    for (int l = 1; l < levels && rc == DP_OK; ++l) {
        const std::vector<dpk::PyrPlane> &src = c->planes[l - 1];
        std::vector<dpk::PyrPlane> dst(V);
        size_t total = 0;
        int mw = 0, mh = 0;
        for (int v = 0; v < V; ++v) {
            dst[v].w = (src[v].w + 1) / 2;
            dst[v].h = (src[v].h + 1) / 2;
            dst[v].pitch = dst[v].w;
            total += (size_t)dst[v].w * (size_t)dst[v].h;
            mw = std::max(mw, dst[v].w);
            mh = std::max(mh, dst[v].h);
        }
        uint32_t *pool = nullptr;
        if (hipMalloc(&pool, total * sizeof(uint32_t)) != hipSuccess) {
            rc = fail(c, DP_E_OOM, "dp_build_pyramid: out of device memory");
            break;
        }
        c->pyr_pool.push_back(pool);
        size_t at = 0;
        for (int v = 0; v < V; ++v) {
            dst[v].img = pool + at;
            at += (size_t)dst[v].w * (size_t)dst[v].h;
        }
        hipError_t e = hipMemcpyAsync(d_tab, src.data(), sizeof(dpk::PyrPlane) * V, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_tab + V, dst.data(), sizeof(dpk::PyrPlane) * V, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = dpk::launch_pyr_down(d_tab, d_tab + V, V, mw, mh, c->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            rc = fail(c, DP_E_HIP, std::string("dp_build_pyramid: ") + hipGetErrorString(e));
            break;
        }
        c->planes.push_back(std::move(dst));
    }
    hipFree(d_tab);
    return rc;
}

extern "C" int dp_set_level(dp_ctx *c, int level)
{
    if (!c)
        return DP_E_ARG;
    if (c->V <= 0 || c->planes.empty())
        return fail(c, DP_E_STATE, "dp_set_level: no views set");
    if (level < 0 || level >= (int)c->planes.size())
        return fail(c, DP_E_ARG, "dp_set_level: level not built (dp_build_pyramid)");
    hipSetDevice(c->device);
    DP_HIP(c, hipStreamSynchronize(c->stream));
    // the level-L scene: pyrDown^L images, projection rows 0-1 scaled by 2^-L
    // (exact), camera geometry and grids recomputed from that P
    const double s = std::ldexp(1.0, -level);
    std::vector<dpg::ViewDev> hv(c->V);
    for (int v = 0; v < c->V; ++v) {
        double P[12];
        for (int i = 0; i < 12; ++i)
            P[i] = c->P0[12 * v + i] * (i < 8 ? s : 1.0);
        const dpk::PyrPlane &pl = c->planes[level][v];
        if (view_from_P(P, pl.w, pl.h, c->opt.grid_scale, hv[v]) != DP_OK)
            return fail(c, DP_E_ARG, "dp_set_level: singular projection matrix");
        hv[v].pitch = pl.pitch;
        hv[v].img = pl.img;
    }
    if (c->d_views)
        hipFree(c->d_views);
    c->d_views = nullptr;
    c->hv = std::move(hv);
    c->level = level;
    c->gray_ready = false;
    return upload_view_table(c);
}

extern "C" int dp_level_info(const dp_ctx *c, int level, int view, int32_t *width, int32_t *height,
                             const void **d_bgra)
{
    if (!c || level < 0 || level >= (int)c->planes.size() || view < 0 || view >= c->V)
        return DP_E_ARG;
    const dpk::PyrPlane &pl = c->planes[level][view];
    if (width)
        *width = pl.w;
    if (height)
        *height = pl.h;
    if (d_bgra)
        *d_bgra = pl.img;
    return DP_OK;
}

extern "C" int dp_read_level(dp_ctx *c, int level, int view, uint8_t *bgr_out)
{
    if (!c || !bgr_out || level < 0 || level >= (int)c->planes.size() || view < 0 || view >= c->V)
        return fail(c, DP_E_ARG, "dp_read_level: bad level/view");
    hipSetDevice(c->device);
    const dpk::PyrPlane &pl = c->planes[level][view];
    std::vector<uint32_t> tmp((size_t)pl.w * pl.h);
    DP_HIP(c, hipStreamSynchronize(c->stream));
    DP_HIP(c, hipMemcpy2D(tmp.data(), sizeof(uint32_t) * pl.w, pl.img, sizeof(uint32_t) * pl.pitch,
                          sizeof(uint32_t) * pl.w, pl.h, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) {
        bgr_out[3 * i] = (uint8_t)(tmp[i] & 255u);
        bgr_out[3 * i + 1] = (uint8_t)((tmp[i] >> 8) & 255u);
        bgr_out[3 * i + 2] = (uint8_t)((tmp[i] >> 16) & 255u);
    }
    return DP_OK;
}

// ---------------------------------------------------------------------------
// patch filter (spec in include/densepoints.h)
// ---------------------------------------------------------------------------

extern "C" void dp_default_filter_options(dp_filter_options *fo)
{
    if (!fo)
        return;
    fo->passes = DP_FILTER_VISIBILITY | DP_FILTER_NEIGHBORS;
    fo->reserved = 0;
    fo->min_neighbor_frac = 0.25;
}

extern "C" int dp_filter_patches_device(dp_ctx *c, const dp_patch *d_patches, int64_t n, const dp_filter_options *fo,
                                        uint8_t *d_keep, void *stream)
{
    if (!c || n < 0 || (n > 0 && (!d_patches || !d_keep)) || n > 0xFFFFFFFFll)
        return fail(c, DP_E_ARG, "dp_filter_patches: bad arguments");
    if (c->V <= 0)
        return fail(c, DP_E_STATE, "dp_filter_patches: no views set");
    dp_filter_options o;
    dp_default_filter_options(&o);
    if (fo)
        o = *fo;
    if (n == 0)
        return DP_OK;
    hipSetDevice(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DP_HIP(c, c->front.reserve((size_t)c->grid_cells + 1));
    DP_HIP(c, c->f_alive.reserve((size_t)n));
    DP_HIP(c, c->f_rho.reserve((size_t)n));
    dpk::FilterArgs a{};
    a.views = c->d_views;
    a.V = c->V;
    a.patches = d_patches;
    a.n = n;
    a.alive = c->f_alive.p;
    a.front = c->front.p;
    a.rho = c->f_rho.p;
    a.grid_scale = (double)c->opt.grid_scale;
    a.min_neighbor_frac = o.min_neighbor_frac;
    const size_t fb = sizeof(unsigned long long) * ((size_t)c->grid_cells + 1);
    DP_HIP(c, hipMemsetAsync(c->f_alive.p, 1, (size_t)n, s));
    DP_HIP(c, dpk::launch_filter_rho(a, s));
    if (o.passes & DP_FILTER_VISIBILITY) {
        DP_HIP(c, hipMemsetAsync(c->front.p, 0xFF, fb, s));
        DP_HIP(c, dpk::launch_filter_front(a, s));
        DP_HIP(c, dpk::launch_filter_visibility(a, d_keep, s));
        DP_HIP(c, hipMemcpyAsync(c->f_alive.p, d_keep, (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    if (o.passes & DP_FILTER_NEIGHBORS) {
        DP_HIP(c, hipMemsetAsync(c->front.p, 0xFF, fb, s));
        DP_HIP(c, dpk::launch_filter_front(a, s));
        DP_HIP(c, dpk::launch_filter_neighbors(a, d_keep, s));
    } else if (!(o.passes & DP_FILTER_VISIBILITY)) {
        DP_HIP(c, hipMemsetAsync(d_keep, 1, (size_t)n, s));
    }
    return DP_OK;
}

extern "C" int dp_filter_patches(dp_ctx *c, const dp_patch *patches, int64_t n, const dp_filter_options *fo,
                                 uint8_t *keep_out)
{
    if (!c || n < 0 || (n > 0 && (!patches || !keep_out)))
        return fail(c, DP_E_ARG, "dp_filter_patches: bad arguments");
    if (n == 0)
        return DP_OK;
    hipSetDevice(c->device);
    DP_HIP(c, c->f_pat.reserve((size_t)n));
    DP_HIP(c, c->f_keep.reserve((size_t)n));
    DP_HIP(c, hipMemcpyAsync(c->f_pat.p, patches, sizeof(dp_patch) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int rc = dp_filter_patches_device(c, c->f_pat.p, n, fo, c->f_keep.p, c->stream);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipMemcpyAsync(keep_out, c->f_keep.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

// ---------------------------------------------------------------------------
// the host forms of the batch entry points
// ---------------------------------------------------------------------------

// One host form, behind one wait: n_in records of `in` uploaded to `up` (in =
// null: the device form stages its own input), the device form queued by
// launch() on the context's stream, then n_out patches of `res` and, where
// asked for, as many accept flags of c->ok (reserved with flags) read back.
template <typename F>
static int staged_batch(dp_ctx *c, const dp_patch *in, size_t n_in, DevBuf<dp_patch> &up, DevBuf<dp_patch> &res,
                        size_t n_out, dp_patch *out, bool flags, uint8_t *accept_out, F launch)
{
    hipSetDevice(c->device);
    if (in)
        DP_HIP(c, up.reserve(n_in));
    DP_HIP(c, res.reserve(n_out));
    if (flags)
        DP_HIP(c, c->ok.reserve(n_out));
    if (in)
        DP_HIP(c, hipMemcpyAsync(up.p, in, sizeof(dp_patch) * n_in, hipMemcpyHostToDevice, c->stream));
    const int rc = launch();
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipMemcpyAsync(out, res.p, sizeof(dp_patch) * n_out, hipMemcpyDeviceToHost, c->stream));
    if (accept_out)
        DP_HIP(c, hipMemcpyAsync(accept_out, c->ok.p, n_out, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

// ---------------------------------------------------------------------------
// seeds: Seed::CreatePatchesFromPoints (seed.cpp:26-54) on the device
// ---------------------------------------------------------------------------

int seeds_device(dp_ctx *c, const double *xyz, int64_t n, dp_patch *d_out, hipStream_t s)
{
    DP_HIP(c, c->seedx.reserve((size_t)(3 * n)));
    DP_HIP(c, hipMemcpyAsync(c->seedx.p, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    DP_HIP(c, dpk::launch_seed_patches(c->d_views, c->V, c->seedx.p, n, c->opt.visible_angle,
                                       c->opt.candidate_angle, d_out, s));
    return DP_OK;
}

extern "C" int dp_seeds_to_patches(dp_ctx *c, const double *xyz, int n, dp_patch *out)
{
    if (!c || n < 0 || (n > 0 && (!xyz || !out)))
        return fail(c, DP_E_ARG, "dp_seeds_to_patches: bad arguments");
    if (!c->V)
        return fail(c, DP_E_STATE, "dp_seeds_to_patches: no views");
    if (n == 0)
        return DP_OK;
    return staged_batch(c, nullptr, 0, c->sconv, c->sconv, (size_t)n, out, false, nullptr,
                        [&] { return seeds_device(c, xyz, n, c->sconv.p, c->stream); });
}

// ---------------------------------------------------------------------------
// refine
// ---------------------------------------------------------------------------

dpk::RefineArgs refine_args(dp_ctx *c, const dpk::RefineJob &job)
{
    const int n = job.n;
    dpk::RefineArgs a{};
    a.views = c->d_views;
    a.V = c->V;
    a.cell = job.cell;
    a.mode = job.mode;
    a.n = n;
    a.opt = c->opt;
    a.patches = job.patches;
    a.accept = job.accept;
    a.work = c->d_work.p;
    a.evals = c->d_evals.p;
    a.parents = job.parents;
    a.parent0 = job.parent0;
    a.max_pops = job.max_pops;
    a.items = job.items;
    a.gen = job.gen;
    // the densify epilogue (the grid and its scale are read under epi only)
    a.epi = job.epi;
    a.seq0 = job.seq0;
    a.claim_grid = c->grid.p;
    a.grid_scale = (double)c->opt.grid_scale;
    a.img_base = c->img_base;
    a.narrow = c->narrow ? 1 : 0;
    // longest-first order (off in a context created with DP_NO_LPT=1, for A/B
    // timing and the order-independence test); without the scratch buffer the
    // kernel dequeues in index order
    if (!c->lpt_off && n > 0) {
        if (c->lpt.reserve((size_t)n + 2 * dpk::kLptBuckets) == hipSuccess) {
            a.order = c->lpt.p;
            a.order_scratch = c->lpt.p + n;
        } else {
            // the failed hipMalloc is recorded as the thread's last error: clear
            // it, or launch_refine's hipGetLastError() would report the
            // index-order launch that follows as failed
            (void)hipGetLastError();
        }
    }
    return a;
}

int densify_epi(const dp_ctx *c)
{
    return dpk::kEpiColor | (c->opt.max_patches_per_cell == 1 ? dpk::kEpiClaims : 0);
}

int launch_job(dp_ctx *c, const dpk::RefineJob &job, hipStream_t s)
{
    if (job.mode >= DP_MODE_FAST_EVAL)
        return dp_fast_launch(c, job, s);
    const dpk::RefineArgs a = refine_args(c, job);
    if (!job.parity_untimed)
        DP_HIP(c, hipEventRecord(c->e0, s));
    DP_HIP(c, dpk::launch_refine(a, s));
    if (!job.parity_untimed) {
        DP_HIP(c, hipEventRecord(c->e1, s));
        c->timed = true;
    }
    return DP_OK;
}

int check_refine(dp_ctx *c, int n, int cell, int mode)
{
    if (!c)
        return DP_E_ARG;
    if (!c->V)
        return fail(c, DP_E_STATE, "no views set");
    if (n < 0 || cell < 2 || cell > DP_MAX_CELL || mode < DP_MODE_EVAL || mode > DP_MODE_FAST_REFINE)
        return fail(c, DP_E_ARG, "refine: bad n/cell/mode");
    return DP_OK;
}

extern "C" int dp_refine_batch_device(dp_ctx *c, dp_patch *d_inout, int n, int cell, int mode,
                                      uint8_t *d_accept, void *stream)
{
    int rc = check_refine(c, n, cell, mode);
    if (rc != DP_OK)
        return rc;
    if (n == 0)
        return DP_OK;
    hipSetDevice(c->device);
    return launch_job(c, dpk::RefineJob{d_inout, d_accept, n, cell, mode}, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int dp_refine_batch(dp_ctx *c, dp_patch *inout, int n, int cell, int mode, uint8_t *accept_out)
{
    int rc = check_refine(c, n, cell, mode);
    if (rc != DP_OK)
        return rc;
    if (n == 0)
        return DP_OK;
    if (!inout)
        return fail(c, DP_E_ARG, "refine: null patches");
    for (int i = 0; i < n; ++i) {
        const dp_patch &p = inout[i];
        const bool bad_hi = c->V <= 64 ? (p.vis[1] != 0 || (c->V < 64 && (p.vis[0] >> c->V))) : (c->V < 128 && (p.vis[1] >> (c->V - 64)));
        if (p.ref >= (uint32_t)c->V || bad_hi)
            return fail(c, DP_E_ARG, "refine: patch " + std::to_string(i) + " names a view outside the scene");
    }
    return staged_batch(c, inout, (size_t)n, c->pat, c->pat, (size_t)n, inout, true, accept_out, [&] {
        return dp_refine_batch_device(c, c->pat.p, n, cell, mode, c->ok.p, c->stream);
    });
}

// Expand::ExpandPatch of n parents into their 4 n children on the engine
// `mode` names: the body of both expand families' device forms
static int expand_device(dp_ctx *c, const dp_patch *d_parents, int n, dp_patch *d_children, uint8_t *d_accept,
                         void *stream, int mode)
{
    hipSetDevice(c->device);
    dpk::RefineJob job{d_children, d_accept, 4 * n, c->opt.expand_cell_size, mode};
    job.parents = d_parents; // every parent expands (max_pops stays INT64_MAX)
    return launch_job(c, job, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int dp_expand_batch_device(dp_ctx *c, const dp_patch *d_parents, int n, dp_patch *d_children,
                                      uint8_t *d_accept, void *stream)
{
    int rc = check_refine(c, n, c ? c->opt.expand_cell_size : 11, DP_MODE_EXPAND);
    if (rc != DP_OK)
        return rc;
    if (n == 0)
        return DP_OK;
    if ((int64_t)n * 4 > INT32_MAX || !d_parents || !d_children)
        return fail(c, DP_E_ARG, "expand: bad arguments");
    return expand_device(c, d_parents, n, d_children, d_accept, stream, DP_MODE_EXPAND);
}

extern "C" int dp_expand_batch(dp_ctx *c, const dp_patch *parents, int n, dp_patch *children, uint8_t *accept_out)
{
    int rc = check_refine(c, n, c ? c->opt.expand_cell_size : 11, DP_MODE_EXPAND);
    if (rc != DP_OK)
        return rc;
    if (n == 0)
        return DP_OK;
    if (!parents || !children)
        return fail(c, DP_E_ARG, "expand: null arrays");
    return staged_batch(c, parents, (size_t)n, c->cand, c->pat, (size_t)4 * n, children, true, accept_out,
                        [&] { return dp_expand_batch_device(c, c->cand.p, n, c->pat.p, c->ok.p, c->stream); });
}

// the performance-mode expand family (its checks differ from the parity
// family's: the host form looks at the views only once it has work)
extern "C" int dp_fast_expand_batch_device(dp_ctx *c, const dp_patch *d_parents, int n, dp_patch *d_children,
                                           uint8_t *d_accept, void *stream)
{
    if (!c)
        return DP_E_ARG;
    if (!c->V)
        return fail(c, DP_E_STATE, "no views set");
    const int cell = c->opt.expand_cell_size;
    if (n < 0 || cell < 2 || cell > DP_MAX_CELL)
        return fail(c, DP_E_ARG, "fast expand: bad n/cell");
    if (n == 0)
        return DP_OK;
    if ((int64_t)n * 4 > INT32_MAX || !d_parents || !d_children)
        return fail(c, DP_E_ARG, "fast expand: bad arguments");
    return expand_device(c, d_parents, n, d_children, d_accept, stream, DP_MODE_FAST_REFINE);
}

extern "C" int dp_fast_expand_batch(dp_ctx *c, const dp_patch *parents, int n, dp_patch *children,
                                    uint8_t *accept_out)
{
    if (!c)
        return DP_E_ARG;
    if (n < 0)
        return fail(c, DP_E_ARG, "fast expand: bad n");
    if (n == 0)
        return DP_OK;
    if (!parents || !children)
        return fail(c, DP_E_ARG, "fast expand: null arrays");
    return staged_batch(c, parents, (size_t)n, c->cand, c->pat, (size_t)4 * n, children, true, accept_out,
                        [&] { return dp_fast_expand_batch_device(c, c->cand.p, n, c->pat.p, c->ok.p, c->stream); });
}

extern "C" int dp_eval_batch(dp_ctx *c, const dp_patch *in, int n, int cell, float *score_out)
{
    int rc = check_refine(c, n, cell, DP_MODE_EVAL);
    if (rc != DP_OK)
        return rc;
    if (n == 0)
        return DP_OK;
    if (!in || !score_out)
        return fail(c, DP_E_ARG, "eval: null arrays");
    std::vector<dp_patch> tmp(in, in + n);
    rc = dp_refine_batch(c, tmp.data(), n, cell, DP_MODE_EVAL, nullptr);
    if (rc != DP_OK)
        return rc;
    for (int i = 0; i < n; ++i)
        score_out[i] = tmp[i].score;
    return DP_OK;
}

extern "C" int dp_last_kernel_ms(dp_ctx *c, double *ms)
{
    if (!c || !ms)
        return DP_E_ARG;
    if (!c->timed)
        return fail(c, DP_E_STATE, "no kernel timed yet");
    DP_HIP(c, hipEventSynchronize(c->e1));
    float f = 0.f;
    DP_HIP(c, hipEventElapsedTime(&f, c->e0, c->e1));
    *ms = f;
    return DP_OK;
}

