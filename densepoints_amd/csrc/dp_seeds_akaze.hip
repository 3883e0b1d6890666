// dp_seeds_akaze.hip -- DetectorType::AKAZE of seed generation as host stages
// (the kernels are dp_akaze.hip; matcher.cpp:56-60 detect, 166-170 compute):
// the scale space, detector, FilterKeypoints and M-LDB per chunk of views (the
// chunk's planes fit DP_AKAZE_CHUNK_BYTES, 8 GiB by default); keypoints come
// out in (view, level, y, x) order, cells filtered as for ORB.
#include "dp_seedgen.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

using namespace dpk;

struct AkGeom {
    int n = 0;
    int w[kAkLevels], h[kAkLevels], octave[kAkLevels], ss[kAkLevels];
    float esigma[kAkLevels];
};

AkGeom akaze_geom(int W, int H)
{
    AkGeom g;
    for (int o = 0; o < 4; ++o) {
        const int w = W >> o, h = H >> o;
        if (o > 0 && (w < 80 || h < 40))
            break;
        for (int j = 0; j < 4; ++j) {
            g.w[g.n] = w;
            g.h[g.n] = h;
            g.octave[g.n] = o;
            g.esigma[g.n] = (float)(1.6 * std::pow(2.0, (double)j / 4.0 + (double)o));
            g.ss[g.n] = (int)std::lrint(g.esigma[g.n] * 1.5f / (float)(1 << o));
            ++g.n;
        }
    }
    return g;
}

// what every chunk of a run shares
struct AkRun {
    std::vector<AkGeom> geo;             // per view
    AkGeom full;                         // all 16 levels (esigma, ss, octave by level)
    std::vector<std::vector<float>> tau; // FED time steps per level (the same for every view)
    AkTaps g16, g10;
    int n_windows = 0;
    int64_t budget = 0; // bytes of planes per chunk
};

// the views [v0, v1) of one chunk and where their planes lie in the pools
struct AkChunk {
    int v0 = 0, v1 = 0, nv = 0;
    std::vector<AkPlane> planes; // [z * kAkLevels + level]
    std::vector<AkView> views;
    int64_t pool = 0, tmp = 0, det = 0, segs = 0; // floats of planes and of temporaries, pixels, row segments
    int mw[kAkLevels] = {0}, mh[kAkLevels] = {0}, nlev = 0; // launch extents per level (max over the views)
    AkArgs a{};
};

// the view sizes AKAZE takes, and the level geometry of each view -> run.geo
int akaze_geometry(dp_ctx *c, const std::vector<int32_t> &vw, const std::vector<int32_t> &vh, AkRun &run)
{
    const int V = c->V;
    for (int v = 0; v < V; ++v)
        if (vw[v] < 16 || vh[v] < 16)
            return fail(c, DP_E_ARG, "dp_generate_seeds: AKAZE needs views of at least 16 x 16 px");
    for (int v = 0; v < V; ++v) // a suppression-list key packs 14 bits of x and of y
        if (vw[v] > kAkMaxSide || vh[v] > kAkMaxSide)
            return fail(c, DP_E_ARG, "dp_generate_seeds: AKAZE takes views of at most 16383 x 16383 px");
    run.geo.resize(V);
    for (int v = 0; v < V; ++v)
        run.geo[v] = akaze_geom(vw[v], vh[v]);
    return DP_OK;
}

// dp_probe_akaze_plane: the probe's plane exists, its size (host only)
int akaze_probe_size(dp_ctx *c, const AkRun &run, SeedProbe *probe)
{
    const AkGeom &g = run.geo[probe->view];
    if (probe->level < 0 || probe->level >= g.n || probe->which < 0 || probe->which > 3)
        return fail(c, DP_E_ARG, "dp_probe_akaze_plane: no such level or plane");
    probe->w = g.w[probe->level];
    probe->h = g.h[probe->level];
    if (probe->out && probe->cap < (int64_t)probe->w * probe->h)
        return fail(c, DP_E_ARG, "dp_probe_akaze_plane: output too small");
    return DP_OK;
}

// the rest of run: the FED schedule, the descriptor's tables in s->akz_g25 /
// akz_bits, the Gaussian taps, the chunk budget
int akaze_tables(dp_ctx *c, dp_seedgen *s, AkRun &run)
{
    hipStream_t st = c->stream;
    run.full = akaze_geom(1 << 20, 1 << 20);
    run.tau.assign(kAkLevels, {});
    for (int i = 1; i < run.full.n; ++i) {
        const float e_prev = 0.5f * (run.full.esigma[i - 1] * run.full.esigma[i - 1]);
        const float e_cur = 0.5f * (run.full.esigma[i] * run.full.esigma[i]);
        float t[kAkMaxFed];
        const int n = akaze_fed_tau(e_cur - e_prev, 0.25f, t);
        if (n < 0)
            return fail(c, DP_E_ARG, "dp_generate_seeds: AKAZE FED schedule too long");
        run.tau[i].assign(t, t + n);
    }
    float g25[49];
    akaze_g25(g25);
    std::vector<uint32_t> bits(kAkBits);
    akaze_bit_pairs(bits.data());
    DP_HIP(c, s->akz_g25.reserve(49));
    DP_HIP(c, s->akz_bits.reserve(kAkBits));
    DP_HIP(c, hipMemcpyAsync(s->akz_g25.p, g25, sizeof(g25), hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemcpyAsync(s->akz_bits.p, bits.data(), kAkBits * 4, hipMemcpyHostToDevice, st));
    run.n_windows = akaze_windows();
    if (run.n_windows > 64)
        return fail(c, DP_E_ARG, "dp_generate_seeds: AKAZE orientation windows exceed a wave");
    auto taps_gauss = [](float sigma) {
        AkTaps t{};
        t.mode = 0;
        t.n = akaze_gauss_kernel(sigma, t.w);
        return t;
    };
    run.g16 = taps_gauss(1.6f);
    run.g10 = taps_gauss(1.0f);
    // chunk budget: DP_AKAZE_CHUNK_BYTES, else 40% of the free device memory
    const char *env = std::getenv("DP_AKAZE_CHUNK_BYTES");
    run.budget = (int64_t)8 << 30;
    if (env) {
        run.budget = std::max<int64_t>(1, std::atoll(env));
    } else {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0)
            run.budget = (int64_t)(0.4 * (double)fr);
    }
    return DP_OK;
}

// The chunk that starts at view v0: as many views as fit the budget (one at
// least), the plane, det and segment offsets of each -> ch, with its tables in
// s->akz_planes / akz_views, the pools sized and the per-view maxima zeroed.
int akaze_plan_chunk(dp_ctx *c, dp_seedgen *s, const AkRun &run, const std::vector<int32_t> &vw,
                     const std::vector<int32_t> &vh, int v0, AkChunk &ch)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    auto view_bytes = [&](int v) {
        int64_t px = 0;
        for (int i = 0; i < run.geo[v].n; ++i)
            px += (int64_t)run.geo[v].w[i] * run.geo[v].h[i];
        return 16 * px + 20 * (int64_t)vw[v] * vh[v] + 8 * (px / 16);
    };
    int v1 = v0;
    int64_t bytes = 0;
    while (v1 < V && (v1 == v0 || bytes + view_bytes(v1) <= run.budget)) {
        bytes += view_bytes(v1);
        ++v1;
    }
    ch = AkChunk{};
    ch.v0 = v0;
    ch.v1 = v1;
    const int nv = ch.nv = v1 - v0;
    ch.planes.resize((size_t)nv * kAkLevels);
    ch.views.resize(nv);
    std::memset(ch.planes.data(), 0, ch.planes.size() * sizeof(AkPlane));
    for (int z = 0; z < nv; ++z) {
        const int v = v0 + z;
        const AkGeom &g = run.geo[v];
        for (int i = 0; i < g.n; ++i) {
            AkPlane &P = ch.planes[(size_t)z * kAkLevels + i];
            P.off = ch.pool;
            P.det_base = ch.det;
            P.seg_base = ch.segs;
            P.w = g.w[i];
            P.h = g.h[i];
            P.octave = g.octave[i];
            P.sigma_size = g.ss[i];
            P.esigma = g.esigma[i];
            ch.pool += 4 * (int64_t)P.w * P.h;
            ch.det += (int64_t)P.w * P.h;
            ch.segs += (int64_t)P.h * ((P.w + 255) / 256);
            ch.mw[i] = std::max(ch.mw[i], P.w);
            ch.mh[i] = std::max(ch.mh[i], P.h);
        }
        ch.nlev = std::max(ch.nlev, g.n);
        const PyrPlane &pl = c->planes[0][v];
        AkView &view = ch.views[z];
        view.bgra = pl.img;
        view.pitch = pl.pitch;
        view.w0 = vw[v];
        view.h0 = vh[v];
        view.view = v;
        view.tmp = ch.tmp;
        view.n0 = (int64_t)vw[v] * vh[v];
        ch.tmp += 5 * view.n0;
    }
    if (ch.det >= INT32_MAX)
        return fail(c, DP_E_ARG, "dp_generate_seeds: AKAZE chunk above 2^31 pixels (lower DP_AKAZE_CHUNK_BYTES)");
    DP_HIP(c, s->akz_pool.reserve(ch.pool + 1));
    DP_HIP(c, s->akz_tmp.reserve(ch.tmp + 1));
    DP_HIP(c, s->akz_planes.reserve(ch.planes.size()));
    DP_HIP(c, s->akz_views.reserve(nv));
    DP_HIP(c, s->akz_hmax.reserve(nv));
    DP_HIP(c, s->akz_hist.reserve((size_t)nv * 301));
    DP_HIP(c, s->akz_k0.reserve(nv));
    DP_HIP(c, s->akz_seg.reserve(2 * (ch.segs + 1) + 8 * ch.segs)); // counts, offsets, 4 u64 ballots per segment
    DP_HIP(c, hipMemcpyAsync(s->akz_planes.p, ch.planes.data(), ch.planes.size() * sizeof(AkPlane),
                             hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemcpyAsync(s->akz_views.p, ch.views.data(), nv * sizeof(AkView), hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemsetAsync(s->akz_hmax.p, 0, nv * 4, st));
    DP_HIP(c, hipMemsetAsync(s->akz_hist.p, 0, (size_t)nv * 301 * 4, st));
    ch.a = AkArgs{s->akz_planes.p, s->akz_views.p, s->akz_pool.p, s->akz_tmp.p, s->akz_hmax.p, s->akz_hist.p,
                  s->akz_k0.p};
    return DP_OK;
}

// the detector's derivatives of level i's Lsmooth (plane ls): Ldet; Lx, Ly scaled
hipError_t akaze_deriv(const AkRun &run, const AkChunk &ch, int i, int ls, hipStream_t st)
{
    const AkArgs &a = ch.a;
    const int nv = ch.nv, mw = ch.mw[i], mh = ch.mh[i];
    if (run.full.ss[i] >= 1 && run.full.ss[i] <= 4)
        return launch_akz_deriv(a, i, ls, run.full.ss[i], nv, mw, mh, st);
    hipError_t e = launch_akz_rows2(a, i, ls, kT1, kT2, 0, nv, mw, mh, st);
    if (e == hipSuccess)
        e = launch_akz_cols2(a, i, kT1, kLx, kT2, kLy, 0, nv, mw, mh, st);
    if (e == hipSuccess)
        e = launch_akz_rows2(a, i, kLx, kT1, kT2, 0, nv, mw, mh, st);
    if (e == hipSuccess)
        e = launch_akz_rows2(a, i, kLy, -1, kT4, 0, nv, mw, mh, st);
    if (e == hipSuccess)
        e = launch_akz_cols_det(a, i, nv, mw, mh, st);
    return e;
}

// The scale space of a planned chunk: Lt, Lx, Ly, Ldet of every level of its
// views in s->akz_pool (the image stage: a probe reads its plane from there).
int akaze_scale_space(dp_ctx *c, dp_seedgen *s, const AkRun &run, const AkChunk &ch)
{
    hipStream_t st = c->stream;
    const AkArgs &a = ch.a;
    const int nv = ch.nv;
    const int *mw = ch.mw, *mh = ch.mh;
    // level 0: gray, L0 = Gaussian(img, 1.6), the contrast factor from the
    // unnormalised Scharr gradient of Gaussian(img, 1) (x in T0, y in T4)
    DP_HIP(c, launch_akz_gray(a, nv, mw[0], mh[0], st));
    DP_HIP(c, launch_akz_gauss2(a, 0, kT0, kLt, run.g16, nv, mw[0], mh[0], st));
    DP_HIP(c, akaze_deriv(run, ch, 0, kLt, st));
    DP_HIP(c, launch_akz_contrast(a, run.g10, nv, mw[0], mh[0], st));
    // FED steps per launch: 4 (config 3, 32 views, 64 x 16 tiles: 44.9 / 41.9 /
    // 40.8 / 40.7 / 41.1 ms detect at 2 / 3 / 4 / 5 / 6); DP_AKAZE_FED_STEPS
    // (1 .. kAkFedPerLaunch) for A/B timing -- every grouping gives the same values
    int fed_k = 4;
    if (const char *fk = std::getenv("DP_AKAZE_FED_STEPS"))
        fed_k = std::max(1, std::min(kAkFedPerLaunch, std::atoi(fk)));
    for (int i = 1; i < ch.nlev; ++i) {
        // the level starts from the previous level's Lt (read in place) or its
        // half-sample; the FED steps ping-pong between T2 and Lt with the
        // parity that ends in Lt (no copies)
        const std::vector<float> &tau = run.tau[i];
        const int nt = (int)tau.size();
        const int nl = (nt + fed_k - 1) / fed_k; // launches
        int src = kPrevLt;
        if (run.full.octave[i] > run.full.octave[i - 1]) {
            src = nl % 2 ? kT2 : kLt;
            DP_HIP(c, launch_akz_half(a, i, src, nv, mw[i], mh[i], st));
        }
        // Lsmooth (T3), g2 conductance (T4) from its unnormalised Scharr gradient
        DP_HIP(c, launch_akz_flow(a, i, src, run.g10, nv, mw[i], mh[i], st));
        // the steps in nl near-equal groups of at most fed_k
        for (int k = 0, j = 0; j < nl; ++j) {
            const int dst = (nl - 1 - j) % 2 ? kT2 : kLt;
            const int g = (nt - k) / (nl - j) + ((nt - k) % (nl - j) ? 1 : 0);
            DP_HIP(c, launch_akz_fedk(a, i, src, dst, tau.data() + k, g, nv, mw[i], mh[i], st));
            k += g;
            src = dst;
        }
        if (src != kLt)
            DP_HIP(c, launch_akz_copy(a, i, src, kLt, nv, mw[i], mh[i], st));
        DP_HIP(c, akaze_deriv(run, ch, i, kT3, st));
    }
    return DP_OK;
}

// dp_probe_akaze_plane: the probe's plane out of a chunk that holds its view
int akaze_probe_copy(dp_ctx *c, dp_seedgen *s, const AkChunk &ch, SeedProbe *probe)
{
    const AkPlane &P = ch.planes[(size_t)(probe->view - ch.v0) * kAkLevels + probe->level];
    const int64_t n = (int64_t)P.w * P.h;
    DP_HIP(c, hipMemcpyAsync(probe->out, s->akz_pool.p + P.off + probe->which * n, n * sizeof(float),
                             hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

// The keypoints of a chunk's scale space, in (view, level, y, x) order, into
// s->kp_a / kv_a; returns how many (or a negative status).  Extrema candidates
// per (row, 256-px segment) are counted, scanned and emitted, then suppressed
// across scales and levels.  Two host waits.
int64_t akaze_extrema(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const AkChunk &ch)
{
    hipStream_t st = c->stream;
    const AkArgs &a = ch.a;
    const int nv = ch.nv;
    const int64_t segs = ch.segs;
    uint32_t *seg_cnt = s->akz_seg.p, *seg_off = s->akz_seg.p + segs + 1;
    auto *seg_mask = reinterpret_cast<unsigned long long *>(s->akz_seg.p + 2 * (segs + 1));
    DP_HIP(c, hipMemsetAsync(seg_cnt, 0, (size_t)(segs + 1) * 4, st));
    for (int i = 0; i < ch.nlev; ++i)
        DP_HIP(c, launch_akz_count(a, i, mo.akaze_threshold, seg_cnt, seg_mask, nv, ch.mw[i], ch.mh[i], st));
    DP_CUB(c, s, hipcub::DeviceScan::ExclusiveSum(_tmp, _bytes, seg_cnt, seg_off, (int)(segs + 1), st));
    uint32_t n_cand32 = 0;
    DP_HIP(c, hipMemcpyAsync(&n_cand32, seg_off + segs, 4, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipStreamSynchronize(st));
    const int64_t n_cand = n_cand32;
    DP_HIP(c, s->akz_cand.reserve(n_cand + 1));
    for (int i = 0; i < ch.nlev; ++i)
        DP_HIP(c, launch_akz_emit(a, i, seg_mask, seg_off, s->akz_cand.p, nv, ch.mw[i], ch.mh[i], st));
    std::vector<int32_t> vids(nv);
    for (int z = 0; z < nv; ++z)
        vids[z] = ch.v0 + z;
    DP_HIP(c, s->akz_vids.reserve(nv));
    if (n_cand > kAkListCap) // only then can a view's list outgrow LDS
        DP_HIP(c, s->akz_spill.reserve(n_cand));
    DP_HIP(c, hipMemcpyAsync(s->akz_vids.p, vids.data(), nv * 4, hipMemcpyHostToDevice, st));
    DP_HIP(c, s->kp_a.reserve(n_cand + 1));
    DP_HIP(c, s->kv_a.reserve(n_cand + 1));
    DP_HIP(c, s->kp_b.reserve(n_cand + 1));
    DP_HIP(c, s->kv_b.reserve(n_cand + 1));
    DP_HIP(c, s->flag.reserve(n_cand + 1));
    DP_HIP(c, s->idx_a.reserve(n_cand + 1));
    AkCandArgs ca{s->akz_planes.p, s->akz_pool.p, s->akz_cand.p, n_cand, nv, s->akz_vids.p, s->kp_b.p,
                  s->kv_b.p, s->flag.p, s->akz_spill.p};
    DP_HIP(c, launch_akz_candidates(ca, st));
    const int64_t n_det =
        select_flagged(c, s, hipcub::CountingInputIterator<int32_t>(0), s->flag.p, s->idx_a.p, n_cand);
    if (n_det < 0)
        return n_det;
    DP_HIP(c, launch_gather_kp(s->kp_b.p, s->kv_b.p, s->idx_a.p, n_det, s->kp_a.p, s->kv_a.p, st));
    return n_det;
}

// M-LDB of a chunk's n_f filtered keypoints (s->kp_b / kv_b) -> s->desc, and
// the three appended to the host lists (s->h_kp, s->h_kv, all_desc).  One
// host wait: the next chunk reuses the device buffers.
int akaze_describe_append(dp_ctx *c, dp_seedgen *s, const AkRun &run, const AkChunk &ch, int64_t n_f,
                          std::vector<uint32_t> &all_desc)
{
    hipStream_t st = c->stream;
    DP_HIP(c, s->desc.reserve((size_t)(n_f + 1) * kAkDescWords));
    AkDescArgs da{s->akz_planes.p, s->akz_pool.p, s->kv_b.p, ch.v0, s->kp_b.p, n_f, s->akz_g25.p, s->akz_bits.p,
                  run.n_windows, s->desc.p};
    DP_HIP(c, launch_akz_describe(da, st));
    const size_t k0 = s->h_kp.size();
    s->h_kp.resize(k0 + n_f);
    s->h_kv.resize(k0 + n_f);
    all_desc.resize((k0 + n_f) * kAkDescWords);
    DP_HIP(c, hipMemcpyAsync(s->h_kp.data() + k0, s->kp_b.p, n_f * sizeof(dp_keypoint), hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(s->h_kv.data() + k0, s->kv_b.p, n_f * 4, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(all_desc.data() + k0 * kAkDescWords, s->desc.p, n_f * kAkDescWords * 4,
                             hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipStreamSynchronize(st));
    return DP_OK;
}

// the host lists of all chunks back into s->kp_b / kv_b / desc
int akaze_upload(dp_ctx *c, dp_seedgen *s, const std::vector<uint32_t> &all_desc)
{
    hipStream_t st = c->stream;
    const int64_t n = (int64_t)s->h_kp.size();
    DP_HIP(c, s->kp_b.reserve(n + 1));
    DP_HIP(c, s->kv_b.reserve(n + 1));
    DP_HIP(c, s->desc.reserve((size_t)(n + 1) * kAkDescWords));
    if (n > 0) {
        DP_HIP(c, hipMemcpyAsync(s->kp_b.p, s->h_kp.data(), n * sizeof(dp_keypoint), hipMemcpyHostToDevice, st));
        DP_HIP(c, hipMemcpyAsync(s->kv_b.p, s->h_kv.data(), n * 4, hipMemcpyHostToDevice, st));
        DP_HIP(c, hipMemcpyAsync(s->desc.p, all_desc.data(), n * kAkDescWords * 4, hipMemcpyHostToDevice, st));
    }
    return DP_OK;
}

} // namespace

int akaze_detect(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                 const std::vector<int32_t> &vh, Detected &det, SeedProbe *probe)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    s->desc_words = kAkDescWords;
    AkRun run;
    int rc = akaze_geometry(c, vw, vh, run);
    if (rc != DP_OK)
        return rc;
    if (probe) { // a size-only query ends here, before any device work
        rc = akaze_probe_size(c, run, probe);
        if (rc != DP_OK || !probe->out)
            return rc;
    }
    rc = akaze_tables(c, s, run);
    if (rc != DP_OK)
        return rc;
    std::vector<uint32_t> all_desc;
    s->h_kp.clear();
    s->h_kv.clear();
    bool e1_done = false;
    DP_HIP(c, hipEventRecord(det.e0, st));
    AkChunk ch;
    for (int v0 = 0; v0 < V; v0 = ch.v1) {
        rc = akaze_plan_chunk(c, s, run, vw, vh, v0, ch);
        if (rc == DP_OK)
            rc = akaze_scale_space(c, s, run, ch);
        if (rc != DP_OK)
            return rc;
        if (probe) { // the image stage is all a probe runs, up to the chunk of its view
            if (probe->view >= ch.v1)
                continue;
            return akaze_probe_copy(c, s, ch, probe);
        }
        const int64_t n_det = akaze_extrema(c, s, mo, ch);
        if (n_det < 0)
            return (int)n_det;
        det.keypoints_detected += n_det;
        int64_t n_f = 0;
        rc = cell_filter(c, s, mo, vw, vh, n_det, &n_f);
        if (rc != DP_OK)
            return rc;
        if (ch.v0 == 0 && ch.v1 == V) { // one chunk: detection ends here; else after the last
            DP_HIP(c, hipEventRecord(det.e1, st));
            e1_done = true;
        }
        rc = akaze_describe_append(c, s, run, ch, n_f, all_desc);
        if (rc != DP_OK)
            return rc;
    }
    if (!e1_done)
        DP_HIP(c, hipEventRecord(det.e1, st));
    rc = akaze_upload(c, s, all_desc);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipEventRecord(det.e2, st));
    DP_HIP(c, hipStreamSynchronize(st));
    det.n = (int64_t)s->h_kp.size();
    return DP_OK;
}
