// dp_seeds_orb.hip -- DetectorType::ORB of seed generation as host stages
// (the kernels are dp_orb.hip): DetectKeypoints (matcher.cpp:45-87),
// FilterKeypoints and ComputeDescriptors (matcher.cpp:155-183).
#include "dp_seedgen.h"

#include <algorithm>
#include <cmath>

namespace {

// the pyramid of every view as the host planned it; g names its device form
struct OrbPyr {
    int V = 0, L = 0;
    std::vector<dpk::OrbLevel> lv; // [v * L + l]
    std::vector<int> lw, lh;       // per-level launch extents (max over views)
    int max_w = 0, max_h = 0;
    int64_t pool = 0, rows = 0;    // gray pixels and rows of all levels
    dpk::OrbGeom g{};
};

// ORB_Impl's pyramid geometry (layerScale, level sizes, features per level)
// -> py, its table in s->lv, the level-0 planes in s->planes0, and the gray
// levels in s->gray.  Records e0 before the first kernel.
int orb_pyramid(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                const std::vector<int32_t> &vh, hipEvent_t e0, OrbPyr &py)
{
    hipStream_t st = c->stream;
    const int V = py.V = c->V, L = py.L = mo.n_levels;
    std::vector<int32_t> nfeat(L);
    dpk::orb_features_per_level(mo.n_features, mo.scale_factor, L, nfeat.data());
    py.lv.resize((size_t)V * L);
    py.lw.assign(L, 0);
    py.lh.assign(L, 0);
    for (int v = 0; v < V; ++v) {
        for (int l = 0; l < L; ++l) {
            const float sc = (float)std::pow(mo.scale_factor, (double)l);
            dpk::OrbLevel &o = py.lv[(size_t)v * L + l];
            o.scale = sc;
            o.w = l == 0 ? vw[v] : (int)std::lrint((float)vw[v] / sc);
            o.h = l == 0 ? vh[v] : (int)std::lrint((float)vh[v] / sc);
            if (o.w < 4 || o.h < 4)
                return fail(c, DP_E_ARG, "dp_generate_seeds: pyramid level smaller than 4 px (reduce n_levels)");
            // INTER_LINEAR's inverse scale, once per level instead of per pixel
            o.rsx = l == 0 ? 0.0 : 1.0 / ((double)o.w / (double)py.lv[(size_t)v * L + l - 1].w);
            o.rsy = l == 0 ? 0.0 : 1.0 / ((double)o.h / (double)py.lv[(size_t)v * L + l - 1].h);
            o.off = py.pool;
            o.row0 = py.rows;
            o.nfeat = nfeat[l];
            py.pool += (int64_t)o.w * o.h;
            py.rows += o.h;
            py.max_w = std::max(py.max_w, o.w);
            py.max_h = std::max(py.max_h, o.h);
            py.lw[l] = std::max(py.lw[l], o.w);
            py.lh[l] = std::max(py.lh[l], o.h);
        }
    }
    DP_HIP(c, s->lv.reserve(py.lv.size()));
    DP_HIP(c, hipMemcpyAsync(s->lv.p, py.lv.data(), py.lv.size() * sizeof(dpk::OrbLevel), hipMemcpyHostToDevice, st));
    DP_HIP(c, s->planes0.reserve(V));
    DP_HIP(c, hipMemcpyAsync(s->planes0.p, c->planes[0].data(), (size_t)V * sizeof(dpk::PyrPlane), hipMemcpyHostToDevice,
                             st));
    DP_HIP(c, s->gray.reserve(py.pool));
    DP_HIP(c, s->score.reserve(py.pool));
    DP_HIP(c, s->row_cnt.reserve(py.rows + 1));
    DP_HIP(c, s->row_off.reserve(py.rows + 1));
    py.g = dpk::OrbGeom{s->lv.p, V, L, s->gray.p};

    DP_HIP(c, hipEventRecord(e0, st));
    DP_HIP(c, dpk::launch_orb_gray(s->planes0.p, py.g, py.lv[0].w > 0 ? py.max_w : 0, py.max_h, st));
    for (int l = 1; l < L; ++l)
        DP_HIP(c, dpk::launch_orb_resize(py.g, l, py.lw[l], py.lh[l], st));
    return DP_OK;
}

// dp_probe_orb_level: the size of one gray level of py and, asked for, its pixels
int orb_probe_level(dp_ctx *c, dp_seedgen *s, const OrbPyr &py, SeedProbe *probe)
{
    const dpk::OrbLevel &o = py.lv[(size_t)probe->view * py.L + probe->level];
    probe->w = o.w;
    probe->h = o.h;
    if (!probe->out)
        return DP_OK;
    if (probe->cap < (int64_t)o.w * o.h)
        return fail(c, DP_E_ARG, "dp_probe_orb_level: output too small");
    DP_HIP(c, hipMemcpyAsync(probe->out, s->gray.p + o.off, (size_t)o.w * o.h, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

// FAST scores of the gray levels (s->score), then the non-maximum suppression
// twice: counts per row, their scan, the *n_cand survivors in (view, level,
// y, x) order in s->cand.  One host wait.
int orb_candidates(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const OrbPyr &py, int64_t *n_cand)
{
    hipStream_t st = c->stream;
    const int L = py.L;
    const int64_t rows = py.rows;
    for (int l = 0; l < L; ++l)
        DP_HIP(c, dpk::launch_orb_fast(py.g, l, mo.fast_threshold, s->score.p, py.lw[l], py.lh[l], st));
    DP_HIP(c, hipMemsetAsync(s->row_cnt.p, 0, (size_t)(rows + 1) * sizeof(int64_t), st));
    // row counts as int32 into the low half of an int64 buffer would alias: count into idx_a
    DP_HIP(c, s->idx_a.reserve(rows + 1));
    DP_HIP(c, hipMemsetAsync(s->idx_a.p, 0, (size_t)(rows + 1) * sizeof(int32_t), st));
    for (int l = 0; l < L; ++l)
        DP_HIP(c, dpk::launch_orb_nms(py.g, l, s->score.p, mo.edge_threshold, nullptr, s->idx_a.p, nullptr, py.lh[l],
                                      st));
    DP_CUB(c, s, hipcub::DeviceScan::ExclusiveSum(_tmp, _bytes, s->idx_a.p, s->row_off.p, (int)(rows + 1), st));
    *n_cand = 0;
    DP_HIP(c, hipMemcpyAsync(n_cand, s->row_off.p + rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipStreamSynchronize(st));
    DP_HIP(c, s->cand.reserve(*n_cand + 1));
    DP_HIP(c, s->cand2.reserve(*n_cand + 1));
    DP_HIP(c, s->flag.reserve(*n_cand + 1));
    for (int l = 0; l < L; ++l)
        DP_HIP(c, dpk::launch_orb_nms(py.g, l, s->score.p, mo.edge_threshold, s->row_off.p, nullptr, s->cand.p,
                                      py.lh[l], st));
    return DP_OK;
}

// retainBest(2 n_l) by FAST score: s->cand (n_cand) -> s->cand2 (the count
// returned, or a negative status).  One host wait.
int64_t orb_retain_fast(dp_ctx *c, dp_seedgen *s, const OrbPyr &py, int64_t n_cand)
{
    hipStream_t st = c->stream;
    const int nseg = py.V * py.L;
    DP_HIP(c, s->hist.reserve((size_t)nseg * 256));
    DP_HIP(c, hipMemsetAsync(s->hist.p, 0, (size_t)nseg * 256 * 4, st));
    DP_HIP(c, s->fthr.reserve(nseg));
    DP_HIP(c, dpk::launch_orb_hist(s->cand.p, n_cand, s->hist.p, st));
    DP_HIP(c, dpk::launch_orb_fast_thresh(py.g, s->hist.p, s->fthr.p, st));
    DP_HIP(c, dpk::launch_orb_flag_fast(s->cand.p, n_cand, s->fthr.p, s->flag.p, st));
    return select_flagged(c, s, s->cand.p, s->flag.p, s->cand2.p, n_cand);
}

// Harris responses and retainBest(n_l) by them: s->cand2 (n2) -> s->cand (the
// count returned, or a negative status).  One host wait.
int64_t orb_retain_harris(dp_ctx *c, dp_seedgen *s, const OrbPyr &py, int64_t n2)
{
    hipStream_t st = c->stream;
    const int nseg = py.V * py.L;
    DP_HIP(c, s->hkey.reserve(n2 + 1));
    DP_HIP(c, s->hkey_sorted.reserve(n2 + 1));
    DP_HIP(c, s->seg_cnt.reserve(nseg + 1));
    DP_HIP(c, s->seg_off.reserve(nseg + 1));
    DP_HIP(c, s->seg_off32.reserve(nseg + 1));
    DP_HIP(c, s->hthr.reserve(nseg));
    DP_HIP(c, s->keep_all.reserve(nseg));
    DP_HIP(c, hipMemsetAsync(s->seg_cnt.p, 0, (size_t)(nseg + 1) * 4, st));
    DP_HIP(c, dpk::launch_orb_harris(py.g, s->cand2.p, n2, s->hkey.p, s->seg_cnt.p, st));
    DP_CUB(c, s, hipcub::DeviceScan::ExclusiveSum(_tmp, _bytes, s->seg_cnt.p, s->seg_off32.p, nseg + 1, st));
    DP_CUB(c, s, hipcub::DeviceScan::ExclusiveSum(_tmp, _bytes, s->seg_cnt.p, s->seg_off.p, nseg + 1, st));
    if (n2 > 0)
        DP_CUB(c, s, hipcub::DeviceSegmentedRadixSort::SortKeys(_tmp, _bytes, s->hkey.p, s->hkey_sorted.p, (int)n2, nseg,
                                                                 s->seg_off32.p, s->seg_off32.p + 1, 0, 32, st));
    DP_HIP(c, dpk::launch_orb_harris_thresh(py.g, s->hkey_sorted.p, s->seg_off.p, s->hthr.p, s->keep_all.p, st));
    DP_HIP(c, dpk::launch_orb_flag_harris(s->cand2.p, n2, s->hthr.p, s->keep_all.p, s->flag.p, st));
    return select_flagged(c, s, s->cand2.p, s->flag.p, s->cand.p, n2);
}

// angles and level-0 coordinates: s->cand (n3) -> s->kp_a / kv_a
int orb_angle(dp_ctx *c, dp_seedgen *s, const OrbPyr &py, int64_t n3)
{
    hipStream_t st = c->stream;
    std::vector<int32_t> umax(dpk::kOrbHalfPatch + 2);
    dpk::orb_umax(umax.data());
    DP_HIP(c, s->umax.reserve(umax.size()));
    DP_HIP(c, hipMemcpyAsync(s->umax.p, umax.data(), umax.size() * 4, hipMemcpyHostToDevice, st));
    DP_HIP(c, s->kp_a.reserve(n3 + 1));
    DP_HIP(c, s->kp_b.reserve(n3 + 1));
    DP_HIP(c, s->kv_a.reserve(n3 + 1));
    DP_HIP(c, s->kv_b.reserve(n3 + 1));
    DP_HIP(c, dpk::launch_orb_angle(py.g, s->cand.p, n3, s->umax.p, s->kp_a.p, s->kv_a.p, st));
    return DP_OK;
}

// runByImageBorder, then the stable order by octave: s->kp_b / kv_b (n4) ->
// the same in their final order (the count returned, or a negative status),
// their copies to s->h_kp / h_kv queued.  One host wait.
int64_t orb_border_octave(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                          const std::vector<int32_t> &vh, int64_t n4)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    DP_HIP(c, s->vw.reserve(V));
    DP_HIP(c, s->vh.reserve(V));
    DP_HIP(c, hipMemcpyAsync(s->vw.p, vw.data(), V * 4, hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemcpyAsync(s->vh.p, vh.data(), V * 4, hipMemcpyHostToDevice, st));
    DP_HIP(c, s->okey.reserve(n4 + 1));
    DP_HIP(c, s->okey_sorted.reserve(n4 + 1));
    DP_HIP(c, dpk::launch_desc_prep(s->kp_b.p, s->kv_b.p, s->vw.p, s->vh.p, n4, mo.edge_threshold, s->flag.p,
                                    s->okey.p, st));
    const int64_t n5 =
        select_flagged(c, s, hipcub::CountingInputIterator<int32_t>(0), s->flag.p, s->idx_a.p, n4);
    if (n5 < 0)
        return n5;
    DP_HIP(c, dpk::launch_gather_kp(s->kp_b.p, s->kv_b.p, s->idx_a.p, n5, s->kp_a.p, s->kv_a.p, st));
    DP_HIP(c, dpk::launch_desc_prep(s->kp_a.p, s->kv_a.p, s->vw.p, s->vh.p, n5, mo.edge_threshold, s->flag.p,
                                    s->okey.p, st));
    DP_HIP(c, dpk::launch_iota(s->idx_a.p, n5, st));
    if (n5 > 0)
        DP_CUB(c, s, hipcub::DeviceRadixSort::SortPairs(_tmp, _bytes, s->okey.p, s->okey_sorted.p, s->idx_a.p,
                                                         s->idx_b.p, (int)n5, 0, 16, st));
    DP_HIP(c, dpk::launch_gather_kp(s->kp_a.p, s->kv_a.p, s->idx_b.p, n5, s->kp_b.p, s->kv_b.p, st));
    s->h_kp.resize(n5);
    s->h_kv.resize(n5);
    DP_HIP(c, hipMemcpyAsync(s->h_kp.data(), s->kp_b.p, n5 * sizeof(dp_keypoint), hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(s->h_kv.data(), s->kv_b.p, n5 * 4, hipMemcpyDeviceToHost, st));
    return n5;
}

// rBRIEF of s->kp_b / kv_b (n5) on the gray levels -> s->desc (8 dwords each)
int orb_describe(dp_ctx *c, dp_seedgen *s, const OrbPyr &py, int64_t n5)
{
    hipStream_t st = c->stream;
    std::vector<int8_t> pat(4 * dpk::kOrbPatternPairs);
    dpk::orb_pattern(pat.data());
    DP_HIP(c, s->pattern.reserve(pat.size()));
    DP_HIP(c, hipMemcpyAsync(s->pattern.p, pat.data(), pat.size(), hipMemcpyHostToDevice, st));
    DP_HIP(c, s->desc.reserve((size_t)(n5 + 1) * 8));
    DP_HIP(c, dpk::launch_orb_desc(py.g, s->kp_b.p, s->kv_b.p, n5, s->pattern.p, s->desc.p, st));
    return DP_OK;
}

} // namespace

int orb_detect(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
               const std::vector<int32_t> &vh, Detected &det, SeedProbe *probe)
{
    hipStream_t st = c->stream;
    s->desc_words = 8;
    OrbPyr py;
    int rc = orb_pyramid(c, s, mo, vw, vh, det.e0, py);
    if (rc != DP_OK)
        return rc;
    if (probe)
        return orb_probe_level(c, s, py, probe);
    int64_t n_cand = 0;
    rc = orb_candidates(c, s, mo, py, &n_cand);
    if (rc != DP_OK)
        return rc;
    const int64_t n2 = orb_retain_fast(c, s, py, n_cand);
    if (n2 < 0)
        return (int)n2;
    const int64_t n3 = orb_retain_harris(c, s, py, n2);
    if (n3 < 0)
        return (int)n3;
    rc = orb_angle(c, s, py, n3);
    if (rc != DP_OK)
        return rc;
    det.keypoints_detected = n3;
    int64_t n4 = 0;
    rc = cell_filter(c, s, mo, vw, vh, n3, &n4);
    if (rc != DP_OK)
        return rc;
    det.n = orb_border_octave(c, s, mo, vw, vh, n4);
    if (det.n < 0)
        return (int)det.n;
    DP_HIP(c, hipEventRecord(det.e1, st));
    rc = orb_describe(c, s, py, det.n);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipEventRecord(det.e2, st));
    DP_HIP(c, hipStreamSynchronize(st));
    return DP_OK;
}
