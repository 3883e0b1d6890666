// dp_seedgen.h -- state and stages of seed generation, shared by its host
// files: dp_seeds_capi.hip (the C entry points, the standalone operators and
// the stages both detectors share), dp_seeds_orb.hip and dp_seeds_akaze.hip
// (the detectors).  A stage is a function on (context, state): its comment
// names the members of dp_seedgen it reads and leaves behind.
#pragma once

#include "dp_akaze.h"
#include "dp_ctx.h"
#include "dp_orb.h"
#include "dp_seeds.h"

#include <hipcub/hipcub.hpp>

#include <vector>

// seed-generation state owned by the context (every member frees itself)
struct dp_seedgen {
    // scratch of the standalone operators
    DevBuf<uint32_t> desc, keys;
    DevBuf<int32_t> i2, d2, off;
    DevBuf<double> P, obs, X;
    DevBuf<dpk::KnnJob> jobs;
    DevBuf<dpk::KnnBlock> blocks;
    DevBuf<uint32_t> pkeys; // per-split partial top-2 keys
    // GenerateSeeds
    DevBuf<dpk::OrbLevel> lv;
    DevBuf<dpk::PyrPlane> planes0;
    DevBuf<uint8_t> gray, score;
    DevBuf<int64_t> row_cnt, row_off;
    DevBuf<dpk::OrbCand> cand, cand2;
    DevBuf<uint32_t> hist, hkey, hkey_sorted, seg_cnt;
    DevBuf<int32_t> seg_off32, fthr, umax;
    DevBuf<int64_t> seg_off;
    DevBuf<float> hthr;
    DevBuf<uint8_t> keep_all, flag;
    DevBuf<dp_keypoint> kp_a, kp_b;
    DevBuf<int32_t> kv_a, kv_b, idx_a, idx_b, gcols, vw, vh;
    DevBuf<int64_t> cell_off;
    DevBuf<uint32_t> cell_cnt, okey, okey_sorted;
    DevBuf<uint64_t> ckey, ckey_sorted;
    DevBuf<int8_t> pattern;
    DevBuf<unsigned char> cub_tmp;
    DevBuf<int64_t> n_sel;
    DevBuf<dpk::SeedPair> pairs;
    DevBuf<int32_t> q2t, t2q;
    DevBuf<int64_t> kp_off;
    DevBuf<uint8_t> valid;
    DevBuf<unsigned long long> counters;
    // AKAZE (DetectorType::AKAZE): scale-space pools and tables
    DevBuf<float> akz_pool, akz_tmp, akz_k0, akz_g25;
    DevBuf<dpk::AkPlane> akz_planes;
    DevBuf<dpk::AkView> akz_views;
    DevBuf<uint32_t> akz_hmax, akz_hist, akz_bits;
    DevBuf<uint32_t> akz_seg;
    DevBuf<int64_t> akz_cand;
    DevBuf<int32_t> akz_vids;
    DevBuf<dpk::AkEntry> akz_spill; // suppression lists of views above the LDS cap
    int desc_words = 8; // 8 (ORB) or 16 (AKAZE) dwords per descriptor
    std::vector<dpk::SeedPair> h_pairs;
    std::vector<dpk::KnnJob> h_jobs;
    std::vector<int64_t> h_kp_off;
    std::vector<dp_keypoint> h_kp; // host copies of kp_b / kv_b (a detector's result)
    std::vector<int32_t> h_kv;
    std::vector<uint8_t> h_desc;
    std::vector<int32_t> h_q2t, h_t2q; // per (pair, query) / (pair, train): the other side's index or -1
    std::vector<double> h_xyz;
    bool have_stages = false;
};

// What either detector leaves behind for matching: n keypoints, view-major, in
// s->kp_b / s->kv_b with their host copies in s->h_kp / s->h_kv, and their
// descriptors in s->desc (s->desc_words dwords each).  The stream is idle and
// the events bound detection (e0 .. e1) and description (e1 .. e2).
struct Detected {
    int64_t n = 0;
    int64_t keypoints_detected = 0; // before FilterKeypoints
    Event e0, e1, e2;
};

// dp_probe_akaze_plane / dp_probe_orb_level: a detector stops after its image
// stage and hands out one plane (include/densepoints_probe.h)
struct SeedProbe {
    int view, level, which;
    void *out;        // host; null asks for the size only
    int64_t cap;      // elements out holds
    int32_t w = 0, h = 0;
};

// hipcub helpers on the context stream, temp storage in s->cub_tmp
#define DP_CUB(c, s, call_with_tmp)                                                                \
    do {                                                                                           \
        size_t _bytes = 0;                                                                         \
        void *_tmp = nullptr;                                                                      \
        DP_HIP(c, (call_with_tmp));                                                                \
        DP_HIP(c, (s)->cub_tmp.reserve(_bytes + 16));                                              \
        _tmp = (s)->cub_tmp.p;                                                                     \
        /* a select over 0 items must still report 0 selected */                                  \
        DP_HIP(c, hipMemsetAsync((s)->n_sel.p, 0, sizeof(int64_t), c->stream));                   \
        DP_HIP(c, (call_with_tmp));                                                                \
    } while (0)

struct NoHook {
    hipError_t operator()() const { return hipSuccess; }
};

// The items of in[0 .. n) whose flag is set, in order, into out; returns how
// many (one host wait), or a negative DP_E_* status.  `queued` runs after the
// select and before the count's copy, for work the wait should cover.
template <typename In, typename Out, typename Hook = NoHook>
int64_t select_flagged(dp_ctx *c, dp_seedgen *s, In in, uint8_t *flag, Out out, int64_t n, Hook queued = Hook())
{
    DP_CUB(c, s, hipcub::DeviceSelect::Flagged(_tmp, _bytes, in, flag, out, s->n_sel.p, (int)n, c->stream));
    DP_HIP(c, queued());
    int64_t n_sel = 0;
    DP_HIP(c, hipMemcpyAsync(&n_sel, s->n_sel.p, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return n_sel;
}

// FilterKeypoints (matcher.cpp:89-153): s->kp_a / kv_a (n3, view-major) ->
// s->kp_b / kv_b (*n4); one host wait (dp_seeds_capi.hip)
int cell_filter(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                const std::vector<int32_t> &vh, int64_t n3, int64_t *n4);

// The detectors: views of vw x vh px -> det (above).  With a probe they stop
// after the image stage: the plane's size always, its pixels when probe->out.
int orb_detect(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
               const std::vector<int32_t> &vh, Detected &det, SeedProbe *probe);
int akaze_detect(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                 const std::vector<int32_t> &vh, Detected &det, SeedProbe *probe);
