// dp_seeds_capi.hip -- C ABI of seed generation (include/densepoints.h,
// "seed generation"): Features::Matcher::GenerateSeeds
// (modules/features/matcher.cpp:18-43) on the device, plus the standalone
// operators (knnMatch, ComputeFundamentalMatrix, DirectLinearTriangulation).
// generate_seeds runs a detector (dp_seeds_orb.hip or dp_seeds_akaze.hip) and
// then the stages both share, which live here: FilterKeypoints, the per-view
// offsets, pair planning, matching, triangulation and the read-back.
#include "dp_dlt.h"
#include "dp_seedgen.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

void dp_seedgen_free(dp_seedgen *s) { delete s; }

static dp_seedgen *seedgen(dp_ctx *c)
{
    if (!c->seeds)
        c->seeds.reset(new (std::nothrow) dp_seedgen());
    return c->seeds.get();
}

extern "C" void dp_default_matcher_options(dp_matcher_options *mo)
{
    if (!mo)
        return;
    std::memset(mo, 0, sizeof(*mo));
    mo->n_features = 40000;
    mo->n_levels = 8;
    mo->scale_factor = 1.2;
    mo->edge_threshold = 31;
    mo->fast_threshold = 20;
    mo->cell_size = 16;
    mo->max_keypoints_per_cell = 4;
    mo->epipolar_matching = 0;
    mo->max_epipolar_distance = 1.5f;
    mo->nn_match_ratio = 0.7f;
    mo->matcher_type = DP_MATCHER_KNN;
    mo->detector_type = DP_DETECTOR_ORB;
    mo->akaze_threshold = 0.001f;
}

extern "C" int dp_orb_pattern(int8_t *xy_out)
{
    if (!xy_out)
        return DP_E_ARG;
    dpk::orb_pattern(xy_out);
    return DP_OK;
}

// ---------------------------------------------------------------------------
// Geometry::ComputeFundamentalMatrix (fundamental_matrix.cpp:6-34):
// F = [P' C]_x P' P^+,  P^+ = P^T (P P^T)^-1,  C = cofactor null vector of P
// (the reference's FullPivLU kernel is the same line, scaled).
// ---------------------------------------------------------------------------
static double det3c(const double *a, const double *b, const double *c)
{
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1])) +
           c[0] * (a[1] * b[2] - a[2] * b[1]);
}

extern "C" int dp_fundamental_matrix(const double P1[12], const double P2[12], double F[9])
{
    if (!P1 || !P2 || !F)
        return DP_E_ARG;
    double col[4][3];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            col[c][r] = P1[r * 4 + c];
    const double C[4] = {det3c(col[1], col[2], col[3]), -det3c(col[0], col[2], col[3]),
                         det3c(col[0], col[1], col[3]), -det3c(col[0], col[1], col[2])};
    double e[3];
    for (int i = 0; i < 3; ++i)
        e[i] = ((P2[i * 4] * C[0] + P2[i * 4 + 1] * C[1]) + P2[i * 4 + 2] * C[2]) + P2[i * 4 + 3] * C[3];
    double M[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[i][j] = ((P1[i * 4] * P1[j * 4] + P1[i * 4 + 1] * P1[j * 4 + 1]) + P1[i * 4 + 2] * P1[j * 4 + 2]) +
                      P1[i * 4 + 3] * P1[j * 4 + 3];
    double cof[3][3];
    cof[0][0] = M[1][1] * M[2][2] - M[1][2] * M[2][1];
    cof[0][1] = -(M[1][0] * M[2][2] - M[1][2] * M[2][0]);
    cof[0][2] = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    cof[1][0] = -(M[0][1] * M[2][2] - M[0][2] * M[2][1]);
    cof[1][1] = M[0][0] * M[2][2] - M[0][2] * M[2][0];
    cof[1][2] = -(M[0][0] * M[2][1] - M[0][1] * M[2][0]);
    cof[2][0] = M[0][1] * M[1][2] - M[0][2] * M[1][1];
    cof[2][1] = -(M[0][0] * M[1][2] - M[0][2] * M[1][0]);
    cof[2][2] = M[0][0] * M[1][1] - M[0][1] * M[1][0];
    const double det = (M[0][0] * cof[0][0] + M[0][1] * cof[0][1]) + M[0][2] * cof[0][2];
    if (det == 0.0 || !std::isfinite(det))
        return DP_E_ARG;
    double Mi[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Mi[i][j] = cof[j][i] / det;
    double Pp[4][3]; // P^T Mi
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j)
            Pp[k][j] = (P1[k] * Mi[0][j] + P1[4 + k] * Mi[1][j]) + P1[8 + k] * Mi[2][j];
    const double ex[3][3] = {{0.0, -e[2], e[1]}, {e[2], 0.0, -e[0]}, {-e[1], e[0], 0.0}};
    double A[3][4];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            A[i][j] = (ex[i][0] * P2[j] + ex[i][1] * P2[4 + j]) + ex[i][2] * P2[8 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            F[i * 3 + j] = ((A[i][0] * Pp[0][j] + A[i][1] * Pp[1][j]) + A[i][2] * Pp[2][j]) + A[i][3] * Pp[3][j];
    return DP_OK;
}

// ---------------------------------------------------------------------------
// knnMatch on one (query, train) pair
// ---------------------------------------------------------------------------
// Workgroups of a knn launch: 256 queries each; when the query blocks alone
// cannot fill the chip (one view pair), the train rows are split into nsplit
// ranges (multiples of the 128-row stage) whose top-2 keys knn_merge_kernel
// combines.  Every (query block, split) gets a workgroup, so every slot is
// written.
static int knn_blocks(const std::vector<dpk::KnnJob> &jobs, std::vector<dpk::KnnBlock> &blocks)
{
    int64_t qblocks = 0, max_nt = 0;
    for (const auto &j : jobs) {
        qblocks += (j.nq + dpk::kKnnQueriesPerBlock - 1) / dpk::kKnnQueriesPerBlock;
        max_nt = std::max<int64_t>(max_nt, j.nt);
    }
    const int64_t target = 3072; // ~12 workgroups per CU: 3 resident per CU, 4 rounds
    int nsplit = 1;
    if (qblocks > 0 && qblocks < target)
        nsplit = (int)std::min<int64_t>((target + qblocks - 1) / qblocks, std::max<int64_t>(1, max_nt / 1024));
    blocks.clear();
    for (size_t j = 0; j < jobs.size(); ++j) {
        int64_t chunk = (jobs[j].nt + nsplit - 1) / nsplit;
        chunk = (chunk + 127) / 128 * 128;
        for (int q = 0; q < jobs[j].nq; q += dpk::kKnnQueriesPerBlock)
            for (int sp = 0; sp < nsplit; ++sp) {
                dpk::KnnBlock b{};
                b.job = (int)j;
                b.q0 = q;
                b.t_lo = (int)std::min<int64_t>(sp * chunk, jobs[j].nt);
                b.t_hi = (int)std::min<int64_t>((sp + 1) * chunk, jobs[j].nt);
                b.slot = sp;
                blocks.push_back(b);
            }
    }
    return nsplit;
}

// knn over uploaded jobs (device copy in s->jobs); final keys into `keys`
static int run_knn(dp_ctx *c, dp_seedgen *s, const std::vector<dpk::KnnJob> &jobs, int64_t q_total, uint32_t *keys,
                   bool timed, int words)
{
    std::vector<dpk::KnnBlock> blocks;
    const int nsplit = knn_blocks(jobs, blocks);
    DP_HIP(c, s->blocks.reserve(blocks.size() + 1));
    if (!blocks.empty())
        DP_HIP(c, hipMemcpyAsync(s->blocks.p, blocks.data(), blocks.size() * sizeof(dpk::KnnBlock),
                                 hipMemcpyHostToDevice, c->stream));
    uint32_t *out = keys;
    const int64_t stride = 2 * q_total;
    if (nsplit > 1) {
        DP_HIP(c, s->pkeys.reserve((size_t)nsplit * stride + 1));
        out = s->pkeys.p;
    }
    dpk::KnnArgs ka{s->desc.p, s->jobs.p, s->blocks.p, out, stride, words};
    if (timed)
        DP_HIP(c, hipEventRecord(c->e0, c->stream));
    DP_HIP(c, dpk::launch_knn(ka, (int)blocks.size(), c->stream));
    if (nsplit > 1)
        DP_HIP(c, dpk::launch_knn_merge(out, nsplit, stride, q_total, keys, c->stream));
    if (timed) {
        DP_HIP(c, hipEventRecord(c->e1, c->stream));
        c->timed = true;
    }
    return DP_OK;
}

static int knn_match_impl(dp_ctx *c, const uint8_t *query, int64_t nq, const uint8_t *train, int64_t nt, int bytes,
                          int32_t *idx2, int32_t *dist2)
{
    if (!c)
        return DP_E_ARG;
    const int words = bytes / 4;
    if ((bytes != 32 && bytes != 64) || nq < 0 || nt < 0 || nt >= (1 << dpk::knn_row_bits(words)) || nq > INT32_MAX ||
        (nq > 0 && (!query || !idx2 || !dist2)) || (nt > 0 && !train))
        return fail(c, DP_E_ARG, "dp_knn_match: bad arguments");
    if (nq == 0)
        return DP_OK;
    dp_seedgen *s = seedgen(c);
    if (!s)
        return fail(c, DP_E_OOM, "seedgen state");
    DP_HIP(c, hipSetDevice(c->device));
    DP_HIP(c, s->desc.reserve((size_t)(nq + nt) * words));
    DP_HIP(c, s->keys.reserve((size_t)nq * 2));
    DP_HIP(c, s->i2.reserve((size_t)nq * 2));
    DP_HIP(c, s->d2.reserve((size_t)nq * 2));
    DP_HIP(c, hipMemcpyAsync(s->desc.p, query, (size_t)nq * bytes, hipMemcpyHostToDevice, c->stream));
    if (nt > 0)
        DP_HIP(c, hipMemcpyAsync(s->desc.p + nq * words, train, (size_t)nt * bytes, hipMemcpyHostToDevice, c->stream));
    std::vector<dpk::KnnJob> jobs(1);
    jobs[0].q_off = 0;
    jobs[0].t_off = nq;
    jobs[0].out_off = 0;
    jobs[0].nq = (int32_t)nq;
    jobs[0].nt = (int32_t)nt;
    DP_HIP(c, s->jobs.reserve(1));
    DP_HIP(c, hipMemcpyAsync(s->jobs.p, jobs.data(), sizeof(dpk::KnnJob), hipMemcpyHostToDevice, c->stream));
    int rc = run_knn(c, s, jobs, nq, s->keys.p, true, words);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, dpk::launch_knn_decode(s->desc.p, words, 0, nq, s->keys.p, s->i2.p, s->d2.p, c->stream));
    DP_HIP(c, hipMemcpyAsync(idx2, s->i2.p, (size_t)nq * 8, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipMemcpyAsync(dist2, s->d2.p, (size_t)nq * 8, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

extern "C" int dp_knn_match(dp_ctx *c, const uint8_t *query, int64_t nq, const uint8_t *train, int64_t nt,
                            int32_t *idx2, int32_t *dist2)
{
    return knn_match_impl(c, query, nq, train, nt, 32, idx2, dist2);
}

extern "C" int dp_knn_match_wide(dp_ctx *c, const uint8_t *query, int64_t nq, const uint8_t *train, int64_t nt,
                                 int descriptor_bytes, int32_t *idx2, int32_t *dist2)
{
    return knn_match_impl(c, query, nq, train, nt, descriptor_bytes, idx2, dist2);
}

// ---------------------------------------------------------------------------
// batched DLT
// ---------------------------------------------------------------------------
extern "C" int dp_triangulate(dp_ctx *c, int64_t n, const int32_t *offsets, const double *P, const double *obs,
                              double *X)
{
    if (!c)
        return DP_E_ARG;
    if (n < 0 || (n > 0 && (!offsets || !P || !obs || !X)))
        return fail(c, DP_E_ARG, "dp_triangulate: bad arguments");
    if (n == 0)
        return DP_OK;
    if (offsets[0] != 0)
        return fail(c, DP_E_ARG, "dp_triangulate: offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] + 1)
            return fail(c, DP_E_ARG, "dp_triangulate: every point needs at least one observation");
    const int64_t m = offsets[n];
    dp_seedgen *s = seedgen(c);
    if (!s)
        return fail(c, DP_E_OOM, "seedgen state");
    DP_HIP(c, hipSetDevice(c->device));
    DP_HIP(c, s->off.reserve((size_t)n + 1));
    DP_HIP(c, s->P.reserve((size_t)m * 12));
    DP_HIP(c, s->obs.reserve((size_t)m * 2));
    DP_HIP(c, s->X.reserve((size_t)n * 3));
    DP_HIP(c, hipMemcpyAsync(s->off.p, offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    DP_HIP(c, hipMemcpyAsync(s->P.p, P, (size_t)m * 96, hipMemcpyHostToDevice, c->stream));
    DP_HIP(c, hipMemcpyAsync(s->obs.p, obs, (size_t)m * 16, hipMemcpyHostToDevice, c->stream));
    DP_HIP(c, dpk::launch_dlt_batch(n, s->off.p, s->P.p, s->obs.p, s->X.p, c->stream));
    DP_HIP(c, hipMemcpyAsync(X, s->X.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
    DP_HIP(c, hipStreamSynchronize(c->stream));
    return DP_OK;
}

// ---------------------------------------------------------------------------
// GenerateSeeds
// ---------------------------------------------------------------------------
static int check_matcher_options(dp_ctx *c, const dp_matcher_options &m)
{
    if (m.n_features < 0 || m.n_levels < 1 || m.n_levels > dpk::kOrbMaxLevels || !(m.scale_factor > 1.0) ||
        m.edge_threshold < 19 || m.fast_threshold < 0 || m.fast_threshold > 254 || m.cell_size < 1 ||
        m.max_keypoints_per_cell < 0 || (m.epipolar_matching != 0 && m.epipolar_matching != 1) ||
        !(m.nn_match_ratio >= 0.0f) || !(m.max_epipolar_distance >= 0.0f) ||
        (m.matcher_type != DP_MATCHER_KNN && m.matcher_type != DP_MATCHER_FLANN) ||
        (m.detector_type != DP_DETECTOR_AKAZE && m.detector_type != DP_DETECTOR_ORB) ||
        !(m.akaze_threshold > 0.0f) || !std::isfinite(m.akaze_threshold))
        return fail(c, DP_E_ARG, "dp_matcher_options: value out of range (edge_threshold >= 19, 1 <= n_levels <= 16, "
                                 "detector_type AKAZE/ORB, akaze_threshold > 0)");
    return DP_OK;
}

// FilterKeypoints (matcher.cpp:89-153): s->kp_a / kv_a (n3, view-major) ->
// s->kp_b / kv_b (*n4): per cell (row-major per view) its keypoints in order,
// or the best max_keypoints_per_cell by (response desc, index)
int cell_filter(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const std::vector<int32_t> &vw,
                const std::vector<int32_t> &vh, int64_t n3, int64_t *n4)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    std::vector<int32_t> gcols(V);
    std::vector<int64_t> cell_off(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        gcols[v] = (vw[v] + mo.cell_size - 1) / mo.cell_size;
        const int64_t grows = (vh[v] + mo.cell_size - 1) / mo.cell_size;
        if ((int64_t)gcols[v] * grows >= (1ll << 24))
            return fail(c, DP_E_ARG, "dp_generate_seeds: more than 2^24 keypoint cells per view");
        cell_off[v + 1] = cell_off[v] + (int64_t)gcols[v] * grows;
    }
    DP_HIP(c, s->gcols.reserve(V));
    DP_HIP(c, s->cell_off.reserve(V + 1));
    DP_HIP(c, s->cell_cnt.reserve(cell_off[V] + 1));
    DP_HIP(c, hipMemcpyAsync(s->gcols.p, gcols.data(), V * 4, hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemcpyAsync(s->cell_off.p, cell_off.data(), (V + 1) * 8, hipMemcpyHostToDevice, st));
    DP_HIP(c, hipMemsetAsync(s->cell_cnt.p, 0, (size_t)(cell_off[V] + 1) * 4, st));
    DP_HIP(c, s->ckey.reserve(n3 + 1));
    DP_HIP(c, s->ckey_sorted.reserve(n3 + 1));
    DP_HIP(c, s->idx_a.reserve(n3 + 1));
    DP_HIP(c, s->idx_b.reserve(n3 + 1));
    DP_HIP(c, s->flag.reserve(n3 + 1));
    DP_HIP(c, dpk::launch_cell_count(s->kp_a.p, s->kv_a.p, n3, s->gcols.p, s->cell_off.p, mo.cell_size, s->cell_cnt.p,
                                     st));
    DP_HIP(c, dpk::launch_cell_key(s->kp_a.p, s->kv_a.p, n3, s->gcols.p, s->cell_off.p, mo.cell_size,
                                   mo.max_keypoints_per_cell, s->cell_cnt.p, s->ckey.p, s->idx_a.p, st));
    if (n3 > 0)
        DP_CUB(c, s, hipcub::DeviceRadixSort::SortPairs(_tmp, _bytes, s->ckey.p, s->ckey_sorted.p, s->idx_a.p,
                                                         s->idx_b.p, (int)n3, 0, 64, st));
    DP_HIP(c, dpk::launch_cell_keep(s->ckey_sorted.p, n3, mo.max_keypoints_per_cell, s->flag.p, st));
    *n4 = select_flagged(c, s, s->idx_b.p, s->flag.p, s->idx_a.p, n3);
    if (*n4 < 0)
        return (int)*n4;
    DP_HIP(c, s->kp_b.reserve(*n4 + 1));
    DP_HIP(c, s->kv_b.reserve(*n4 + 1));
    DP_HIP(c, dpk::launch_gather_kp(s->kp_a.p, s->kv_a.p, s->idx_a.p, *n4, s->kp_b.p, s->kv_b.p, st));
    return DP_OK;
}

// ---------------------------------------------------------------------------
// the stages after a detector (Detected, dp_seedgen.h)
// ---------------------------------------------------------------------------
namespace {

double ev_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    hipEventElapsedTime(&ms, a, b);
    return (double)ms;
}

// the view pairs of a run and the sizes of their match tables
struct PairPlan {
    int np = 0;
    int64_t q_total = 0, t2q_total = 0; // queries (rows of keys / q2t), train rows (t2q) over all pairs
};

// s->h_kv (n keypoints, view-major) -> s->h_kp_off, the first keypoint of each view
int view_offsets(dp_ctx *c, dp_seedgen *s, int64_t n)
{
    const int V = c->V;
    s->h_kp_off.assign(V + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        s->h_kp_off[s->h_kv[i] + 1]++;
    for (int v = 0; v < V; ++v)
        s->h_kp_off[v + 1] += s->h_kp_off[v];
    for (int v = 0; v < V; ++v)
        if (s->h_kp_off[v + 1] - s->h_kp_off[v] >= (1 << dpk::knn_row_bits(s->desc_words)))
            return fail(c, DP_E_ARG, "dp_generate_seeds: more than 2^22 (ORB) / 2^21 (AKAZE) keypoints in one view");
    return DP_OK;
}

// DefaultPairsList: every pair (i < j) with its fundamental matrix and kNN job
// from s->h_kp_off -> s->h_pairs / h_jobs and their device copies s->pairs /
// jobs; the match tables sized, s->t2q and s->counters cleared
int plan_pairs(dp_ctx *c, dp_seedgen *s, PairPlan &plan)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    s->h_pairs.clear();
    s->h_jobs.clear();
    int64_t q_total = 0, t2q_total = 0;
    for (int i = 0; i < V; ++i)
        for (int j = i + 1; j < V; ++j) {
            dpk::SeedPair pr{};
            if (dp_fundamental_matrix(c->P0.data() + 12 * i, c->P0.data() + 12 * j, pr.F) != DP_OK)
                return fail(c, DP_E_ARG, "dp_generate_seeds: degenerate projection matrix");
            pr.first = i;
            pr.second = j;
            pr.t2q_off = t2q_total;
            dpk::KnnJob jb{};
            jb.q_off = s->h_kp_off[i];
            jb.t_off = s->h_kp_off[j];
            jb.out_off = q_total;
            jb.nq = (int32_t)(s->h_kp_off[i + 1] - s->h_kp_off[i]);
            jb.nt = (int32_t)(s->h_kp_off[j + 1] - s->h_kp_off[j]);
            q_total += jb.nq;
            t2q_total += jb.nt;
            s->h_pairs.push_back(pr);
            s->h_jobs.push_back(jb);
        }
    const int np = (int)s->h_pairs.size();
    plan = PairPlan{np, q_total, t2q_total};
    DP_HIP(c, s->pairs.reserve(np + 1));
    DP_HIP(c, s->jobs.reserve(np + 1));
    DP_HIP(c, s->q2t.reserve(q_total + 1));
    DP_HIP(c, s->t2q.reserve(t2q_total + 1));
    DP_HIP(c, s->keys.reserve((size_t)2 * (q_total + 1)));
    DP_HIP(c, s->counters.reserve(2));
    if (np > 0) {
        DP_HIP(c, hipMemcpyAsync(s->pairs.p, s->h_pairs.data(), np * sizeof(dpk::SeedPair), hipMemcpyHostToDevice, st));
        DP_HIP(c, hipMemcpyAsync(s->jobs.p, s->h_jobs.data(), np * sizeof(dpk::KnnJob), hipMemcpyHostToDevice, st));
    }
    static_assert(dpk::kNoMatch == 0x7F7F7F7F, "t2q sentinel is the 0x7F byte fill");
    DP_HIP(c, hipMemsetAsync(s->t2q.p, 0x7F, (size_t)(t2q_total + 1) * 4, st)); // kNoMatch > any index
    DP_HIP(c, hipMemsetAsync(s->counters.p, 0, 2 * sizeof(unsigned long long), st));
    return DP_OK;
}

// MatchKeypoints + FilterMatches of the planned pairs on s->desc / kp_b ->
// s->q2t / t2q, and s->counters = {ratio matches, matches}
int match_pairs(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, const PairPlan &plan)
{
    hipStream_t st = c->stream;
    dpk::MatchArgs ma{s->jobs.p, s->pairs.p, plan.np, plan.q_total, s->keys.p, s->desc.p, s->kp_b.p, s->desc_words,
                      mo.nn_match_ratio, mo.max_epipolar_distance, mo.matcher_type == DP_MATCHER_FLANN,
                      s->q2t.p, s->t2q.p, s->counters.p, s->counters.p + 1};
    if (mo.epipolar_matching) {
        DP_HIP(c, dpk::launch_epipolar_match(ma, st));
    } else {
        int rc = run_knn(c, s, s->h_jobs, plan.q_total, s->keys.p, false, s->desc_words);
        if (rc != DP_OK)
            return rc;
        DP_HIP(c, dpk::launch_match(ma, st));
    }
    return DP_OK;
}

// TriangulateMatches (matcher.cpp:415-450): one point per keypoint (n) that
// starts a track, from s->q2t / t2q -> s->X with s->valid; s->obs sized for
// the compacted points
int triangulate(dp_ctx *c, dp_seedgen *s, const PairPlan &plan, int64_t n)
{
    hipStream_t st = c->stream;
    const int V = c->V;
    DP_HIP(c, s->kp_off.reserve(V + 1));
    DP_HIP(c, hipMemcpyAsync(s->kp_off.p, s->h_kp_off.data(), (V + 1) * 8, hipMemcpyHostToDevice, st));
    DP_HIP(c, s->P.reserve((size_t)V * 12));
    DP_HIP(c, hipMemcpyAsync(s->P.p, c->P0.data(), (size_t)V * 96, hipMemcpyHostToDevice, st));
    DP_HIP(c, s->X.reserve((size_t)3 * (n + 1)));
    DP_HIP(c, s->obs.reserve((size_t)3 * (n + 1)));
    DP_HIP(c, s->valid.reserve(n + 1));
    dpk::TriangArgs ta{V, plan.np, n, s->kp_off.p, s->kp_b.p, s->P.p, s->jobs.p, s->pairs.p, s->q2t.p, s->t2q.p,
                       s->X.p, s->valid.p};
    DP_HIP(c, dpk::launch_triang(ta, st));
    return DP_OK;
}

// the n6 points (s->obs), the n descriptors and the match tables to the host
// (s->h_xyz, h_desc, h_q2t, h_t2q with -1 for an empty slot).  One host wait.
int read_back(dp_ctx *c, dp_seedgen *s, const PairPlan &plan, int64_t n, int64_t n6)
{
    hipStream_t st = c->stream;
    s->h_xyz.resize((size_t)3 * n6);
    const size_t dbytes = (size_t)4 * s->desc_words;
    s->h_desc.resize(dbytes * n);
    s->h_q2t.resize(plan.q_total);
    s->h_t2q.resize(plan.t2q_total);
    DP_HIP(c, hipMemcpyAsync(s->h_xyz.data(), s->obs.p, (size_t)n6 * 24, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(s->h_desc.data(), s->desc.p, (size_t)n * dbytes, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(s->h_q2t.data(), s->q2t.p, (size_t)plan.q_total * 4, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipMemcpyAsync(s->h_t2q.data(), s->t2q.p, (size_t)plan.t2q_total * 4, hipMemcpyDeviceToHost, st));
    DP_HIP(c, hipStreamSynchronize(st));
    for (int32_t &q : s->h_t2q)
        if (q == dpk::kNoMatch)
            q = -1;
    return DP_OK;
}

// what the stages after a detector leave behind besides the host tables
struct StageResult {
    int np = 0;
    int64_t ratio_matches = 0, matches = 0, points = 0;
    Event t3, t4; // matching ends at t3, triangulation at t4
};

// Everything after a detector: n keypoints as Detected (dp_seedgen.h) states
// them -> the points in s->h_xyz and the tables of read_back.  The one
// sequence dp_generate_seeds and dp_probe_seed_stages both run.
int stages_after_detect(dp_ctx *c, dp_seedgen *s, const dp_matcher_options &mo, int64_t n, StageResult &r)
{
    hipStream_t st = c->stream;
    int rc = view_offsets(c, s, n);
    if (rc != DP_OK)
        return rc;

    // ---- DefaultPairsList + MatchKeypoints + FilterMatches
    PairPlan plan;
    rc = plan_pairs(c, s, plan);
    if (rc == DP_OK)
        rc = match_pairs(c, s, mo, plan);
    if (rc != DP_OK)
        return rc;
    DP_HIP(c, hipEventRecord(r.t3, st));

    // ---- TriangulateMatches, the valid points compacted into s->obs
    rc = triangulate(c, s, plan, n);
    if (rc != DP_OK)
        return rc;
    struct P3 { // local to this function: its name is part of the select kernel's
        double x, y, z;
    };
    unsigned long long cnt[2] = {0, 0};
    const int64_t n6 = select_flagged(
        c, s, reinterpret_cast<P3 *>(s->X.p), s->valid.p, reinterpret_cast<P3 *>(s->obs.p), n, [&]() {
            hipError_t e = hipEventRecord(r.t4, st);
            return e != hipSuccess ? e : hipMemcpyAsync(cnt, s->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, st);
        });
    if (n6 < 0)
        return (int)n6;
    rc = read_back(c, s, plan, n, n6);
    if (rc != DP_OK)
        return rc;
    r.np = plan.np;
    r.ratio_matches = (int64_t)cnt[0];
    r.matches = (int64_t)cnt[1];
    r.points = n6;
    return DP_OK;
}

} // namespace

static int generate_seeds(dp_ctx *c, const dp_matcher_options *mo_in, const double **xyz_out, int64_t *n_out,
                          dp_seed_stats *stats, SeedProbe *probe);

extern "C" int dp_generate_seeds(dp_ctx *c, const dp_matcher_options *mo_in, const double **xyz_out, int64_t *n_out,
                                 dp_seed_stats *stats)
{
    return generate_seeds(c, mo_in, xyz_out, n_out, stats, nullptr);
}

// The probes run seed generation's own launch sequence up to the planes they
// return (no second copy of it), with the options' defaults but for the
// detector and, for ORB, the pyramid's shape.
extern "C" int dp_probe_akaze_plane(dp_ctx *c, int view, int level, int which, float *out, int64_t cap, int32_t *wh)
{
    if (!c)
        return DP_E_ARG;
    if (!wh || view < 0 || view >= c->V)
        return fail(c, DP_E_ARG, "dp_probe_akaze_plane: bad view or null size");
    dp_matcher_options mo;
    dp_default_matcher_options(&mo);
    mo.detector_type = DP_DETECTOR_AKAZE;
    SeedProbe pr{view, level, which, out, cap};
    const double *xyz = nullptr;
    int64_t n = 0;
    const int rc = generate_seeds(c, &mo, &xyz, &n, nullptr, &pr);
    wh[0] = pr.w;
    wh[1] = pr.h;
    return rc;
}

extern "C" int dp_probe_orb_level(dp_ctx *c, int view, int level, int n_levels, double scale_factor, uint8_t *out,
                                  int64_t cap, int32_t *wh)
{
    if (!c)
        return DP_E_ARG;
    if (!wh || view < 0 || view >= c->V || level < 0 || level >= n_levels)
        return fail(c, DP_E_ARG, "dp_probe_orb_level: bad view or level, or null size");
    dp_matcher_options mo;
    dp_default_matcher_options(&mo);
    mo.detector_type = DP_DETECTOR_ORB;
    mo.n_levels = n_levels;
    mo.scale_factor = scale_factor;
    SeedProbe pr{view, level, 0, out, cap};
    const double *xyz = nullptr;
    int64_t n = 0;
    const int rc = generate_seeds(c, &mo, &xyz, &n, nullptr, &pr);
    wh[0] = pr.w;
    wh[1] = pr.h;
    return rc;
}

static int generate_seeds(dp_ctx *c, const dp_matcher_options *mo_in, const double **xyz_out, int64_t *n_out,
                          dp_seed_stats *stats, SeedProbe *probe)
{
    if (!c)
        return DP_E_ARG;
    if (!xyz_out || !n_out)
        return fail(c, DP_E_ARG, "dp_generate_seeds: null output");
    *xyz_out = nullptr;
    *n_out = 0;
    if (c->V < 1 || c->planes.empty())
        return fail(c, DP_E_STATE, "dp_generate_seeds: no views set");
    dp_matcher_options mo;
    if (mo_in)
        mo = *mo_in;
    else
        dp_default_matcher_options(&mo);
    int rc = check_matcher_options(c, mo);
    if (rc != DP_OK)
        return rc;
    dp_seedgen *s = seedgen(c);
    if (!s)
        return fail(c, DP_E_OOM, "seedgen state");
    s->have_stages = false;
    DP_HIP(c, hipSetDevice(c->device));
    const auto t_wall0 = std::chrono::steady_clock::now();
    const int V = c->V;
    std::vector<int32_t> vw(V), vh(V);
    for (int v = 0; v < V; ++v) {
        vw[v] = c->hv[v].W;
        vh[v] = c->hv[v].H;
    }
    DP_HIP(c, s->n_sel.reserve(1));

    Detected det;
    rc = (mo.detector_type == DP_DETECTOR_AKAZE ? akaze_detect : orb_detect)(c, s, mo, vw, vh, det, probe);
    if (rc != DP_OK || probe)
        return rc;
    StageResult sr;
    rc = stages_after_detect(c, s, mo, det.n, sr);
    if (rc != DP_OK)
        return rc;

    dp_seed_stats S{};
    S.keypoints_detected = det.keypoints_detected;
    S.keypoints = det.n;
    S.pairs = sr.np;
    S.ratio_matches = sr.ratio_matches;
    S.matches = sr.matches;
    S.points = sr.points;
    S.detect_ms = ev_ms(det.e0, det.e1);
    S.describe_ms = ev_ms(det.e1, det.e2);
    S.match_ms = ev_ms(det.e2, sr.t3);
    S.triangulate_ms = ev_ms(sr.t3, sr.t4);
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wall0).count();
    s->have_stages = true;
    if (stats)
        *stats = S;
    *xyz_out = s->h_xyz.data();
    *n_out = sr.points;
    return DP_OK;
}

// The caller's keypoints and descriptors stand in for a detector's result
// (Detected, dp_seedgen.h); the stages after it are dp_generate_seeds' own.
extern "C" int dp_probe_seed_stages(dp_ctx *c, int n_views, const int32_t *counts, const dp_keypoint *kp,
                                    const uint8_t *desc, int descriptor_bytes, const dp_matcher_options *mo_in,
                                    const double **xyz_out, int64_t *n_out, dp_seed_stats *stats)
{
    if (!c)
        return DP_E_ARG;
    if (!xyz_out || !n_out)
        return fail(c, DP_E_ARG, "dp_probe_seed_stages: null output");
    *xyz_out = nullptr;
    *n_out = 0;
    if (c->V < 1)
        return fail(c, DP_E_STATE, "dp_probe_seed_stages: no views set");
    if (n_views != c->V)
        return fail(c, DP_E_ARG, "dp_probe_seed_stages: one keypoint count per view of the context is needed");
    if (descriptor_bytes != 32 && descriptor_bytes != 64)
        return fail(c, DP_E_ARG, "dp_probe_seed_stages: descriptors are 32 or 64 bytes wide");
    if (!counts)
        return fail(c, DP_E_ARG, "dp_probe_seed_stages: null counts");
    const int words = descriptor_bytes / 4;
    int64_t n = 0;
    for (int v = 0; v < n_views; ++v) {
        if (counts[v] < 0)
            return fail(c, DP_E_ARG, "dp_probe_seed_stages: negative keypoint count");
        if (counts[v] >= (1 << dpk::knn_row_bits(words)))
            return fail(c, DP_E_ARG, "dp_probe_seed_stages: 2^22 (32-byte) / 2^21 (64-byte) or more keypoints in one view");
        n += counts[v];
    }
    if (n > 0 && (!kp || !desc))
        return fail(c, DP_E_ARG, "dp_probe_seed_stages: null keypoints or descriptors");
    dp_matcher_options mo;
    if (mo_in)
        mo = *mo_in;
    else
        dp_default_matcher_options(&mo);
    int rc = check_matcher_options(c, mo);
    if (rc != DP_OK)
        return rc;
    dp_seedgen *s = seedgen(c);
    if (!s)
        return fail(c, DP_E_OOM, "seedgen state");
    s->have_stages = false;
    DP_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_wall0 = std::chrono::steady_clock::now();
    DP_HIP(c, s->n_sel.reserve(1));

    s->desc_words = words;
    s->h_kp.assign(kp, kp + n);
    s->h_kv.resize(n);
    for (int64_t v = 0, i = 0; v < n_views; ++v)
        for (int32_t k = 0; k < counts[v]; ++k)
            s->h_kv[i++] = (int32_t)v;
    DP_HIP(c, s->kp_b.reserve(n + 1));
    DP_HIP(c, s->kv_b.reserve(n + 1));
    DP_HIP(c, s->desc.reserve((size_t)(n + 1) * words));
    if (n > 0) {
        DP_HIP(c, hipMemcpyAsync(s->kp_b.p, s->h_kp.data(), (size_t)n * sizeof(dp_keypoint), hipMemcpyHostToDevice, st));
        DP_HIP(c, hipMemcpyAsync(s->kv_b.p, s->h_kv.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        DP_HIP(c, hipMemcpyAsync(s->desc.p, desc, (size_t)n * descriptor_bytes, hipMemcpyHostToDevice, st));
    }
    Event t2;
    DP_HIP(c, hipEventRecord(t2, st));
    DP_HIP(c, hipStreamSynchronize(st)); // a detector leaves the stream idle; desc is the caller's

    StageResult sr;
    rc = stages_after_detect(c, s, mo, n, sr);
    if (rc != DP_OK)
        return rc;

    dp_seed_stats S{};
    S.keypoints_detected = n;
    S.keypoints = n;
    S.pairs = sr.np;
    S.ratio_matches = sr.ratio_matches;
    S.matches = sr.matches;
    S.points = sr.points;
    S.match_ms = ev_ms(t2, sr.t3);
    S.triangulate_ms = ev_ms(sr.t3, sr.t4);
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wall0).count();
    s->have_stages = true;
    if (stats)
        *stats = S;
    *xyz_out = s->h_xyz.data();
    *n_out = sr.points;
    return DP_OK;
}

extern "C" int dp_seed_keypoints(dp_ctx *c, int view, const dp_keypoint **kp, const uint8_t **desc32, int64_t *n)
{
    if (!c)
        return DP_E_ARG;
    dp_seedgen *s = c->seeds.get();
    if (!s || !s->have_stages)
        return fail(c, DP_E_STATE, "dp_seed_keypoints: no dp_generate_seeds result");
    if (view < 0 || view >= (int)s->h_kp_off.size() - 1 || !n)
        return fail(c, DP_E_ARG, "dp_seed_keypoints: bad view");
    const int64_t a = s->h_kp_off[view], b = s->h_kp_off[view + 1];
    if (kp)
        *kp = s->h_kp.data() + a;
    if (desc32)
        *desc32 = s->h_desc.data() + (size_t)4 * s->desc_words * a;
    *n = b - a;
    return DP_OK;
}

extern "C" int dp_seed_descriptor_bytes(dp_ctx *c)
{
    if (!c)
        return DP_E_ARG;
    dp_seedgen *s = c->seeds.get();
    if (!s || !s->have_stages)
        return fail(c, DP_E_STATE, "dp_seed_descriptor_bytes: no dp_generate_seeds result");
    return 4 * s->desc_words;
}

extern "C" int dp_seed_matches(dp_ctx *c, int pair, int32_t *first, int32_t *second, const int32_t **q2t, int64_t *nq)
{
    if (!c)
        return DP_E_ARG;
    dp_seedgen *s = c->seeds.get();
    if (!s || !s->have_stages)
        return fail(c, DP_E_STATE, "dp_seed_matches: no dp_generate_seeds result");
    if (pair < 0 || pair >= (int)s->h_pairs.size())
        return fail(c, DP_E_ARG, "dp_seed_matches: bad pair");
    if (first)
        *first = s->h_pairs[pair].first;
    if (second)
        *second = s->h_pairs[pair].second;
    if (q2t)
        *q2t = s->h_q2t.data() + s->h_jobs[pair].out_off;
    if (nq)
        *nq = s->h_jobs[pair].nq;
    return DP_OK;
}

extern "C" int dp_probe_seed_t2q(dp_ctx *c, int pair, const int32_t **t2q, int64_t *nt)
{
    if (!c)
        return DP_E_ARG;
    dp_seedgen *s = c->seeds.get();
    if (!s || !s->have_stages)
        return fail(c, DP_E_STATE, "dp_probe_seed_t2q: no dp_generate_seeds result");
    if (pair < 0 || pair >= (int)s->h_pairs.size() || !t2q || !nt)
        return fail(c, DP_E_ARG, "dp_probe_seed_t2q: bad pair or null output");
    *t2q = s->h_t2q.data() + s->h_pairs[pair].t2q_off;
    *nt = s->h_jobs[pair].nt;
    return DP_OK;
}
