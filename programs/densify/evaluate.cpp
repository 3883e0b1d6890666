// evaluate.cpp -- see evaluate.h.  The device calls of --evaluate; every number
// and every piece of the report comes from eval_stats.h.
#include "evaluate.h"

#include "eval_stats.h"

#include <algorithm>

struct Evaluation::Found {
    DeviceMaps out;
    int64_t nq;
    int32_t *d_index = nullptr;
    float *d_dist = nullptr;
    explicit Found(int64_t n) : nq(n)
    {
        d_index = (int32_t *)out.bytes((size_t)nq * 4, "--evaluate");
        d_dist = (float *)out.bytes((size_t)nq * 4, "--evaluate");
    }
    void read(std::vector<int32_t> &index, std::vector<float> &dist, const char *message) const
    {
        index.resize((size_t)nq);
        dist.resize((size_t)nq);
        download(index, d_index, message);
        download(dist, d_dist, message);
    }
    evalstats::Matched matched() const
    {
        std::vector<int32_t> index;
        std::vector<float> dist;
        read(index, dist, "--evaluate: copy of the distances failed");
        return evalstats::matched_distances(index, dist);
    }
};

Evaluation::Evaluation(dp_ctx *c, const Args &args, const std::vector<double> &truth)
    : ctx(c), tau(args.eval_tau), max_dist((float)args.eval_max_dist), n_truth((int64_t)(truth.size() / 3)),
      align(args.eval_align), normals(args.eval_normals)
{
    align_opts.max_dist = (float)args.eval_align_radius;
    align_opts.iterations = args.eval_align_iterations;
    align_opts.min_pairs = 3;
    align_opts.flags = args.eval_align_scale ? DP_CLOUD_ALIGN_SCALE : 0;
    align_opts.rms_tol = 0.0;
    normals_opts.max_dist = (float)args.eval_normals_radius;
    normals_opts.k = args.eval_normals_k;
    normals_opts.min_neighbours = 3;
    normals_opts.flags = 0;
    const std::vector<float> xyz(truth.begin(), truth.end());
    d_truth = (float *)mem.bytes(xyz.size() * sizeof(float), "--evaluate");
    upload(d_truth, xyz, "--evaluate: copy of the ground truth failed");
}

// --eval-normals: the normals of the queries (normal_offset bytes behind their
// positions) against the truth's, which the first call estimates, over the
// matches of the accuracy direction
JsonObject Evaluation::normals_entry(const Found &f, const void *d_q, int64_t nq, int64_t qs, int64_t normal_offset)
{
    if (!d_truth_normal) {
        d_truth_normal = (float *)mem.bytes((size_t)std::max<int64_t>(n_truth, 1) * 12, "--eval-normals");
        check(ctx,
              dp_cloud_normals_device(ctx, n_truth ? d_truth : nullptr, n_truth, 12, &normals_opts, nullptr, 0,
                                      d_truth_normal, nullptr, nullptr, nullptr, nullptr),
              "dp_cloud_normals_device");
    }
    const char *failed = "--eval-normals: copy of the normals failed";
    std::vector<int32_t> index;
    std::vector<float> dist, truth((size_t)n_truth * 3);
    // the records up to the end of the last one's normal
    std::vector<char> recs(nq > 0 ? (size_t)(nq - 1) * (size_t)qs + (size_t)normal_offset + 12 : 0);
    if (hipDeviceSynchronize() != hipSuccess)
        throw std::runtime_error(failed);
    f.read(index, dist, failed);
    download(recs, d_q, failed);
    download(truth, d_truth_normal, failed);
    return evalstats::normals_entry(recs.data(), (size_t)qs, (size_t)normal_offset, index, dist, truth, tau);
}

// one direction between two clouds; normal_offset >= 0: the entry of the queries' normals into *normals_json
JsonObject Evaluation::side(const void *d_q, int64_t nq, int64_t qs, const void *d_t, int64_t nt, int64_t ts,
                            double *ratio, int64_t normal_offset, JsonObject *normals_json)
{
    Found f(nq);
    const dp_cloud_nearest_options o{max_dist, 0, 0};
    dp_cloud_nearest_stats st;
    check(ctx,
          dp_cloud_nearest_device(ctx, nq ? d_q : nullptr, nq, qs, nt ? d_t : nullptr, nt, ts, &o, f.d_index, f.d_dist,
                                  nullptr, &st, nullptr),
          "dp_cloud_nearest_device");
    if (normal_offset >= 0)
        *normals_json = normals_entry(f, d_q, nq, qs, normal_offset);
    return evalstats::side_entry(f.matched(), st.queries, st.matched, tau, ratio);
}

// points against the surface of a device mesh (dp_mesh_nearest_device)
dp_mesh_nearest_stats Evaluation::surface(const Found &f, const void *d_q, int64_t nq, int64_t qs,
                                          const dp_mesh_vertex *d_v, int64_t nv, const int32_t *d_t, int64_t nt)
{
    const dp_mesh_nearest_options o{max_dist, 0, 0};
    dp_mesh_nearest_stats st;
    check(ctx,
          dp_mesh_nearest_device(ctx, nq ? d_q : nullptr, nq, qs, nv ? d_v : nullptr, nv, nt ? d_t : nullptr, nt, &o,
                                 f.d_index, f.d_dist, nullptr, nullptr, &st, nullptr),
          "dp_mesh_nearest_device");
    return st;
}

void Evaluation::add_mesh_surface(const dp_mesh_vertex *d_v, int64_t nv, const int32_t *d_t, int64_t nt)
{
    DeviceMaps copy;
    d_v = (const dp_mesh_vertex *)moved(copy, d_v, nv, sizeof(dp_mesh_vertex));
    double p = 0.0, r = 0.0;
    const JsonObject acc = side(d_v, nv, sizeof(dp_mesh_vertex), d_truth, n_truth, 12, &p);
    Found f(n_truth);
    const dp_mesh_nearest_stats st = surface(f, d_truth, n_truth, 12, d_v, nv, d_t, nt);
    const JsonObject com = evalstats::side_entry(f.matched(), st.queries, st.matched, tau, &r);
    JsonObject e;
    entries.object("mesh_surface",
                   e.object("accuracy", acc).object("completeness", com).g17("fscore", evalstats::fscore(p, r)));
}

// the vertices of one mesh against the surface of another: the entry and the largest distance
JsonObject Evaluation::deviation_side(const dp_mesh_vertex *d_q, int64_t nq, const dp_mesh_vertex *d_v, int64_t nv,
                                      const int32_t *d_t, int64_t nt, double *top)
{
    Found f(nq);
    const dp_mesh_nearest_stats st = surface(f, d_q, nq, sizeof(dp_mesh_vertex), d_v, nv, d_t, nt);
    return evalstats::deviation_entry(f.matched(), st.queries, st.matched, top);
}

void Evaluation::add_deviation(const char *name, const dp_mesh_vertex *d_va, int64_t nva, const int32_t *d_ta,
                               int64_t nta, const dp_mesh_vertex *d_vb, int64_t nvb, const int32_t *d_tb, int64_t ntb)
{
    double ta = 0.0, tb = 0.0;
    const JsonObject ab = deviation_side(d_va, nva, d_vb, nvb, d_tb, ntb, &ta);
    const JsonObject ba = deviation_side(d_vb, nvb, d_va, nva, d_ta, nta, &tb);
    JsonObject e;
    entries.object(name, e.object("a_to_b", ab).object("b_to_a", ba).g17("max", evalstats::larger(ta, tb)));
}

// --eval-align: the transform that moves the cloud onto the truth (dp_cloud_align_device)
void Evaluation::estimate(const void *d_points, int64_t n, int64_t stride)
{
    std::vector<dp_cloud_align_step> trace((size_t)align_opts.iterations + 1);
    dp_cloud_align_stats st;
    double scale = 1.0;
    check(ctx,
          dp_cloud_align_device(ctx, n ? d_points : nullptr, n, stride, n_truth ? d_truth : nullptr, n_truth, 12,
                                &align_opts, nullptr, M, &scale, trace.data(), nullptr, nullptr, &st, nullptr),
          "dp_cloud_align_device");
    aligned = true;
    const dp_cloud_align_step &last = trace[(size_t)st.iterations_run];
    align_json.array("matrix", M, 12).g17("scale", scale).integer("iterations", st.iterations_run);
    align_json.integer("matched", last.matched).g17("rms_before", trace[0].rms).g17("rms", last.rms);
}

// --eval-align: a copy of n records (the position first) under the transform,
// their normals with them when normal_offset >= 0; without it the records themselves
const void *Evaluation::moved(DeviceMaps &copy, const void *d_records, int64_t n, int64_t stride, int64_t normal_offset)
{
    if (!aligned)
        return d_records;
    void *d = copy.bytes((size_t)n * (size_t)stride, "--eval-align");
    check(ctx, dp_cloud_transform_device(ctx, n ? d_records : nullptr, n, stride, M, normal_offset, d, nullptr),
          "dp_cloud_transform_device");
    return d;
}

void Evaluation::add(const char *name, const void *d_points, int64_t n, int64_t stride, int64_t normal_offset)
{
    static_assert(offsetof(dp_patch, pos) == 0 && offsetof(dp_fused_point, pos) == 0 &&
                      offsetof(dp_mesh_vertex, pos) == 0,
                  "moved() copies records from their positions on");
    if (align && !aligned)
        estimate(d_points, n, stride); // the first cloud added: the written patches
    DeviceMaps copy;
    if (!normals)
        normal_offset = -1;
    d_points = moved(copy, d_points, n, stride, normal_offset);
    double p = 0.0, r = 0.0;
    JsonObject normals_json, e;
    const JsonObject acc = side(d_points, n, stride, d_truth, n_truth, 12, &p, normal_offset, &normals_json);
    const JsonObject com = side(d_truth, n_truth, 12, d_points, n, stride, &r);
    e.object("accuracy", acc).object("completeness", com).g17("fscore", evalstats::fscore(p, r));
    if (normal_offset >= 0)
        e.object("normals", normals_json);
    entries.object(name, e);
}

void Evaluation::report(JsonObject &to) const
{
    to.object("evaluate", entries);
    if (!align_json.empty())
        to.object("align", align_json);
}
