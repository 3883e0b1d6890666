// evaluate.h -- --evaluate: the ground-truth points on the device and, per
// evaluated cloud, the report's entry.  A cloud is searched where it lies
// (dp_cloud_nearest_device, both directions, radius --eval-max-dist); only index
// and dist come back, and eval_stats.h makes the entry of them on the host.
#pragma once

#include "device_maps.h"

#include <cstddef>
#include <cstdint>
#include <vector>

class Evaluation {
public:
    Evaluation(dp_ctx *ctx, const Args &args, const std::vector<double> &truth);

    // the cloud of n points at d_points (device memory, `stride` bytes apart, each the head
    // of its record) against the truth; normal_offset: where a record's normal
    // lies, for --eval-normals (-1: the records have none)
    void add(const char *name, const void *d_points, int64_t n, int64_t stride, int64_t normal_offset = -1);

    // host records, uploaded first
    template <typename T>
    void add_host(const char *name, const std::vector<T> &recs, size_t pos_offset, int64_t normal_offset = -1)
    {
        DeviceMaps up;
        char *d = (char *)up.bytes(recs.size() * sizeof(T), "--evaluate");
        upload(d, recs, "--evaluate: copy of a cloud failed");
        add(name, d + pos_offset, (int64_t)recs.size(), (int64_t)sizeof(T), normal_offset);
    }

    // --eval-mesh-surface: the mesh's vertices against the truth and the truth
    // against the mesh's surface
    void add_mesh_surface(const dp_mesh_vertex *d_v, int64_t nv, const int32_t *d_t, int64_t nt);

    // --eval-mesh-surface with --mesh-decimate: mesh a (before) and mesh b (after), both ways
    void add_deviation(const char *name, const dp_mesh_vertex *d_va, int64_t nva, const int32_t *d_ta, int64_t nta,
                       const dp_mesh_vertex *d_vb, int64_t nvb, const int32_t *d_tb, int64_t ntb);

    // "evaluate" and, with --eval-align, "align" into the report
    void report(JsonObject &to) const;

private:
    struct Found; // the results of one search: indices and distances on the device

    void estimate(const void *d_points, int64_t n, int64_t stride);
    const void *moved(DeviceMaps &copy, const void *d_records, int64_t n, int64_t stride, int64_t normal_offset = -1);
    JsonObject side(const void *d_q, int64_t nq, int64_t qs, const void *d_t, int64_t nt, int64_t ts, double *ratio,
                    int64_t normal_offset = -1, JsonObject *normals_json = nullptr);
    JsonObject normals_entry(const Found &f, const void *d_q, int64_t nq, int64_t qs, int64_t normal_offset);
    dp_mesh_nearest_stats surface(const Found &f, const void *d_q, int64_t nq, int64_t qs, const dp_mesh_vertex *d_v,
                                  int64_t nv, const int32_t *d_t, int64_t nt);
    JsonObject deviation_side(const dp_mesh_vertex *d_q, int64_t nq, const dp_mesh_vertex *d_v, int64_t nv,
                              const int32_t *d_t, int64_t nt, double *top);

    dp_ctx *ctx = nullptr;
    double tau = 0.0;
    float max_dist = 0.0f;
    int64_t n_truth = 0;
    DeviceMaps mem;
    float *d_truth = nullptr;
    JsonObject entries;
    // --eval-align: the options, the transform once it is estimated, the report's member
    dp_cloud_align_options align_opts{};
    bool align = false, aligned = false;
    double M[12] = {0};
    JsonObject align_json;
    // --eval-normals: the options and the truth's normals once they are estimated
    dp_cloud_normals_options normals_opts{};
    bool normals = false;
    float *d_truth_normal = nullptr;
};
