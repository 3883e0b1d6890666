// eval_stats.h -- the host arithmetic of --evaluate: what Evaluation
// (evaluate.h) makes of the indices and distances its searches return.  The C++
// twins of cloud_quantile, cloud_side and cloud_normal_error of
// densepoints_amd/pmvs.py, operation for operation in fp64; a statistic over no
// value is NaN, which the report writes as null.  No GPU, nothing of the library.
#pragma once

#include "report_json.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace evalstats {

// d[lo] + (d[min(lo + 1, m - 1)] - d[lo]) * (pos - lo), pos = p (m - 1), of ascending values
double quantile(const std::vector<double> &d, double p);

// the matched distances of a search (index >= 0), ascending, and their sum in index order
struct Matched {
    std::vector<double> d;
    double sum = 0.0;
};
Matched matched_distances(const std::vector<int32_t> &index, const std::vector<float> &dist);

// one direction of an evaluation: n, matched, within_tau (<= tau), ratio, mean,
// median, p90; *ratio = within_tau / n, 0 when n is 0
JsonObject side_entry(const Matched &m, int64_t queries, int64_t matched, double tau, double *ratio);

// one direction of a deviation: n, matched, mean, median, p90, max; *top = max
JsonObject deviation_entry(const Matched &m, int64_t queries, int64_t matched, double *top);

// the larger of two maxima of which either may be NaN (nothing matched)
double larger(double a, double b);

// 2 p r / (p + r), 0 when both are 0
double fscore(double p, double r);

// cloud_normal_error: query i (its normal `normal_offset` bytes into record i,
// the records `stride` bytes apart) counts iff index[i] >= 0, dist[i] <= tau and
// its normal and truth_normals[index[i]] are finite and not zero; the unsigned
// angles between the two, in degrees: n, mean_deg, median_deg, p90_deg
JsonObject normals_entry(const char *records, size_t stride, size_t normal_offset, const std::vector<int32_t> &index,
                         const std::vector<float> &dist, const std::vector<float> &truth_normals, double tau);

} // namespace evalstats
