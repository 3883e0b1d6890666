// eval_stats.cpp -- see eval_stats.h.
#include "eval_stats.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

namespace evalstats {

double quantile(const std::vector<double> &d, double p)
{
    if (d.empty())
        return std::nan("");
    const double pos = p * (double)(d.size() - 1);
    const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, d.size() - 1);
    return d[lo] + (d[hi] - d[lo]) * (pos - (double)lo);
}

Matched matched_distances(const std::vector<int32_t> &index, const std::vector<float> &dist)
{
    Matched m;
    for (size_t i = 0; i < index.size(); ++i)
        if (index[i] >= 0) {
            m.d.push_back((double)dist[i]);
            m.sum += (double)dist[i];
        }
    std::sort(m.d.begin(), m.d.end());
    return m;
}

// mean, median and p90 of ascending values and their sum; `unit` ends the keys
static JsonObject &summary(JsonObject &o, const std::vector<double> &d, double sum, const std::string &unit = "")
{
    return o.g17(("mean" + unit).c_str(), d.empty() ? std::nan("") : sum / (double)d.size())
        .g17(("median" + unit).c_str(), quantile(d, 0.5))
        .g17(("p90" + unit).c_str(), quantile(d, 0.9));
}

JsonObject side_entry(const Matched &m, int64_t queries, int64_t matched, double tau, double *ratio)
{
    const int64_t within = (int64_t)(std::upper_bound(m.d.begin(), m.d.end(), tau) - m.d.begin());
    *ratio = queries > 0 ? (double)within / (double)queries : 0.0;
    JsonObject o;
    o.integer("n", queries).integer("matched", matched).integer("within_tau", within).g17("ratio", *ratio);
    return summary(o, m.d, m.sum);
}

JsonObject deviation_entry(const Matched &m, int64_t queries, int64_t matched, double *top)
{
    *top = m.d.empty() ? std::nan("") : m.d.back();
    JsonObject o;
    o.integer("n", queries).integer("matched", matched);
    return summary(o, m.d, m.sum).g17("max", *top);
}

double larger(double a, double b)
{
    return std::isnan(a) ? b : (std::isnan(b) ? a : std::max(a, b));
}

double fscore(double p, double r)
{
    return p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
}

JsonObject normals_entry(const char *records, size_t stride, size_t normal_offset, const std::vector<int32_t> &index,
                         const std::vector<float> &dist, const std::vector<float> &truth_normals, double tau)
{
    std::vector<double> deg;
    double sum = 0.0;
    for (size_t i = 0; i < index.size(); ++i) {
        if (index[i] < 0 || !((double)dist[i] <= tau))
            continue;
        float af[3];
        std::memcpy(af, records + i * stride + normal_offset, 12);
        const float *bf = truth_normals.data() + 3 * (size_t)index[i];
        const double a[3] = {af[0], af[1], af[2]}, b[3] = {bf[0], bf[1], bf[2]};
        bool ok = true, a_any = false, b_any = false;
        for (int k = 0; k < 3; ++k) {
            ok = ok && std::isfinite(a[k]) && std::isfinite(b[k]);
            a_any = a_any || a[k] != 0.0;
            b_any = b_any || b[k] != 0.0;
        }
        if (!ok || !a_any || !b_any)
            continue;
        const double dot = std::fabs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
        const double la = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        const double lb = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        const double angle = std::acos(std::min(1.0, dot / (la * lb))) * (180.0 / 3.14159265358979323846);
        deg.push_back(angle);
        sum += angle;
    }
    std::sort(deg.begin(), deg.end());
    JsonObject o;
    o.integer("n", deg.size());
    return summary(o, deg, sum, "_deg");
}

} // namespace evalstats
