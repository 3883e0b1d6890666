// The densify CLI's report writer (programs/densify/report_json.h) and its
// evaluation statistics (eval_stats.h/.cpp) on the host: the cases of the file
// named by argv[1], one JSON object a case on stdout.  It needs no HIP header
// and no library, which is the check that those files are free of the GPU.
// Built with the host compiler under ASan + UBSan and run by
// tests/test_cli_report_cpu.py, which writes the cases and judges the answers.
#include "eval_stats.h"
#include "report_json.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

static std::ifstream g_in;

static std::string word()
{
    std::string w;
    if (!(g_in >> w)) {
        std::fprintf(stderr, "the case file ends inside a case\n");
        std::exit(2);
    }
    return w;
}
static double real() { return std::strtod(word().c_str(), nullptr); } // "nan" and "inf" included
static float real32() { return std::strtof(word().c_str(), nullptr); }
static long long whole() { return std::strtoll(word().c_str(), nullptr, 10); }

// N, then N times: index dist
static void search(std::vector<int32_t> &index, std::vector<float> &dist)
{
    const long long n = whole();
    for (long long i = 0; i < n; ++i) {
        index.push_back((int32_t)whole());
        dist.push_back(real32());
    }
}

// side TAU QUERIES MATCHED <search>
static JsonObject side_case()
{
    const double tau = real();
    const long long queries = whole(), matched = whole();
    std::vector<int32_t> index;
    std::vector<float> dist;
    search(index, dist);
    double ratio = -1.0;
    const evalstats::Matched m = evalstats::matched_distances(index, dist);
    const JsonObject e = evalstats::side_entry(m, queries, matched, tau, &ratio);
    JsonObject o;
    return o.object("entry", e).g17("ratio", ratio);
}

// deviation QUERIES MATCHED <search>
static JsonObject deviation_case()
{
    const long long queries = whole(), matched = whole();
    std::vector<int32_t> index;
    std::vector<float> dist;
    search(index, dist);
    double top = -1.0;
    const JsonObject e = evalstats::deviation_entry(evalstats::matched_distances(index, dist), queries, matched, &top);
    JsonObject o;
    return o.object("entry", e).g17("top", top);
}

// normals TAU STRIDE OFFSET NT <3 NT truth floats> NQ, then NQ times: index dist nx ny nz.
// The records are STRIDE bytes of 0xFF each (a NaN to whoever reads a float
// there) with the normal OFFSET bytes in.
static JsonObject normals_case()
{
    const double tau = real();
    const size_t stride = (size_t)whole(), offset = (size_t)whole();
    std::vector<float> truth((size_t)whole() * 3);
    for (float &t : truth)
        t = real32();
    const size_t nq = (size_t)whole();
    std::vector<char> records(nq * stride, (char)0xFF);
    std::vector<int32_t> index;
    std::vector<float> dist;
    for (size_t i = 0; i < nq; ++i) {
        index.push_back((int32_t)whole());
        dist.push_back(real32());
        const float n[3] = {real32(), real32(), real32()};
        std::memcpy(records.data() + i * stride + offset, n, 12);
    }
    // as the CLI hands them over: no byte behind the last record's normal
    records.resize(nq ? (nq - 1) * stride + offset + 12 : 0);
    return evalstats::normals_entry(records.data(), stride, offset, index, dist, truth, tau);
}

// integers N <N values>: members k0 .. k<N-1>
static JsonObject integers_case()
{
    JsonObject o;
    const long long n = whole();
    for (long long i = 0; i < n; ++i)
        o.integer(("k" + std::to_string(i)).c_str(), whole());
    return o;
}

// numbers N <N doubles>: the array and each as a %.17g member
static JsonObject numbers_case()
{
    std::vector<double> v((size_t)whole());
    for (double &x : v)
        x = real();
    JsonObject o, each;
    for (size_t i = 0; i < v.size(); ++i)
        each.g17(("v" + std::to_string(i)).c_str(), v[i]);
    return o.array("array", v.data(), v.size()).object("each", each);
}

// formats X: every other format of the report
static JsonObject formats_case()
{
    const double x = real();
    const int32_t dim[3] = {7, -8, 2147483647};
    JsonObject o, empty, inner, outer;
    o.boolean("yes", true).boolean("no", false).object("empty", empty).string("name", "a b/c.ply");
    o.ms("ms", x).g9("g9", x).g17("g17", x).integer("size", std::numeric_limits<size_t>::max());
    o.integer("least", std::numeric_limits<int64_t>::min()).integer("short", (short)-3).array("dim", dim, 3);
    o.array("none", dim, 0).raw("raw", json_array({empty.str(), "\"s\"", number(x)}));
    outer.object("inner", inner.integer("deep", 1)).members(empty);
    return o.object("outer", outer).members(inner);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: cli_report_check CASES\n");
        return 2;
    }
    g_in.open(argv[1]);
    std::string kind;
    while (g_in >> kind) {
        JsonObject o;
        if (kind == "side")
            o = side_case();
        else if (kind == "deviation")
            o = deviation_case();
        else if (kind == "normals")
            o = normals_case();
        else if (kind == "integers")
            o = integers_case();
        else if (kind == "numbers")
            o = numbers_case();
        else if (kind == "formats")
            o = formats_case();
        else if (kind == "fscore") {
            const double p = real(), r = real();
            o.g17("fscore", evalstats::fscore(p, r));
        } else if (kind == "larger") {
            const double a = real(), b = real();
            o.g17("larger", evalstats::larger(a, b));
        } else if (kind == "quantile") { // quantile P N <N ascending doubles>
            const double p = real();
            std::vector<double> d((size_t)whole());
            for (double &x : d)
                x = real();
            o.g17("quantile", evalstats::quantile(d, p));
        } else {
            std::fprintf(stderr, "unknown case '%s'\n", kind.c_str());
            return 2;
        }
        std::printf("%s\n", o.str().c_str());
    }
    return 0;
}
