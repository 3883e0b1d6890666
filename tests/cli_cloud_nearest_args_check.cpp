// The densify CLI's --evaluate, --eval-tau and --eval-max-dist options on the
// host: parse_args of programs/densify/cli_args.cpp fed whole command lines, with
// stand-ins for the three dp_default_* functions it calls (no library, no
// device).  Built with the host compiler under ASan + UBSan and run by
// tests/test_cli_cloud_nearest_cpu.py.
#include "cli_args.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

extern "C" void dp_default_matcher_options(dp_matcher_options *m) { std::memset(m, 0, sizeof *m); }
extern "C" void dp_default_fast_options(dp_fast_options *f) { std::memset(f, 0, sizeof *f); }
extern "C" void dp_default_fuse_options(dp_fuse_options *f) { std::memset(f, 0, sizeof *f); }

static int g_bad = 0;
#define CHECK(x) ((x) ? (void)0 : (void)(++g_bad, std::printf("FAIL line %d: %s\n", __LINE__, #x)))

struct Parsed {
    Parse outcome;
    Args a;
    std::string error;
};

static Parsed parse(const std::vector<const char *> &words)
{
    std::vector<std::string> store{"densify", "-i", "x"};
    store.insert(store.end(), words.begin(), words.end());
    std::vector<char *> argv;
    for (std::string &s : store)
        argv.push_back(&s[0]);
    argv.push_back(nullptr);
    Parsed p;
    p.error = "stale";
    p.outcome = parse_args((int)store.size(), argv.data(), p.a, p.error);
    return p;
}

// the other options as the parser left them
static bool same_others(const Args &x, const Args &y)
{
    return x.mesh_path == y.mesh_path && x.mesh_dim == y.mesh_dim && x.mesh_smooth == y.mesh_smooth &&
           x.mesh_normals == y.mesh_normals && x.mesh_decimate == y.mesh_decimate && x.mesh_colour == y.mesh_colour &&
           x.depth_dir == y.depth_dir && x.fuse_path == y.fuse_path && x.level == y.level && x.device == y.device &&
           x.gpus == y.gpus && x.iterations == y.iterations && x.seeds_path == y.seeds_path && x.output == y.output &&
           x.check_only == y.check_only && x.do_filter == y.do_filter;
}

int main()
{
    const char *need_eval = "--eval-tau and --eval-max-dist need --evaluate";
    const char *need_tau = "--evaluate needs --eval-tau";
    const char *small = "--eval-max-dist expects a finite number of at least --eval-tau";
    { // not given: no evaluation
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && p.a.eval_path.empty() && p.a.eval_tau == 0.0 &&
              p.a.eval_max_dist == 0.0);
    }
    { // accepted: the radius defaults to ten thresholds, or is given, down to the threshold itself
        const Parsed a = parse({"--evaluate", "t.xyz", "--eval-tau", "0.25"});
        CHECK(a.outcome == Parse::Run && a.error.empty() && a.a.eval_path == "t.xyz" && a.a.eval_tau == 0.25 &&
              a.a.eval_max_dist == 2.5);
        const Parsed b = parse({"--eval-max-dist", "0.75", "--eval-tau", "0.5", "--evaluate", "t.xyz"});
        CHECK(b.outcome == Parse::Run && b.a.eval_tau == 0.5 && b.a.eval_max_dist == 0.75);
        const Parsed c = parse({"--evaluate", "t.xyz", "--eval-tau", "0.5", "--eval-max-dist", "0.5"});
        CHECK(c.outcome == Parse::Run && c.a.eval_max_dist == 0.5);
        const Parsed d = parse({"--evaluate", "t.xyz", "--eval-tau", "1e-3", "--check-only"});
        CHECK(d.outcome == Parse::Run && d.a.check_only && d.a.eval_tau == 1e-3 && d.a.eval_max_dist == 10.0 * 1e-3);
    }
    { // every other option parses as it does without the new ones
        const std::vector<const char *> rest = {"--mesh", "m.ply", "--mesh-smooth", "3", "--mesh-colour", "--fuse", "f.ply",
                                                "--seeds", "s.xyz", "-o", "p.ply", "--mesh-dim", "40", "--level", "1",
                                                "--filter"};
        const Parsed without = parse(rest);
        std::vector<const char *> with = rest;
        with.insert(with.begin() + 2, {"--evaluate", "t.xyz", "--eval-tau", "0.125"});
        with.push_back("--eval-max-dist");
        with.push_back("4");
        const Parsed p = parse(with);
        CHECK(without.outcome == Parse::Run && p.outcome == Parse::Run && same_others(without.a, p.a));
        CHECK(p.a.eval_path == "t.xyz" && p.a.eval_tau == 0.125 && p.a.eval_max_dist == 4.0 && without.a.eval_path.empty());
        CHECK(p.a.seeds_path == "s.xyz" && p.a.fuse_path == "f.ply" && p.a.mesh_smooth == 3);
    }
    { // a missing or a bad value
        const Parsed p = parse({"--evaluate", "t.xyz", "--eval-tau"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
        const Parsed q = parse({"--eval-tau", "1", "--evaluate"});
        CHECK(q.outcome == Parse::UsageError && q.error.empty());
        const std::vector<std::vector<const char *>> bad = {
            {"--eval-tau", "0"},      {"--eval-tau", "-1"},       {"--eval-tau", "nan"},       {"--eval-tau", "inf"},
            {"--eval-tau", "x"},      {"--eval-tau", ""},         {"--eval-tau", "1e39"},      {"--eval-tau", "1e-50"},
            {"--eval-tau", "0.5x"},   {"--eval-max-dist", "0"},   {"--eval-max-dist", "-2"},   {"--eval-max-dist", "nan"},
            {"--eval-max-dist", "inf"}, {"--eval-max-dist", "1e39"}, {"--eval-max-dist", "two"}};
        for (std::vector<const char *> w : bad) {
            w.insert(w.begin(), {"--evaluate", "t.xyz"});
            const Parsed r = parse(w);
            CHECK(r.outcome == Parse::UsageError && r.error.find(w[2]) == 0 && r.error.find("expects") != std::string::npos);
        }
    }
    { // the threshold is required, and the radius may not be below it
        const Parsed p = parse({"--evaluate", "t.xyz"});
        CHECK(p.outcome == Parse::UsageError && p.error == need_tau);
        const Parsed q = parse({"--evaluate", "t.xyz", "--eval-max-dist", "2"});
        CHECK(q.outcome == Parse::UsageError && q.error == need_tau);
        const Parsed r = parse({"--evaluate", "t.xyz", "--eval-tau", "0.5", "--eval-max-dist", "0.25"});
        CHECK(r.outcome == Parse::UsageError && r.error == small);
        const Parsed s = parse({"--evaluate", "t.xyz", "--eval-tau", "1e38"}); // ten thresholds are no float
        CHECK(s.outcome == Parse::UsageError && s.error == small);
    }
    { // the details without --evaluate, --check-only included
        const std::vector<std::vector<const char *>> alone = {{"--eval-tau", "0.5"},
                                                              {"--eval-max-dist", "2"},
                                                              {"--eval-tau", "0.5", "--eval-max-dist", "2"},
                                                              {"--check-only", "--eval-tau", "0.5"},
                                                              {"--mesh", "m.ply", "--eval-max-dist", "2"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_eval);
        }
    }
    if (g_bad)
        return 1;
    std::printf("ok: evaluate options\n");
    return 0;
}
