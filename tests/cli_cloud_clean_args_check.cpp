// The densify CLI's --fuse-clean-* options on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_cli_cloud_clean_cpu.py.
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

// the clean-up options as a struct that was never parsed into has them
static bool clean_defaults(const Args &x)
{
    return x.fuse_clean_k == 0 && x.fuse_clean_radius == 0.0 && x.fuse_clean_std == -1.0 &&
           x.fuse_clean_min_neighbours == 0 && !x.fuse_clean_radius_only && !x.fuse_clean();
}

// the other options as the parser left them
static bool same_others(const Args &x, const Args &y)
{
    return x.mesh_path == y.mesh_path && x.mesh_dim == y.mesh_dim && x.mesh_smooth == y.mesh_smooth &&
           x.depth_dir == y.depth_dir && x.fuse_path == y.fuse_path && x.level == y.level && x.device == y.device &&
           x.gpus == y.gpus && x.iterations == y.iterations && x.seeds_path == y.seeds_path && x.output == y.output &&
           x.check_only == y.check_only && x.do_filter == y.do_filter && x.eval_path == y.eval_path &&
           x.eval_tau == y.eval_tau && x.fuse.min_views == y.fuse.min_views && x.fuse.depth_tol == y.fuse.depth_tol &&
           x.refine_passes == y.refine_passes && x.splat_scale == y.splat_scale;
}

int main()
{
    const char *need_fuse = "--fuse-clean-k, -radius, -std, -min-neighbours and -radius-only need --fuse";
    const char *together =
        "--fuse-clean-k and --fuse-clean-radius go together, and the other --fuse-clean options need both";
    const char *min_nb = "--fuse-clean-min-neighbours expects 1..K of --fuse-clean-k";
    { // not given: the defaults, with and without --fuse
        CHECK(clean_defaults(Args()));
        const Parsed p = parse({"--fuse", "f.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && clean_defaults(p.a));
        const Parsed q = parse({"--mesh", "m.ply"});
        CHECK(q.outcome == Parse::Run && clean_defaults(q.a));
    }
    { // accepted: the defaults resolved, every option given, the ends of the ranges
        const Parsed a = parse({"--fuse", "f.ply", "--fuse-clean-k", "8", "--fuse-clean-radius", "0.25"});
        CHECK(a.outcome == Parse::Run && a.error.empty() && a.a.fuse_clean() && a.a.fuse_clean_k == 8 &&
              a.a.fuse_clean_radius == 0.25 && a.a.fuse_clean_std == 2.0 && a.a.fuse_clean_min_neighbours == 1 &&
              !a.a.fuse_clean_radius_only);
        const Parsed b = parse({"--fuse-clean-radius-only", "--fuse-clean-min-neighbours", "3", "--fuse-clean-std", "0",
                                "--fuse-clean-radius", "1e-3", "--fuse-clean-k", "3", "--fuse", "f.ply"});
        CHECK(b.outcome == Parse::Run && b.a.fuse_clean_k == 3 && b.a.fuse_clean_radius == 1e-3 &&
              b.a.fuse_clean_std == 0.0 && b.a.fuse_clean_min_neighbours == 3 && b.a.fuse_clean_radius_only);
        const Parsed c = parse({"--fuse", "f.ply", "--fuse-clean-k", "1", "--fuse-clean-radius", "3e38"});
        CHECK(c.outcome == Parse::Run && c.a.fuse_clean_k == 1);
        const Parsed d = parse({"--fuse", "f.ply", "--fuse-clean-k", "32", "--fuse-clean-radius", "1",
                                "--fuse-clean-min-neighbours", "32", "--fuse-clean-std", "1.5", "--check-only"});
        CHECK(d.outcome == Parse::Run && d.a.fuse_clean_k == 32 && d.a.fuse_clean_min_neighbours == 32 &&
              d.a.fuse_clean_std == 1.5 && d.a.check_only);
    }
    { // every other option parses as it does without the new ones
        const std::vector<const char *> rest = {"--mesh", "m.ply", "--mesh-smooth", "3", "--fuse", "f.ply", "--seeds",
                                                "s.xyz", "-o", "p.ply", "--mesh-dim", "40", "--level", "1", "--filter",
                                                "--fuse-min-views", "3", "--evaluate", "t.xyz", "--eval-tau", "0.5"};
        const Parsed without = parse(rest);
        std::vector<const char *> with = rest;
        with.insert(with.begin() + 2, {"--fuse-clean-k", "16", "--fuse-clean-radius", "0.5"});
        with.push_back("--fuse-clean-radius-only");
        const Parsed p = parse(with);
        CHECK(without.outcome == Parse::Run && p.outcome == Parse::Run && same_others(without.a, p.a));
        CHECK(clean_defaults(without.a) && p.a.fuse_clean_k == 16 && p.a.fuse_clean_radius_only);
    }
    { // a missing or a bad value
        const Parsed p = parse({"--fuse", "f.ply", "--fuse-clean-radius", "1", "--fuse-clean-k"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
        const std::vector<std::vector<const char *>> bad = {
            {"--fuse-clean-k", "0"},          {"--fuse-clean-k", "33"},         {"--fuse-clean-k", "-1"},
            {"--fuse-clean-k", "8.5"},        {"--fuse-clean-k", "x"},          {"--fuse-clean-k", ""},
            {"--fuse-clean-radius", "0"},     {"--fuse-clean-radius", "-1"},    {"--fuse-clean-radius", "nan"},
            {"--fuse-clean-radius", "inf"},   {"--fuse-clean-radius", "1e39"},  {"--fuse-clean-radius", "1e-50"},
            {"--fuse-clean-radius", "0.5x"},  {"--fuse-clean-std", "-0.5"},     {"--fuse-clean-std", "nan"},
            {"--fuse-clean-std", "inf"},      {"--fuse-clean-std", "1e39"},     {"--fuse-clean-std", "two"},
            {"--fuse-clean-min-neighbours", "0"}, {"--fuse-clean-min-neighbours", "33"},
            {"--fuse-clean-min-neighbours", "1.0"}};
        for (std::vector<const char *> w : bad) {
            w.insert(w.begin(), {"--fuse", "f.ply"});
            const Parsed r = parse(w);
            CHECK(r.outcome == Parse::UsageError && r.error.find(w[2]) == 0 && r.error.find("expects") != std::string::npos);
        }
    }
    { // K and R go together, and the details need both
        const std::vector<std::vector<const char *>> half = {{"--fuse-clean-k", "8"},
                                                             {"--fuse-clean-radius", "0.5"},
                                                             {"--fuse-clean-std", "2"},
                                                             {"--fuse-clean-min-neighbours", "1"},
                                                             {"--fuse-clean-radius-only"},
                                                             {"--fuse-clean-k", "8", "--fuse-clean-std", "1"},
                                                             {"--fuse-clean-radius", "1", "--fuse-clean-radius-only"}};
        for (std::vector<const char *> w : half) {
            const Parsed alone = parse(w);
            CHECK(alone.outcome == Parse::UsageError && alone.error == need_fuse);
            w.insert(w.begin(), {"--fuse", "f.ply"});
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == together);
        }
        // complete, but without --fuse (with --mesh, with --check-only)
        const Parsed q = parse({"--fuse-clean-k", "8", "--fuse-clean-radius", "0.5"});
        CHECK(q.outcome == Parse::UsageError && q.error == need_fuse);
        const Parsed r = parse({"--mesh", "m.ply", "--check-only", "--fuse-clean-k", "8", "--fuse-clean-radius", "0.5"});
        CHECK(r.outcome == Parse::UsageError && r.error == need_fuse);
    }
    { // min_neighbours is at most K
        const Parsed p = parse({"--fuse", "f.ply", "--fuse-clean-k", "4", "--fuse-clean-radius", "1",
                                "--fuse-clean-min-neighbours", "5"});
        CHECK(p.outcome == Parse::UsageError && p.error == min_nb);
        const Parsed q = parse({"--fuse", "f.ply", "--fuse-clean-min-neighbours", "4", "--fuse-clean-k", "4",
                                "--fuse-clean-radius", "1"});
        CHECK(q.outcome == Parse::Run && q.a.fuse_clean_min_neighbours == 4);
    }
    if (g_bad)
        return 1;
    std::printf("ok: fuse-clean options\n");
    return 0;
}
