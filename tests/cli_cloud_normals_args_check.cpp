// The densify CLI's --eval-normals, --eval-normals-k and --eval-normals-radius
// options on the host: parse_args of programs/densify/cli_args.cpp fed whole
// command lines, with stand-ins for the three dp_default_* functions it calls (no
// library, no device).  Built with the host compiler under ASan + UBSan and run
// by tests/test_cli_cloud_normals_cpu.py.
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
    return x.mesh_path == y.mesh_path && x.mesh_dim == y.mesh_dim && x.fuse_path == y.fuse_path && x.level == y.level &&
           x.device == y.device && x.gpus == y.gpus && x.iterations == y.iterations && x.seeds_path == y.seeds_path &&
           x.output == y.output && x.check_only == y.check_only && x.do_filter == y.do_filter &&
           x.eval_path == y.eval_path && x.eval_tau == y.eval_tau && x.eval_max_dist == y.eval_max_dist &&
           x.eval_mesh_surface == y.eval_mesh_surface && x.eval_align == y.eval_align &&
           x.eval_align_iterations == y.eval_align_iterations && x.eval_align_radius == y.eval_align_radius &&
           x.eval_align_scale == y.eval_align_scale;
}

int main()
{
    const char *need_normals = "--eval-normals-k and -radius need --eval-normals";
    const char *need_eval = "--eval-normals needs --evaluate";
    const std::vector<const char *> ev = {"--evaluate", "t.xyz", "--eval-tau", "0.25"};
    auto with = [&ev](std::vector<const char *> w) {
        w.insert(w.begin(), ev.begin(), ev.end());
        return w;
    };
    { // not given: no normals, nothing resolved
        const Parsed p = parse(ev);
        CHECK(p.outcome == Parse::Run && p.error.empty() && !p.a.eval_normals && p.a.eval_normals_k == 0 &&
              p.a.eval_normals_radius == 0.0);
    }
    { // accepted: the defaults are 16 neighbours and the evaluation's radius
        const Parsed a = parse(with({"--eval-normals"}));
        CHECK(a.outcome == Parse::Run && a.error.empty() && a.a.eval_normals && a.a.eval_normals_k == 16 &&
              a.a.eval_normals_radius == 2.5);
        const Parsed b = parse(with({"--eval-max-dist", "0.75", "--eval-normals"}));
        CHECK(b.outcome == Parse::Run && b.a.eval_normals_radius == 0.75);
        const Parsed c = parse({"--eval-normals-radius", "0.125", "--eval-normals-k", "32", "--eval-normals", "--evaluate",
                                "t.xyz", "--eval-tau", "0.25"});
        CHECK(c.outcome == Parse::Run && c.a.eval_normals && c.a.eval_normals_k == 32 &&
              c.a.eval_normals_radius == 0.125 && c.a.eval_max_dist == 2.5);
        const Parsed d = parse(with({"--eval-normals", "--eval-normals-k", "3", "--check-only"}));
        CHECK(d.outcome == Parse::Run && d.a.check_only && d.a.eval_normals_k == 3);
        const Parsed e = parse(with({"--eval-normals", "--eval-normals-radius", "1e-3"})); // below the threshold is allowed
        CHECK(e.outcome == Parse::Run && e.a.eval_normals_radius == 1e-3);
        // with the registration: each keeps its own radius
        const Parsed f = parse(with({"--eval-align", "--eval-align-radius", "4", "--eval-normals"}));
        CHECK(f.outcome == Parse::Run && f.a.eval_align && f.a.eval_align_radius == 4.0 && f.a.eval_normals_radius == 2.5);
    }
    { // every other option parses as it does without the new ones
        const std::vector<const char *> rest =
            with({"--mesh", "m.ply", "--fuse", "f.ply", "--seeds", "s.xyz", "-o", "p.ply", "--mesh-dim", "40", "--level",
                  "1", "--filter", "--eval-mesh-surface", "--eval-align", "--eval-align-iterations", "7"});
        const Parsed without = parse(rest);
        std::vector<const char *> more = rest;
        more.insert(more.begin() + 6, {"--eval-normals", "--eval-normals-k", "9"});
        more.push_back("--eval-normals-radius");
        more.push_back("0.5");
        const Parsed p = parse(more);
        CHECK(without.outcome == Parse::Run && p.outcome == Parse::Run && same_others(without.a, p.a));
        CHECK(p.a.eval_normals && p.a.eval_normals_k == 9 && p.a.eval_normals_radius == 0.5 && !without.a.eval_normals);
        CHECK(p.a.seeds_path == "s.xyz" && p.a.fuse_path == "f.ply" && p.a.eval_align_iterations == 7);
    }
    { // a missing or a bad value
        const Parsed p = parse(with({"--eval-normals", "--eval-normals-k"}));
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
        const Parsed q = parse(with({"--eval-normals", "--eval-normals-radius"}));
        CHECK(q.outcome == Parse::UsageError && q.error.empty());
        const std::vector<std::vector<const char *>> bad = {
            {"--eval-normals-k", "2"},        {"--eval-normals-k", "33"},        {"--eval-normals-k", "0"},
            {"--eval-normals-k", "-3"},       {"--eval-normals-k", "x"},         {"--eval-normals-k", ""},
            {"--eval-normals-k", "8.5"},      {"--eval-normals-k", "16x"},       {"--eval-normals-radius", "0"},
            {"--eval-normals-radius", "-2"},  {"--eval-normals-radius", "nan"},  {"--eval-normals-radius", "inf"},
            {"--eval-normals-radius", "1e39"}, {"--eval-normals-radius", "1e-50"}, {"--eval-normals-radius", "two"},
            {"--eval-normals-radius", "0.5x"}};
        for (std::vector<const char *> w : bad) {
            const std::string opt = w[0];
            w.insert(w.begin(), "--eval-normals");
            const Parsed r = parse(with(w));
            CHECK(r.outcome == Parse::UsageError && r.error.find(opt) == 0 && r.error.find("expects") != std::string::npos);
        }
    }
    { // the details without --eval-normals, --check-only included
        const std::vector<std::vector<const char *>> alone = {{"--eval-normals-k", "5"},
                                                              {"--eval-normals-radius", "2"},
                                                              {"--check-only", "--eval-normals-k", "5"},
                                                              {"--eval-normals-k", "5", "--eval-normals-radius", "2"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(with(w));
            CHECK(p.outcome == Parse::UsageError && p.error == need_normals);
            const Parsed q = parse(w); // and without --evaluate: the same message comes first
            CHECK(q.outcome == Parse::UsageError && q.error == need_normals);
        }
    }
    { // --eval-normals without --evaluate
        const Parsed p = parse({"--eval-normals"});
        CHECK(p.outcome == Parse::UsageError && p.error == need_eval);
        const Parsed q = parse({"--eval-normals", "--eval-normals-k", "5", "--fuse", "f.ply"});
        CHECK(q.outcome == Parse::UsageError && q.error == need_eval);
        const Parsed r = parse({"--eval-normals", "--eval-tau", "0.5"}); // the older rule speaks first
        CHECK(r.outcome == Parse::UsageError && r.error == "--eval-tau and --eval-max-dist need --evaluate");
        const Parsed s = parse({"--eval-normals", "--evaluate", "t.xyz"});
        CHECK(s.outcome == Parse::UsageError && s.error == "--evaluate needs --eval-tau");
    }
    if (g_bad)
        return 1;
    std::printf("ok: eval-normals options\n");
    return 0;
}
