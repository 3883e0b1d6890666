// The densify CLI's --eval-mesh-surface option on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_cli_mesh_nearest_cpu.py.
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
           x.mesh_normals == y.mesh_normals && x.mesh_decimate == y.mesh_decimate &&
           x.mesh_decimate_quadric == y.mesh_decimate_quadric && x.mesh_colour == y.mesh_colour &&
           x.fuse_path == y.fuse_path && x.level == y.level && x.device == y.device && x.gpus == y.gpus &&
           x.output == y.output && x.check_only == y.check_only && x.do_filter == y.do_filter &&
           x.eval_path == y.eval_path && x.eval_tau == y.eval_tau && x.eval_max_dist == y.eval_max_dist;
}

int main()
{
    const char *need = "--eval-mesh-surface needs --evaluate and --mesh";
    { // not given: off
        const Parsed p = parse({"--mesh", "m.ply", "--evaluate", "t.xyz", "--eval-tau", "0.5"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && !p.a.eval_mesh_surface);
    }
    { // accepted with both, in any order, with and without the simplification
        const Parsed a = parse({"--eval-mesh-surface", "--mesh", "m.ply", "--evaluate", "t.xyz", "--eval-tau", "0.5"});
        CHECK(a.outcome == Parse::Run && a.error.empty() && a.a.eval_mesh_surface && a.a.eval_max_dist == 5.0);
        const Parsed b = parse({"--mesh", "m.ply", "--mesh-decimate", "2", "--mesh-decimate-quadric", "--evaluate", "t.xyz",
                                "--eval-tau", "0.5", "--eval-max-dist", "0.75", "--eval-mesh-surface", "--check-only"});
        CHECK(b.outcome == Parse::Run && b.a.eval_mesh_surface && b.a.mesh_decimate == 2.0 && b.a.check_only);
    }
    { // every other option parses as it does without the new one
        const std::vector<const char *> rest = {"--mesh", "m.ply", "--mesh-smooth", "3", "--mesh-colour", "--fuse", "f.ply",
                                                "--evaluate", "t.xyz", "--eval-tau", "0.125", "-o", "p.ply", "--mesh-dim",
                                                "40", "--mesh-decimate", "1.5", "--filter"};
        const Parsed without = parse(rest);
        std::vector<const char *> with = rest;
        with.insert(with.begin() + 4, "--eval-mesh-surface");
        const Parsed p = parse(with);
        CHECK(without.outcome == Parse::Run && p.outcome == Parse::Run && same_others(without.a, p.a));
        CHECK(p.a.eval_mesh_surface && !without.a.eval_mesh_surface);
    }
    { // it takes no value: the next word is an option of its own
        const Parsed p = parse({"--mesh", "m.ply", "--evaluate", "t.xyz", "--eval-tau", "0.5", "--eval-mesh-surface", "1"});
        CHECK(p.outcome == Parse::UsageError);
    }
    { // without --evaluate, without --mesh, without either; --check-only included
        const std::vector<std::vector<const char *>> alone = {
            {"--eval-mesh-surface"},
            {"--eval-mesh-surface", "--mesh", "m.ply"},
            {"--eval-mesh-surface", "--mesh", "m.ply", "--mesh-decimate", "2"},
            {"--eval-mesh-surface", "--evaluate", "t.xyz", "--eval-tau", "0.5"},
            {"--eval-mesh-surface", "--evaluate", "t.xyz", "--eval-tau", "0.5", "--fuse", "f.ply"},
            {"--check-only", "--eval-mesh-surface"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need);
        }
    }
    if (g_bad)
        return 1;
    std::printf("ok: eval-mesh-surface option\n");
    return 0;
}
