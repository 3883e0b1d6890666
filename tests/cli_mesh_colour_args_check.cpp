// The densify CLI's mesh colour options on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_cli_mesh_colour_cpu.py.
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

// the other mesh options as the parser left them
static bool same_others(const Args &x, const Args &y)
{
    return x.mesh_path == y.mesh_path && x.mesh_dim == y.mesh_dim && x.mesh_smooth == y.mesh_smooth &&
           x.mesh_smooth_lambda == y.mesh_smooth_lambda && x.mesh_smooth_mu == y.mesh_smooth_mu &&
           x.mesh_smooth_free_boundary == y.mesh_smooth_free_boundary && x.mesh_normals == y.mesh_normals &&
           x.mesh_decimate == y.mesh_decimate && x.mesh_decimate_quadric == y.mesh_decimate_quadric &&
           x.mesh_depth_dir == y.mesh_depth_dir && x.mesh_depth_normals == y.mesh_depth_normals &&
           x.mesh_cull_back == y.mesh_cull_back && x.mesh_min_component == y.mesh_min_component &&
           x.mesh_keep_largest == y.mesh_keep_largest && x.depth_dir == y.depth_dir && x.fuse_path == y.fuse_path &&
           x.level == y.level && x.device == y.device && x.gpus == y.gpus && x.iterations == y.iterations;
}

int main()
{
    const char *need_mesh = "--mesh-colour and its options need --mesh";
    const char *need_colour = "--mesh-colour-bilinear, -tol and -min-cos need --mesh-colour";
    { // not given: no stage, the library's defaults
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && !p.a.mesh_colour && !p.a.mesh_colour_bilinear &&
              p.a.mesh_colour_tol < 0.0 && p.a.mesh_colour_min_cos < 0.0);
    }
    { // accepted, alone and with the other mesh stages, in any order
        const Parsed a = parse({"--mesh", "m.ply", "--mesh-colour"});
        CHECK(a.outcome == Parse::Run && a.a.mesh_colour && !a.a.mesh_colour_bilinear && a.a.mesh_colour_tol < 0.0 &&
              a.a.mesh_colour_min_cos < 0.0);
        const Parsed b = parse({"--mesh-colour-min-cos", "0.5", "--mesh-colour-tol", "0.125", "--mesh-colour-bilinear",
                                "--mesh-colour", "--mesh", "m.ply"});
        CHECK(b.outcome == Parse::Run && b.a.mesh_colour && b.a.mesh_colour_bilinear && b.a.mesh_colour_tol == 0.125 &&
              b.a.mesh_colour_min_cos == 0.5);
        const Parsed z = parse({"--mesh", "m.ply", "--mesh-colour", "--mesh-colour-tol", "0", "--mesh-colour-min-cos", "1"});
        CHECK(z.outcome == Parse::Run && z.a.mesh_colour_tol == 0.0 && z.a.mesh_colour_min_cos == 1.0);
    }
    { // every other option parses as it does without the new ones
        const std::vector<const char *> rest = {"--mesh", "m.ply", "--mesh-smooth", "3", "--mesh-smooth-lambda", "0.25",
                                                "--mesh-decimate", "2", "--mesh-decimate-quadric", "--mesh-normals",
                                                "--mesh-depth-maps", "d", "--mesh-cull-back", "--depth-maps", "e",
                                                "--mesh-keep-largest", "1", "--mesh-dim", "40", "--level", "1"};
        const Parsed without = parse(rest);
        std::vector<const char *> with = rest;
        with.insert(with.begin() + 2, {"--mesh-colour", "--mesh-colour-tol", "0.5"});
        with.push_back("--mesh-colour-bilinear");
        const Parsed p = parse(with);
        CHECK(without.outcome == Parse::Run && p.outcome == Parse::Run && same_others(without.a, p.a));
        CHECK(p.a.mesh_colour && p.a.mesh_colour_bilinear && p.a.mesh_colour_tol == 0.5 && !without.a.mesh_colour);
        CHECK(p.a.mesh_smooth == 3 && p.a.mesh_decimate == 2.0 && p.a.mesh_normals && p.a.mesh_depth_dir == "d");
    }
    { // a missing or a bad value
        const Parsed p = parse({"--mesh", "m.ply", "--mesh-colour", "--mesh-colour-tol"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
        const std::vector<std::vector<const char *>> bad = {{"--mesh-colour-tol", "-0.5"}, {"--mesh-colour-tol", "nan"},
                                                            {"--mesh-colour-tol", "inf"},  {"--mesh-colour-tol", "x"},
                                                            {"--mesh-colour-min-cos", "-0.1"},
                                                            {"--mesh-colour-min-cos", "1.5"},
                                                            {"--mesh-colour-min-cos", ""}};
        for (std::vector<const char *> w : bad) {
            w.insert(w.begin(), {"--mesh", "m.ply", "--mesh-colour"});
            const Parsed q = parse(w);
            CHECK(q.outcome == Parse::UsageError && q.error.find(w[3]) == 0);
        }
    }
    { // the missing --mesh
        const std::vector<std::vector<const char *>> alone = {{"--mesh-colour"},
                                                              {"--mesh-colour-bilinear"},
                                                              {"--mesh-colour-tol", "0.5"},
                                                              {"--mesh-colour-min-cos", "0.5"},
                                                              {"--mesh-colour", "--mesh-colour-bilinear"},
                                                              {"--depth-maps", "e", "--mesh-colour"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_mesh);
        }
    }
    { // the details without --mesh-colour
        const std::vector<std::vector<const char *>> flags = {{"--mesh-colour-bilinear"},
                                                              {"--mesh-colour-tol", "0.5"},
                                                              {"--mesh-colour-min-cos", "0"},
                                                              {"--mesh-normals", "--mesh-colour-bilinear"}};
        for (std::vector<const char *> w : flags) {
            w.insert(w.begin(), {"--mesh", "m.ply"});
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_colour);
        }
    }
    if (g_bad)
        return 1;
    std::printf("ok: mesh colour options\n");
    return 0;
}
