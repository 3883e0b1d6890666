// The densify CLI's mesh smoothing and normals options on the host: parse_args
// of programs/densify/cli_args.cpp fed whole command lines, with stand-ins for
// the three dp_default_* functions it calls (no library, no device).  Built with
// the host compiler under ASan + UBSan and run by tests/test_cli_mesh_smooth_cpu.py.
#include "cli_args.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>
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

// with --mesh given, so that only the value can be at fault
static bool refuses(const char *option, const char *value, const char *message)
{
    const Parsed p = parse({"--mesh", "m.ply", "--mesh-smooth", "1", option, value});
    return p.outcome == Parse::UsageError && p.error == message;
}

int main()
{
    const char *need_mesh = "--mesh-smooth, its options and --mesh-normals need --mesh";
    const char *need_smooth = "--mesh-smooth-lambda, -mu and -free-boundary need --mesh-smooth";
    { // none given: neither stage
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && p.a.mesh_smooth < 0 && !p.a.mesh_normals);
        CHECK(!p.a.mesh_smooth_free_boundary && p.a.mesh_smooth_lambda == 0.0 && p.a.mesh_smooth_mu > 0.0);
    }
    { // the flags parse, alone and together, at their limits
        const Parsed s = parse({"--mesh", "m.ply", "--mesh-smooth", "3"});
        CHECK(s.outcome == Parse::Run && s.a.mesh_smooth == 3 && !s.a.mesh_normals && s.a.mesh_smooth_mu > 0.0);
        const Parsed n = parse({"--mesh-normals", "--mesh", "m.ply"});
        CHECK(n.outcome == Parse::Run && n.a.mesh_normals && n.a.mesh_smooth < 0);
        const Parsed all = parse({"--mesh", "m.ply", "--mesh-smooth", "1000", "--mesh-smooth-lambda", "1", "--mesh-smooth-mu",
                                  "0", "--mesh-smooth-free-boundary", "--mesh-normals"});
        CHECK(all.outcome == Parse::Run && all.a.mesh_smooth == 1000 && all.a.mesh_smooth_lambda == 1.0);
        CHECK(all.a.mesh_smooth_mu == 0.0 && all.a.mesh_smooth_free_boundary && all.a.mesh_normals);
        const Parsed z = parse({"--mesh", "m.ply", "--mesh-smooth", "0", "--mesh-smooth-lambda", "0.25", "--mesh-smooth-mu",
                                "-0.26"});
        CHECK(z.outcome == Parse::Run && z.a.mesh_smooth == 0 && z.a.mesh_smooth_lambda == 0.25 &&
              z.a.mesh_smooth_mu == -0.26);
    }
    { // refused without --mesh, each with the message
        const std::vector<std::vector<const char *>> alone = {
            {"--mesh-smooth", "3"}, {"--mesh-normals"}, {"--mesh-smooth-free-boundary"}, {"--mesh-smooth-lambda", "0.5"},
            {"--mesh-smooth-mu", "-0.5"}, {"--mesh-smooth", "3", "--mesh-normals", "--mesh-smooth-mu", "0"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_mesh);
        }
        // the smoothing's details without the smoothing
        const std::vector<std::vector<const char *>> details = {
            {"--mesh", "m.ply", "--mesh-smooth-lambda", "0.5"}, {"--mesh", "m.ply", "--mesh-smooth-mu", "0"},
            {"--mesh", "m.ply", "--mesh-normals", "--mesh-smooth-free-boundary"}};
        for (const std::vector<const char *> &w : details) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_smooth);
        }
    }
    { // the limits, just outside them, and values that are no numbers
        for (const char *v : {"-1", "1001", "x", "", "3x", "1.5"})
            CHECK(refuses("--mesh-smooth", v, "--mesh-smooth expects 0..1000"));
        for (const char *v : {"0", "-0.1", "1.0001", "nan", "inf", "x", "", "0.5x", "1e-60"})
            CHECK(refuses("--mesh-smooth-lambda", v, "--mesh-smooth-lambda expects a number in (0, 1]"));
        for (const char *v : {"0.1", "nan", "inf", "-inf", "-1e39", "x", "", "-0.5x"})
            CHECK(refuses("--mesh-smooth-mu", v, "--mesh-smooth-mu expects a finite number <= 0"));
        // a missing value: the usage text is the message
        const Parsed p = parse({"--mesh", "m.ply", "--mesh-smooth"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
    }
    if (g_bad)
        return 1;
    std::printf("ok: mesh smoothing and normals options\n");
    return 0;
}
