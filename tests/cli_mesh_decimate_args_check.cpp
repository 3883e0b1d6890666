// The densify CLI's mesh simplification options on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_cli_mesh_decimate_cpu.py.
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

int main()
{
    const char *need_mesh = "--mesh-decimate and --mesh-decimate-quadric need --mesh";
    const char *need_factor = "--mesh-decimate-quadric needs --mesh-decimate";
    const char *expects = "--mesh-decimate expects a finite number > 0";
    { // not given: no stage
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && p.a.mesh_decimate == 0.0 && !p.a.mesh_decimate_quadric);
    }
    { // accepted values, alone and with the other mesh stages, in any order
        const Parsed a = parse({"--mesh", "m.ply", "--mesh-decimate", "2"});
        CHECK(a.outcome == Parse::Run && a.a.mesh_decimate == 2.0 && !a.a.mesh_decimate_quadric);
        const Parsed b = parse({"--mesh-decimate-quadric", "--mesh-decimate", "0.5", "--mesh", "m.ply"});
        CHECK(b.outcome == Parse::Run && b.a.mesh_decimate == 0.5 && b.a.mesh_decimate_quadric);
        const Parsed c = parse({"--mesh", "m.ply", "--mesh-smooth", "3", "--mesh-decimate", "1e-3", "--mesh-normals",
                                "--mesh-min-component", "8"});
        CHECK(c.outcome == Parse::Run && c.a.mesh_decimate == 1e-3 && c.a.mesh_smooth == 3 && c.a.mesh_normals);
        const Parsed d = parse({"--mesh", "m.ply", "--mesh-decimate", "3e38"});
        CHECK(d.outcome == Parse::Run && d.a.mesh_decimate == 3e38);
    }
    { // refused values, each with the message
        for (const char *v : {"0", "-1", "-0.5", "nan", "inf", "-inf", "1e39", "x", "", "2x"}) {
            const Parsed p = parse({"--mesh", "m.ply", "--mesh-decimate", v});
            CHECK(p.outcome == Parse::UsageError && p.error == expects);
        }
        // a missing value: the usage text is the message
        const Parsed p = parse({"--mesh", "m.ply", "--mesh-decimate"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
    }
    { // the missing --mesh, and -quadric without the factor
        const std::vector<std::vector<const char *>> alone = {
            {"--mesh-decimate", "2"}, {"--mesh-decimate-quadric"}, {"--mesh-decimate", "2", "--mesh-decimate-quadric"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_mesh);
        }
        const Parsed q = parse({"--mesh", "m.ply", "--mesh-decimate-quadric"});
        CHECK(q.outcome == Parse::UsageError && q.error == need_factor);
        const Parsed r = parse({"--mesh", "m.ply", "--mesh-normals", "--mesh-decimate-quadric"});
        CHECK(r.outcome == Parse::UsageError && r.error == need_factor);
    }
    if (g_bad)
        return 1;
    std::printf("ok: mesh simplification options\n");
    return 0;
}
