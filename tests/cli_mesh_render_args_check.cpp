// The densify CLI's mesh render options on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_cli_mesh_render_cpu.py.
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

int main()
{
    const char *need_mesh = "--mesh-depth-maps, --mesh-depth-normals and --mesh-cull-back need --mesh";
    const char *need_dir = "--mesh-depth-normals and --mesh-cull-back need --mesh-depth-maps";
    { // not given: no stage
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && p.a.mesh_depth_dir.empty() && !p.a.mesh_depth_normals &&
              !p.a.mesh_cull_back);
    }
    { // accepted, alone and with the other mesh stages, in any order
        const Parsed a = parse({"--mesh", "m.ply", "--mesh-depth-maps", "d"});
        CHECK(a.outcome == Parse::Run && a.a.mesh_depth_dir == "d" && !a.a.mesh_depth_normals && !a.a.mesh_cull_back);
        const Parsed b = parse({"--mesh-cull-back", "--mesh-depth-normals", "--mesh-depth-maps", "out/maps", "--mesh", "m.ply"});
        CHECK(b.outcome == Parse::Run && b.a.mesh_depth_dir == "out/maps" && b.a.mesh_depth_normals && b.a.mesh_cull_back);
        const Parsed c = parse({"--mesh", "m.ply", "--mesh-smooth", "3", "--mesh-decimate", "2", "--mesh-normals",
                                "--mesh-depth-maps", "d", "--mesh-cull-back", "--depth-maps", "e"});
        CHECK(c.outcome == Parse::Run && c.a.mesh_depth_dir == "d" && c.a.depth_dir == "e" && c.a.mesh_cull_back &&
              !c.a.mesh_depth_normals && !c.a.depth_normals && c.a.mesh_normals);
    }
    { // a missing value: the usage text is the message
        const Parsed p = parse({"--mesh", "m.ply", "--mesh-depth-maps"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
    }
    { // the missing --mesh
        const std::vector<std::vector<const char *>> alone = {{"--mesh-depth-maps", "d"},
                                                              {"--mesh-depth-normals"},
                                                              {"--mesh-cull-back"},
                                                              {"--mesh-depth-maps", "d", "--mesh-depth-normals"},
                                                              {"--depth-maps", "e", "--mesh-cull-back"}};
        for (const std::vector<const char *> &w : alone) {
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_mesh);
        }
    }
    { // the flags without the directory; --depth-maps is another option
        const std::vector<std::vector<const char *>> flags = {{"--mesh-depth-normals"},
                                                              {"--mesh-cull-back"},
                                                              {"--mesh-cull-back", "--mesh-depth-normals"},
                                                              {"--depth-maps", "e", "--mesh-depth-normals"}};
        for (std::vector<const char *> w : flags) {
            w.insert(w.begin(), {"--mesh", "m.ply"});
            const Parsed p = parse(w);
            CHECK(p.outcome == Parse::UsageError && p.error == need_dir);
        }
    }
    if (g_bad)
        return 1;
    std::printf("ok: mesh render options\n");
    return 0;
}
