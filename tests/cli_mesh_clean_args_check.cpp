// The densify CLI's mesh clean-up options on the host: parse_args of
// programs/densify/cli_args.cpp fed whole command lines, with stand-ins for the
// three dp_default_* functions it calls (no library, no device).  Built with the
// host compiler under ASan + UBSan and run by tests/test_mesh_clean_cpu.py.
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

static Parsed parse(std::initializer_list<const char *> words)
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

static bool refuses(const char *option, const char *value, const char *message)
{
    const Parsed p = parse({option, value});
    return p.outcome == Parse::UsageError && p.error == message;
}

int main()
{
    { // none of the three given: no clean-up
        const Parsed p = parse({"--mesh", "m.ply"});
        CHECK(p.outcome == Parse::Run && p.error.empty() && p.a.mesh_path == "m.ply" && !p.a.mesh_clean());
        CHECK(p.a.mesh_min_component < 0 && p.a.mesh_min_component_frac < 0.0 && p.a.mesh_keep_largest < 0);
    }
    { // each alone turns it on and leaves the other two to the library
        const Parsed n = parse({"--mesh-min-component", "0"});
        CHECK(n.outcome == Parse::Run && n.a.mesh_clean() && n.a.mesh_min_component == 0);
        CHECK(n.a.mesh_min_component_frac < 0.0 && n.a.mesh_keep_largest < 0);
        const Parsed f = parse({"--mesh-min-component-frac", "0"});
        CHECK(f.outcome == Parse::Run && f.a.mesh_clean() && f.a.mesh_min_component_frac == 0.0);
        CHECK(f.a.mesh_min_component < 0 && f.a.mesh_keep_largest < 0);
        const Parsed k = parse({"--mesh-keep-largest", "1"});
        CHECK(k.outcome == Parse::Run && k.a.mesh_clean() && k.a.mesh_keep_largest == 1);
        const Parsed all = parse({"--mesh-min-component", "2147483647", "--mesh-min-component-frac", "1",
                                  "--mesh-keep-largest", "2147483647"});
        CHECK(all.outcome == Parse::Run && all.a.mesh_min_component == 2147483647LL);
        CHECK(all.a.mesh_min_component_frac == 1.0 && all.a.mesh_keep_largest == 2147483647LL);
        CHECK(parse({"--mesh-min-component-frac", "0.25"}).a.mesh_min_component_frac == 0.25);
    }
    { // the limits, just outside them, and values that are no numbers
        for (const char *v : {"-1", "2147483648", "x", "", "7x", "1.5"})
            CHECK(refuses("--mesh-min-component", v, "--mesh-min-component expects 0..2147483647"));
        for (const char *v : {"-0.1", "1.0001", "nan", "inf", "x", "", "0.5x"})
            CHECK(refuses("--mesh-min-component-frac", v, "--mesh-min-component-frac expects a number in 0..1"));
        for (const char *v : {"0", "-1", "2147483648", "x", "", "2k"})
            CHECK(refuses("--mesh-keep-largest", v, "--mesh-keep-largest expects 1..2147483647"));
        // a missing value: the usage text is the message
        const Parsed p = parse({"--mesh-keep-largest"});
        CHECK(p.outcome == Parse::UsageError && p.error.empty());
    }
    if (g_bad)
        return 1;
    std::printf("ok: mesh clean-up options\n");
    return 0;
}
