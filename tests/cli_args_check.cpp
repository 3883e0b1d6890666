// programs/densify/cli_args.cpp on the host: parse_args fed whole command
// lines, with stand-ins for the three dp_default_* functions it calls (no
// library, no device) that fill recognisable values.  Built with the host
// compiler under ASan + UBSan and run by tests/test_cli_args_cpu.py.
#include "cli_args.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

extern "C" void dp_default_matcher_options(dp_matcher_options *m)
{
    std::memset(m, 0, sizeof *m);
    m->n_features = 111;
    m->fast_threshold = 22;
    m->matcher_type = DP_MATCHER_KNN;
    m->detector_type = DP_DETECTOR_ORB;
    m->akaze_threshold = 0.5f;
}
extern "C" void dp_default_fast_options(dp_fast_options *f)
{
    std::memset(f, 0, sizeof *f);
    f->iters = 44;
    f->gradient = 55;
    f->densify = 7; // parse_args owns this one: 0 unless --mode fast
}
extern "C" void dp_default_fuse_options(dp_fuse_options *f)
{
    std::memset(f, 0, sizeof *f);
    f->depth_tol = 0.25f;
    f->min_views = 6;
}

static int g_bad = 0;
#define CHECK(x) ((x) ? (void)0 : (void)(++g_bad, std::printf("FAIL line %d: %s\n", __LINE__, #x)))

struct Parsed {
    Parse outcome;
    Args a;
    std::string error;
};

static Parsed parse(std::initializer_list<const char *> words)
{
    std::vector<std::string> store{"densify"};
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

// the outcome of `-i x <option> <value>`
static Parse with(const char *option, const char *value) { return parse({"-i", "x", option, value}).outcome; }

// a usage error that carries its own message (the usage text is not printed)
static bool refuses(const char *option, const char *value, const char *message)
{
    const Parsed p = parse({"-i", "x", option, value});
    return p.outcome == Parse::UsageError && p.error == message;
}

int main()
{
    { // the defaults: the library's for its structs, with fast.densify cleared
        const Parsed p = parse({"-i", "scene.json"});
        const Args &a = p.a;
        CHECK(p.outcome == Parse::Run && p.error.empty());
        CHECK(a.input == "scene.json" && a.settings.empty() && a.output == "points.ply" && a.seeds_path.empty());
        CHECK(a.synth.empty() && a.scene_dir.empty() && a.depth_dir.empty() && a.fuse_path.empty());
        CHECK(a.device == 0 && a.gpus == 1 && !a.force_multi && a.exchange_mode == "auto");
        CHECK(a.replicate_below == 1024 && a.max_pops == -1 && a.level == 0);
        CHECK(!a.check_only && !a.do_filter && a.iterations == 1 && a.splat_scale == 1.0 && !a.depth_normals);
        CHECK(a.matcher.n_features == 111 && a.matcher.fast_threshold == 22 && a.matcher.epipolar_matching == 0);
        CHECK(a.matcher.matcher_type == DP_MATCHER_KNN && a.matcher.detector_type == DP_DETECTOR_ORB);
        CHECK(a.matcher.akaze_threshold == 0.5f);
        CHECK(a.fast.densify == 0 && a.fast.iters == 44 && a.fast.gradient == 55);
        CHECK(a.fuse.depth_tol == 0.25f && a.fuse.min_views == 6);
    }
    { // every option once
        const Parsed p = parse({"--input", "in.json", "--settings", "s.json", "--output", "o.ply", "--seeds", "s.xyz",
                                "--device", "3", "--gpus", "4", "--multi", "--replicate-below", "77", "--exchange", "copy",
                                "--max-pops", "123456789012", "--level", "2", "--filter", "--iterations", "16",
                                "--check-only", "--features", "2000", "--fast-threshold", "8", "--epipolar-matching",
                                "--matcher", "flann", "--detector", "akaze", "--akaze-threshold", "0.0002", "--mode",
                                "fast", "--fast-iters", "9", "--fast-gradient", "1", "--synthetic", "4,160,120,1",
                                "--write-scene", "dir", "--depth-maps", "maps", "--splat-scale", "1.5", "--depth-normals",
                                "--fuse", "f.ply", "--fuse-min-views", "63", "--fuse-depth-tol", "0.02"});
        const Args &a = p.a;
        CHECK(p.outcome == Parse::Run && p.error.empty());
        CHECK(a.input == "in.json" && a.settings == "s.json" && a.output == "o.ply" && a.seeds_path == "s.xyz");
        CHECK(a.device == 3 && a.gpus == 4 && a.force_multi && a.replicate_below == 77 && a.exchange_mode == "copy");
        CHECK(a.max_pops == 123456789012ll && a.level == 2 && a.do_filter && a.iterations == 16 && a.check_only);
        CHECK(a.matcher.n_features == 2000 && a.matcher.fast_threshold == 8 && a.matcher.epipolar_matching == 1);
        CHECK(a.matcher.matcher_type == DP_MATCHER_FLANN && a.matcher.detector_type == DP_DETECTOR_AKAZE);
        CHECK(a.matcher.akaze_threshold == 0.0002f);
        CHECK(a.fast.densify == 1 && a.fast.iters == 9 && a.fast.gradient == 1);
        CHECK(a.synth == "4,160,120,1" && a.scene_dir == "dir" && a.depth_dir == "maps" && a.fuse_path == "f.ply");
        CHECK(a.splat_scale == 1.5 && a.depth_normals && a.fuse.min_views == 63 && a.fuse.depth_tol == 0.02f);
        const Parsed q = parse({"-i", "a", "-s", "b", "-o", "c", "--matcher", "knn", "--detector", "orb", "--mode",
                                "parity", "--exchange", "rccl"});
        CHECK(q.outcome == Parse::Run && q.a.input == "a" && q.a.settings == "b" && q.a.output == "c");
        CHECK(q.a.matcher.matcher_type == DP_MATCHER_KNN && q.a.matcher.detector_type == DP_DETECTOR_ORB);
        CHECK(q.a.fast.densify == 0 && q.a.exchange_mode == "rccl");
        CHECK(with("--exchange", "auto") == Parse::Run);
    }
    { // help; the usage errors whose message is the usage text
        CHECK(parse({"-h"}).outcome == Parse::Help && parse({"-i", "x", "--help"}).outcome == Parse::Help);
        for (const Parsed &p : {parse({}), parse({"--filter"}), parse({"-i", "x", "--level"}), parse({"-i"}),
                                parse({"-i", "x", "--no-such-flag"}), parse({"-i", "x", "--no-such-flag", "1"}),
                                parse({"-i", "x", "--mode", "turbo"})})
            CHECK(p.outcome == Parse::UsageError && p.error.empty());
        // a scene to write needs no input (that --write-scene came with it is main's to check)
        CHECK(parse({"--synthetic", "2,32,24,0"}).outcome == Parse::Run);
    }
    { // the ranged options at their limits and just outside
        CHECK(refuses("--iterations", "0", "--iterations expects 1..16"));
        CHECK(refuses("--iterations", "17", "--iterations expects 1..16"));
        CHECK(refuses("--iterations", "x", "--iterations expects 1..16")); // atoi: 0
        CHECK(with("--iterations", "1") == Parse::Run && with("--iterations", "16") == Parse::Run);
        for (const char *v : {"-1", "64", "x", "", "7x"})
            CHECK(refuses("--fuse-min-views", v, "--fuse-min-views expects 0..63"));
        CHECK(parse({"-i", "x", "--fuse-min-views", "0"}).a.fuse.min_views == 0);
        CHECK(with("--fuse-min-views", "0") == Parse::Run && with("--fuse-min-views", "63") == Parse::Run);
        for (const char *v : {"-1", "x", "1e39", "", "nan", "inf", "0.5x"})
            CHECK(refuses("--fuse-depth-tol", v, "--fuse-depth-tol expects a finite number >= 0"));
        CHECK(with("--fuse-depth-tol", "0") == Parse::Run && parse({"-i", "x", "--fuse-depth-tol", "0"}).a.fuse.depth_tol == 0.0f);
        CHECK(with("--fuse-depth-tol", "3e38") == Parse::Run);
        CHECK(refuses("--splat-scale", "0", "--splat-scale expects a positive number"));
        CHECK(refuses("--splat-scale", "-2", "--splat-scale expects a positive number"));
        CHECK(refuses("--splat-scale", "x", "--splat-scale expects a positive number")); // atof: 0
        CHECK(refuses("--exchange", "mpi", "--exchange expects auto, rccl or copy"));
        CHECK(refuses("--matcher", "lsh", "--matcher expects knn or flann"));
        CHECK(refuses("--detector", "sift", "--detector expects orb or akaze"));
    }
    { // the options read with atoi / atof take a leading number, else 0
        const Parsed p = parse({"-i", "x", "--iterations", "2x", "--device", "1z", "--features", "q", "--splat-scale",
                                "2.5m", "--akaze-threshold", "z"});
        CHECK(p.outcome == Parse::Run && p.a.iterations == 2 && p.a.device == 1 && p.a.matcher.n_features == 0);
        CHECK(p.a.splat_scale == 2.5 && p.a.matcher.akaze_threshold == 0.0f);
        // a negative --fast-iters / --fast-gradient leaves the library's default
        const Parsed q = parse({"-i", "x", "--fast-iters", "-1", "--fast-gradient", "-3"});
        CHECK(q.outcome == Parse::Run && q.a.fast.iters == 44 && q.a.fast.gradient == 55);
    }
    { // --iterations > 1 implies --filter; replicate_below defaults to 1024 x gpus
        CHECK(parse({"-i", "x", "--iterations", "2"}).a.do_filter && !parse({"-i", "x", "--iterations", "1"}).a.do_filter);
        CHECK(parse({"-i", "x", "--gpus", "3"}).a.replicate_below == 3072);
        CHECK(parse({"-i", "x", "--gpus", "3", "--replicate-below", "0"}).a.replicate_below == 0);
        CHECK(parse({"-i", "x", "--replicate-below", "5", "--gpus", "2"}).a.replicate_below == 5);
    }
    if (g_bad)
        return 1;
    std::printf("ok: parse_args\n");
    return 0;
}
