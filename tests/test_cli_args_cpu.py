"""programs/densify/cli_args.cpp on the host: tests/cli_args_check.cpp, a
stand-alone program that feeds parse_args whole command lines, built by the
host compiler under ASan + UBSan (with stand-ins for the dp_default_* functions,
so without the library) and run as its own process.  It checks the defaults,
every option once, a missing value, an unknown flag, each ranged option at its
limits and just outside, the words --exchange / --matcher / --detector / --mode
refuse, the leniency of the options read with atoi / atof, that --iterations > 1
turns --filter on, and that replicate_below defaults to 1024 x gpus."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_args_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cli_args_check")
    cli = os.path.join(ROOT, "programs", "densify")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", cli, os.path.join(ROOT, "tests", "cli_args_check.cpp"),
                    os.path.join(cli, "cli_args.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
