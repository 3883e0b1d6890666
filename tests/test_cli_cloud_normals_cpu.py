"""The densify CLI's --eval-normals options without a GPU:
tests/cli_cloud_normals_args_check.cpp, a stand-alone program around the one
parser (programs/densify/cli_args.cpp), built with the host compiler under ASan +
UBSan."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_options_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cli_cloud_normals_args_check")
    cli = os.path.join(ROOT, "programs", "densify")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", cli,
                    os.path.join(ROOT, "tests", "cli_cloud_normals_args_check.cpp"), os.path.join(cli, "cli_args.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def test_usage_names_the_options():
    with open(os.path.join(ROOT, "programs", "densify", "cli_args.cpp")) as f:
        text = f.read()
    for opt in ("--eval-normals [--eval-normals-k K]", "--eval-normals-radius R", "dp_cloud_normals"):
        assert opt in text, opt
