"""csrc/dp_buf.h on the host: tests/buf_check.cpp, a stand-alone program with
counting stand-ins for the HIP calls the owning types make, built by the host
compiler under ASan + UBSan and run as its own process.  It checks the growth
policy (DevBuf: 1024 elements below 1024, else n + n/4; HostBuf: k + k/4; neither
shrinks), that a failed allocation leaves a buffer empty, that a moved-from
object frees nothing, and that allocations minus frees is zero once a struct of
buffers and events, and a vector of events, go out of scope."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for cand in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("hip/hip_runtime_api.h not found")


def test_owning_buffers_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "buf_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(),
                    "-I", os.path.join(ROOT, "densepoints_amd", "csrc"), os.path.join(ROOT, "tests", "buf_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
