"""densify --evaluate truth.xyz --eval-tau T --eval-normals on the tiny synthetic
scene the other CLI tests use, with --fuse: the "normals" members of the report
equal cloud_compare(..., normals=...) run here on the PLYs the run wrote, whose
normals carry every digit with --eval-normals."""
import json

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import _native as N

from test_gpu_cloud_nearest_cli import scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def read_ply_records(path):
    """the vertices of an ASCII cloud PLY (x y z r g b nx ny nz) as FUSED_DTYPE records"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    nv = int([h for h in lines[:end] if h.startswith("element vertex")][0].split()[-1])
    rows = np.array([ln.split() for ln in lines[end + 1:end + 1 + nv]], dtype=np.float64).reshape(nv, 9)
    rec = np.zeros(nv, N.FUSED_DTYPE)
    rec["pos"] = rows[:, :3].astype(np.float32)
    rec["normal"] = rows[:, 6:].astype(np.float32)
    return rec


def close(got, want):
    """n exactly; the angles to 1e-9 degrees: both sides run the same IEEE
    operations in the same order but for acos (two libm results differ by a few
    ulp of a value that is at most 90) and the order of the mean's sum"""
    assert got["n"] == want["n"] > 0
    for name in ("mean_deg", "median_deg", "p90_deg"):
        assert abs(got[name] - want[name]) <= 1e-9, (name, got[name], want[name])


@pytest.mark.parametrize("align", [False, True], ids=["as_written", "eval_align"])
def test_report_normals_equal_cloud_compare_on_the_written_plys(scene, tmp_path, align):
    from test_cli import run

    TAU = scene["tau"]
    pts, fused = str(tmp_path / "points.ply"), str(tmp_path / "fused.ply")
    extra = ("--eval-align", "--eval-align-iterations", "5") if align else ()
    report = json.loads(run(*scene["base"], "-o", pts, "--fuse", fused, "--evaluate", scene["truth_path"], "--eval-tau",
                            "%.17g" % TAU, "--eval-normals", "--eval-normals-k", "12", *extra).stdout)
    ev = report["evaluate"]
    assert sorted(ev) == ["fused", "patches"]
    with dp.Engine(device=0) as eng:
        for name, path in (("patches", pts), ("fused", fused)):
            cloud = read_ply_records(path)
            if align:
                # the CLI moves copies of every cloud, normals included, by the reported transform
                M = np.float64(report["align"]["matrix"]).reshape(3, 4)
                assert report["align"]["iterations"] == 5 and not np.array_equal(M, np.eye(3, 4))
                cloud = eng.cloud_transform(cloud, M, normals=True)
            want = dp.cloud_compare(eng, cloud, scene["truth"], TAU, normals=dict(k=12))
            close(ev[name]["normals"], want["normals"])
            assert want["normals"]["n"] <= want["accuracy"]["within_tau"]
            assert 0 <= want["normals"]["median_deg"] <= want["normals"]["p90_deg"] <= 90


def test_defaults_refusals_and_nothing_changes_without_the_flag(scene, tmp_path):
    from test_cli import run

    TAU = "%.17g" % scene["tau"]
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    plain = json.loads(run(*scene["base"], "-o", a, "--evaluate", scene["truth_path"], "--eval-tau", TAU).stdout)
    report = json.loads(run(*scene["base"], "-o", b, "--evaluate", scene["truth_path"], "--eval-tau", TAU,
                            "--eval-normals").stdout)
    assert "normals" not in plain["evaluate"]["patches"] and "normals" in report["evaluate"]["patches"]
    rest = {k: v for k, v in report["evaluate"]["patches"].items() if k != "normals"}
    assert rest == plain["evaluate"]["patches"]
    with dp.Engine(device=0) as eng:  # k = 16 and the evaluation's radius
        want = dp.cloud_compare(eng, read_ply_records(b), scene["truth"], scene["tau"], normals={})
    close(report["evaluate"]["patches"]["normals"], want["normals"])
    sj = scene["base"][1]
    r = run("-i", sj, "--eval-normals", check=False)
    assert r.returncode == 2 and "--eval-normals needs --evaluate" in r.stderr
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--eval-tau", TAU, "--eval-normals-k", "8", check=False)
    assert r.returncode == 2 and "need --eval-normals" in r.stderr
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--eval-tau", TAU, "--eval-normals", "--eval-normals-k", "2",
            check=False)
    assert r.returncode == 2 and "--eval-normals-k expects 3..32" in r.stderr
