"""densify --fuse fused.ply --fuse-clean-k K --fuse-clean-radius R [...] on the
tiny synthetic scene the other CLI tests use: the cleaned PLY holds exactly the
records Engine.cloud_clean keeps of the un-cleaned one, the report names the
counts, and without the flags nothing changes."""
import json

import numpy as np
import pytest

import densepoints_amd as dp

from test_gpu_cloud_nearest_cli import read_ply_positions, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def ply_rows(path):
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    nv = int([h for h in lines[:end] if h.startswith("element vertex")][0].split()[-1])
    return lines[:end + 1], lines[end + 1:end + 1 + nv]


@pytest.fixture(scope="module")
def plain(scene, tmp_path_factory):  # noqa: F811
    """the un-cleaned run, with --evaluate so that the PLY carries every digit of
    the positions; its fused cloud's spacing sets the radius"""
    from test_cli import run

    d = tmp_path_factory.mktemp("plain")
    pts, fused = str(d / "points.ply"), str(d / "fused.ply")
    ev = ("--evaluate", scene["truth_path"], "--eval-tau", "%.17g" % scene["tau"])
    report = json.loads(run(*scene["base"], "-o", pts, "--fuse", fused, *ev).stdout)
    pos = read_ply_positions(fused)
    assert len(pos) == report["fused"]["points"] > 500 and "fused_clean" not in report
    with dp.Engine(device=0) as eng:
        near = eng.cloud_knn(pos, pos, 1, 1e3, exclude_self=True)
    radius = float(np.float32(4 * np.median(near["dist"][:, 0])))
    return dict(pts=pts, fused=fused, ev=ev, pos=pos, radius=radius, report=report)


@pytest.mark.parametrize("mode", ["statistical", "radius_only"])
def test_cleaned_ply_is_what_cloud_clean_keeps(scene, plain, tmp_path, mode):  # noqa: F811
    from test_cli import run

    pts, fused = str(tmp_path / "points.ply"), str(tmp_path / "fused.ply")
    flags = ["--fuse-clean-k", "8", "--fuse-clean-radius", "%.17g" % plain["radius"]]
    kw = dict(k=8, max_dist=plain["radius"])
    if mode == "statistical":
        flags += ["--fuse-clean-std", "0.5", "--fuse-clean-min-neighbours", "2"]
        kw.update(std_mul=0.5, min_neighbours=2)
    else:
        flags += ["--fuse-clean-radius-only", "--fuse-clean-min-neighbours", "8"]
        kw.update(min_neighbours=8, radius_only=True)
    report = json.loads(run(*scene["base"], "-o", pts, "--fuse", fused, *plain["ev"], *flags).stdout)
    with dp.Engine(device=0) as eng:
        want = eng.cloud_clean(plain["pos"], **kw)
    st = want["stats"]
    assert 0 < st["kept"] < len(plain["pos"])  # the filter does something on this cloud
    head, rows = ply_rows(fused)
    head0, rows0 = ply_rows(plain["fused"])
    assert rows == [r for r, keep in zip(rows0, want["keep"]) if keep]
    assert [h for h in head if not h.startswith("element vertex")] == \
        [h for h in head0 if not h.startswith("element vertex")]
    fc = report["fused_clean"]
    assert (fc["points"], fc["kept"], fc["removed_sparse"], fc["removed_far"]) == \
        (len(plain["pos"]), st["kept"], st["removed_sparse"], st["removed_far"])
    assert fc["mu"] == pytest.approx(st["mu"], rel=1e-8) and fc["sigma"] == pytest.approx(st["sigma"], rel=1e-8)
    assert report["fused"]["points"] == st["kept"]
    # --evaluate reads the cleaned cloud, and the patches are not touched
    assert report["evaluate"]["fused"]["accuracy"]["n"] == st["kept"]
    assert open(pts, "rb").read() == open(plain["pts"], "rb").read()
    assert report["evaluate"]["patches"] == plain["report"]["evaluate"]["patches"]


def test_without_the_flags_nothing_changes(scene, plain, tmp_path):  # noqa: F811
    from test_cli import run

    # two runs without the clean flags (and without --evaluate: the short positions) are the same bytes
    out = []
    for name in ("a", "b"):
        pts, fused = str(tmp_path / (name + "_points.ply")), str(tmp_path / (name + "_fused.ply"))
        report = json.loads(run(*scene["base"], "-o", pts, "--fuse", fused).stdout)
        assert "fused_clean" not in report and report["fused"]["points"] == plain["report"]["fused"]["points"]
        out.append((open(pts, "rb").read(), open(fused, "rb").read()))
    assert out[0] == out[1]
    # and with --evaluate the un-cleaned cloud is the one `plain` wrote
    pts, fused = str(tmp_path / "c_points.ply"), str(tmp_path / "c_fused.ply")
    run(*scene["base"], "-o", pts, "--fuse", fused, *plain["ev"])
    assert open(fused, "rb").read() == open(plain["fused"], "rb").read()
    # the flags without --fuse, or K without R, are usage errors
    for bad in (["--fuse-clean-k", "8", "--fuse-clean-radius", "0.1"], ["--fuse", fused, "--fuse-clean-k", "8"]):
        r = run(*scene["base"], "-o", pts, *bad, check=False)
        assert r.returncode != 0 and "--fuse-clean" in r.stderr
