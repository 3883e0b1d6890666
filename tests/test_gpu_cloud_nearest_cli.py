"""densify --evaluate truth.xyz --eval-tau T [--eval-max-dist D] on the tiny
synthetic scene the other CLI tests use, with --fuse and --mesh: the report's
"evaluate" entries equal cloud_compare run here on the PLYs the run wrote."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import synth

import cloudnearest_ref as CR

pytestmark = pytest.mark.gpu


def read_ply_positions(path):
    """the x y z of an ASCII PLY's vertices as float32"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    nv = int([h for h in lines[:end] if h.startswith("element vertex")][0].split()[-1])
    rows = [ln.split()[:3] for ln in lines[end + 1:end + 1 + nv]]
    return np.array(rows, dtype=np.float64).astype(np.float32).reshape(-1, 3)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the scene on disk and a truth cloud: the height field sampled on a coarse
    grid over the seeds' extent, written with every digit of its float32"""
    from test_cli import run

    d = str(tmp_path_factory.mktemp("scene"))
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    cfg = synth.config(4, 160, 120, 1)
    seeds = synth.seeds(cfg, synth.cameras(cfg))
    lo, hi = seeds[:, :2].min(axis=0), seeds[:, :2].max(axis=0)
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 96), np.linspace(lo[1], hi[1], 72), indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
    z, _ = synth.surface(cfg, xy)
    truth = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    path = os.path.join(d, "truth.xyz")
    with open(path, "w") as f:
        f.write("# ground truth\n")
        for p in truth:
            f.write("%.9g %.9g %.9g\n" % tuple(float(c) for c in p))
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"))
    # the threshold: two grid pitches, so a point on the surface has a sample within it
    tau = float(np.float32(2 * max((hi[0] - lo[0]) / 95, (hi[1] - lo[1]) / 71)))
    return dict(dir=d, base=base, truth=truth, truth_path=path, tau=tau)


def entry(e):
    """a report entry with its nulls as NaN"""
    return {k: ({f: float("nan") if x is None else x for f, x in v.items()} if isinstance(v, dict) else v)
            for k, v in e.items()}


@pytest.mark.parametrize("radius", [None, 3.0], ids=["ten_tau", "three_tau"])
def test_report_equals_cloud_compare_on_the_written_plys(scene, tmp_path, radius):
    from test_cli import run

    TAU = scene["tau"]
    max_dist = None if radius is None else float(np.float32(radius * TAU))
    pts, fused, mesh = (str(tmp_path / n) for n in ("points.ply", "fused.ply", "mesh.ply"))
    extra = () if max_dist is None else ("--eval-max-dist", "%.17g" % max_dist)
    report = json.loads(run(*scene["base"], "-o", pts, "--fuse", fused, "--mesh", mesh, "--mesh-dim", "40",
                            "--evaluate", scene["truth_path"], "--eval-tau", "%.17g" % TAU, *extra).stdout)
    ev = report["evaluate"]
    assert sorted(ev) == ["fused", "mesh_vertices", "patches"]
    with dp.Engine(device=0) as eng:
        for name, path in (("patches", pts), ("fused", fused), ("mesh_vertices", mesh)):
            cloud = read_ply_positions(path)
            want = dp.cloud_compare(eng, cloud, scene["truth"], TAU, max_dist)
            CR.assert_compare(entry(ev[name]), want)
            # not vacuous: the cloud is there, some of it lies on the surface and covers some of it
            acc, com = want["accuracy"], want["completeness"]
            assert acc["n"] == len(cloud) > 0 and com["n"] == len(scene["truth"]), name
            assert 0 < acc["within_tau"] <= acc["matched"] and 0 < com["within_tau"] < com["n"], name
            assert 0 < want["fscore"] <= 1 and 0 < acc["median"] <= acc["p90"], name
    # the patch cloud against the brute-force reference too
    CR.assert_compare(entry(ev["patches"]), CR.compare(read_ply_positions(pts), scene["truth"], TAU, max_dist))


def test_entries_follow_the_stages_and_nothing_changes_without_evaluate(scene, tmp_path):
    from test_cli import run

    TAU = "%.17g" % scene["tau"]
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    plain = json.loads(run(*scene["base"], "-o", a).stdout)
    assert "evaluate" not in plain
    report = json.loads(run(*scene["base"], "-o", b, "--evaluate", scene["truth_path"], "--eval-tau", TAU).stdout)
    assert sorted(report["evaluate"]) == ["patches"]
    assert {k: v for k, v in report.items() if k not in ("evaluate", "output") and not k.endswith("_ms")} == \
        {k: v for k, v in plain.items() if k != "output" and not k.endswith("_ms")}
    # the same patches; with --evaluate their positions carry every digit
    pa, pb = read_ply_positions(a), read_ply_positions(b)
    assert pa.shape == pb.shape and np.allclose(pa, pb, rtol=1e-5, atol=1e-7)
    # --check-only reads the truth file and covers the refusals
    sj = scene["base"][1]
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--eval-tau", TAU, "--check-only")
    assert json.loads(r.stdout)["truth"] == len(scene["truth"])
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--check-only", check=False)
    assert r.returncode == 2 and "--evaluate needs --eval-tau" in r.stderr
    r = run("-i", sj, "--eval-tau", "0.5", check=False)
    assert r.returncode == 2 and "need --evaluate" in r.stderr
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--eval-tau", "0.5", "--eval-max-dist", "0.1", check=False)
    assert r.returncode == 2 and "at least --eval-tau" in r.stderr
    r = run("-i", sj, "--evaluate", os.path.join(scene["dir"], "missing.xyz"), "--eval-tau", "0.5", "--check-only",
            check=False)
    assert r.returncode != 0 and r.stdout == ""
