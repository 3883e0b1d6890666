"""densify --mesh ... --evaluate ... --eval-mesh-surface on the tiny synthetic
scene of the other evaluate CLI test: the report's "mesh_surface" equals
mesh_compare run here on the mesh PLY the run wrote, "decimate_deviation" is
there with --mesh-decimate, and nothing changes without the flag."""
import json
import math
import os

import numpy as np
import pytest

import densepoints_amd as dp

import cloudnearest_ref as CR
from test_gpu_cloud_nearest_cli import entry, scene  # noqa: F401  (scene is a fixture)
from test_tsdf_cpu import parse_ply

pytestmark = pytest.mark.gpu


def test_mesh_surface_and_decimate_deviation(scene, tmp_path):  # noqa: F811
    from test_cli import run

    TAU = scene["tau"]
    mesh = str(tmp_path / "mesh.ply")
    common = (*scene["base"], "-o", str(tmp_path / "points.ply"), "--mesh", mesh, "--mesh-dim", "40", "--mesh-decimate",
              "2", "--evaluate", scene["truth_path"], "--eval-tau", "%.17g" % TAU)
    plain = json.loads(run(*common).stdout)
    # without the flag the key set is what it was
    assert sorted(plain["evaluate"]) == ["mesh_vertices", "patches"]
    report = json.loads(run(*common, "--eval-mesh-surface").stdout)
    ev = report["evaluate"]
    assert sorted(ev) == ["decimate_deviation", "mesh_surface", "mesh_vertices", "patches"]
    assert ev["mesh_vertices"] == plain["evaluate"]["mesh_vertices"] and ev["patches"] == plain["evaluate"]["patches"]
    v, f = parse_ply(mesh)
    pos, tris = v[:, :3].astype(np.float32), f[:, 1:].astype(np.int32)
    with dp.Engine(device=0) as eng:
        want = dp.mesh_compare(eng, pos, tris, scene["truth"], TAU)
    CR.assert_compare(entry(ev["mesh_surface"]), want)
    com, acc = want["completeness"], want["accuracy"]
    assert com["n"] == len(scene["truth"]) and acc["n"] == len(pos) > 0 and 0 < want["fscore"] <= 1
    # the surface is never less complete than its vertices, and here it is more
    assert entry(ev["mesh_surface"])["accuracy"] == entry(ev["mesh_vertices"])["accuracy"]
    assert com["within_tau"] >= ev["mesh_vertices"]["completeness"]["within_tau"] > 0
    assert com["matched"] >= ev["mesh_vertices"]["completeness"]["matched"]
    dev = ev["decimate_deviation"]
    assert sorted(dev) == ["a_to_b", "b_to_a", "max"]
    for side in (dev["a_to_b"], dev["b_to_a"]):
        assert sorted(side) == ["matched", "max", "mean", "median", "n", "p90"]
        assert 0 < side["matched"] <= side["n"]
        assert all(math.isfinite(side[k]) for k in ("mean", "median", "p90", "max"))
        assert 0 <= side["median"] <= side["p90"] <= side["max"] <= dev["max"]
    assert dev["b_to_a"]["n"] == len(pos) and dev["a_to_b"]["n"] == report["mesh_decimate"]["vertices_in"]
    assert dev["max"] == max(dev["a_to_b"]["max"], dev["b_to_a"]["max"]) <= float(np.float32(10 * TAU))
    # without --mesh-decimate there is no deviation to report
    report = json.loads(run(*scene["base"], "-o", str(tmp_path / "p2.ply"), "--mesh", str(tmp_path / "m2.ply"),
                            "--mesh-dim", "40", "--evaluate", scene["truth_path"], "--eval-tau", "%.17g" % TAU,
                            "--eval-mesh-surface").stdout)
    assert sorted(report["evaluate"]) == ["mesh_surface", "mesh_vertices", "patches"]


def test_refusals(scene):  # noqa: F811
    from test_cli import run

    sj = scene["base"][1]
    need = "--eval-mesh-surface needs --evaluate and --mesh"
    r = run("-i", sj, "--eval-mesh-surface", "--check-only", check=False)
    assert r.returncode == 2 and need in r.stderr
    r = run("-i", sj, "--mesh", os.path.join(scene["dir"], "m.ply"), "--eval-mesh-surface", check=False)
    assert r.returncode == 2 and need in r.stderr
    r = run("-i", sj, "--evaluate", scene["truth_path"], "--eval-tau", "0.5", "--eval-mesh-surface", check=False)
    assert r.returncode == 2 and need in r.stderr
    r = run("-i", sj, "--mesh", os.path.join(scene["dir"], "m.ply"), "--evaluate", scene["truth_path"], "--eval-tau",
            "0.5", "--eval-mesh-surface", "--check-only")
    assert r.returncode == 0
