"""densify --mesh with --mesh-decimate [--mesh-decimate-quadric], and PMVS.mesh
with decimate=, on the tiny synthetic scene test_gpu_mesh_smooth_cli.py uses: the
written PLY is PMVS.mesh's mesh of the same scene, the report carries the
statistics, the mesh has fewer triangles than without the option, and without it
the PLY keeps its bytes."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import synth

import meshdecimate_ref as DR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the scene on disk, its plain mesh by the CLI, and the same scene run through PMVS"""
    from test_cli import run

    d = str(tmp_path_factory.mktemp("scene"))
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o",
            os.path.join(d, "points.ply"), "--mesh-dim", "40")
    plain = os.path.join(d, "plain.ply")
    report = json.loads(run(*base, "--mesh", plain).stdout)
    cfg = synth.config(4, 160, 120, 1)
    P = synth.cameras(cfg)
    pm = dp.PMVS()
    for v in range(4):
        pm.add_camera(dp.View(P[v], synth.render_host(cfg, P, v)))
    assert pm.run(synth.seeds(cfg, P))
    return dict(dir=d, base=base, plain=plain, report=report, pm=pm)


@pytest.mark.parametrize("quadric", [False, True], ids=["mean", "quadric"])
def test_cli_mesh_decimate(scene, tmp_path, quadric):
    from test_cli import run
    from test_tsdf_cpu import parse_ply

    out = str(tmp_path / "decimated.ply")
    flags = ("--mesh-decimate", "2") + (("--mesh-decimate-quadric",) if quadric else ())
    report = json.loads(run(*scene["base"], "--mesh", out, *flags).stdout)
    v0, f0 = parse_ply(scene["plain"])
    v1, f1 = parse_ply(out)
    assert "mesh_decimate" not in scene["report"] and 0 < len(f1) < len(f0) and 0 < len(v1) < len(v0)
    # PMVS.mesh of the same scene
    pm = scene["pm"]
    pv, pt = pm.mesh(dim=40)
    assert len(pv) == len(v0) and np.array_equal(pt, f0[:, 1:])
    dv, dt = pm.mesh(dim=40, decimate=dict(factor=2, quadric=quadric))
    ref = str(tmp_path / "python.ply")
    dp.write_mesh_ply(ref, dv, dt)
    with open(out, "rb") as a, open(ref, "rb") as b:
        assert a.read() == b.read()
    st = pm.stats["mesh"]["decimate"]
    md = report["mesh_decimate"]
    assert {k: md[k] for k in DR.COUNTS} == {k: st[k] for k in DR.COUNTS}
    assert md["quadric"] is quadric and md["vertices_out"] == len(v1) == report["mesh"]["vertices"]
    assert md["triangles_out"] == len(f1) == report["mesh"]["triangles"] and md["triangles_in"] == len(f0)
    assert (md["quadric_vertices"] > 0) == quadric
    vol = pm.stats["mesh"]
    # the report prints the float32 cell with nine digits, which round-trip
    assert np.float32(md["cell"]) == np.float32(2.0 * float(np.float32(vol["voxel"])))
    # the reference on PMVS.mesh's plain mesh
    want = DR.decimate(pv, pt, md["cell"], vol["origin"], quadric)
    assert dv.tobytes() == want["vertices"].tobytes() and dt.tobytes() == want["triangles"].tobytes()
    assert np.array_equal(np.unique(dt), np.arange(len(dv)))  # no unused vertex


def test_pipeline_order_and_unchanged_paths(scene, tmp_path):
    """clean -> smooth -> decimate -> normals, outward normals, and the paths without the option"""
    from test_cli import run

    pm = scene["pm"]
    pv, pt = pm.mesh(dim=40)
    sv, st_, sn = pm.mesh(dim=40, smooth=dict(iterations=2), normals=True)
    assert "decimate" not in pm.stats["mesh"]
    dv, dt, dn = pm.mesh(dim=40, smooth=dict(iterations=2), decimate=dict(factor=2), normals=True)
    vol = pm.stats["mesh"]
    want = DR.decimate(sv, st_, float(np.float32(2.0 * float(np.float32(vol["voxel"])))), vol["origin"], False)
    assert dv.tobytes() == want["vertices"].tobytes() and dt.tobytes() == want["triangles"].tobytes()
    assert len(dn) == len(dv) and 0 < len(dt) < len(pt)
    with dp.Engine(device=0) as eng:
        nrm, _ = eng.mesh_normals(dv, dt)
    assert dn.tobytes() == nrm.tobytes()
    # the winding survived: a vertex's normal and its cluster's point to the same
    # side.  A flipped winding would turn every product negative, a kept one leaves
    # all but the noisy vertices positive: the majority tells the two apart
    vm = want["vertex_map"]
    ok = vm >= 0
    dots = np.einsum("ij,ij->i", sn[ok].astype(np.float64), dn[vm[ok]].astype(np.float64))
    assert (dots > 0).mean() > 0.5
    # without the option: the same bytes as before
    again = str(tmp_path / "again.ply")
    run(*scene["base"], "--mesh", again)
    with open(again, "rb") as a, open(scene["plain"], "rb") as b:
        assert a.read() == b.read()
    for bad in (dict(), dict(cell=1.0, factor=2.0), dict(factor=-1), dict(cell=0.0)):
        with pytest.raises(ValueError):
            pm.mesh(dim=40, decimate=bad)
    r = run("-i", os.path.join(scene["dir"], "scene.json"), "--mesh-decimate", "2", check=False)
    assert r.returncode == 2 and "need --mesh" in r.stderr
    r = run("-i", os.path.join(scene["dir"], "scene.json"), "--mesh", again, "--mesh-decimate", "0", check=False)
    assert r.returncode == 2 and "expects" in r.stderr
