"""densify --mesh with --mesh-depth-maps [--mesh-depth-normals] [--mesh-cull-back],
and PMVS.mesh_depth_maps, on the tiny synthetic scene the other mesh CLI tests
use: the PFM files equal Engine.mesh_render of the written mesh, the report
carries the statistics, and the PLY keeps its bytes with and without the option."""
import json
import os

import pytest

import densepoints_amd as dp
from densepoints_amd import synth

import meshrender_ref as MR

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


@pytest.mark.parametrize("cull", [False, True], ids=["all", "cull_back"])
def test_cli_mesh_depth_maps(scene, tmp_path, cull):
    from test_cli import run

    out, maps = str(tmp_path / "mesh.ply"), tmp_path / "maps"
    flags = ("--mesh-depth-maps", str(maps), "--mesh-depth-normals") + (("--mesh-cull-back",) if cull else ())
    report = json.loads(run(*scene["base"], "--mesh", out, *flags).stdout)
    # the mesh is the one written without the option, and PMVS.mesh's
    pm = scene["pm"]
    pv, pt = pm.mesh(dim=40)
    ref = str(tmp_path / "python.ply")
    dp.write_mesh_ply(ref, pv, pt)
    with open(out, "rb") as a, open(scene["plain"], "rb") as b, open(ref, "rb") as c:
        ply = a.read()
        assert ply == b.read() == c.read()
    assert "mesh_render" not in scene["report"] and len(pt) > 0
    want = pm.mesh_depth_maps(pv, pt, normals=True, cull_back=cull)
    assert sorted(os.listdir(maps)) == sorted(["mesh_depth_%04d.pfm" % v for v in range(4)] +
                                              ["mesh_normal_%04d.pfm" % v for v in range(4)])
    for v in range(4):
        assert MR.same_bits(dp.read_pfm(str(maps / ("mesh_depth_%04d.pfm" % v))), want["depth"][v])
        assert MR.same_bits(dp.read_pfm(str(maps / ("mesh_normal_%04d.pfm" % v))), want["normal"][v])
    mr = report["mesh_render"]
    assert {c: mr[c] for c in MR.COUNTS} == {c: want["stats"][c] for c in MR.COUNTS}
    assert pm.stats["mesh_render"] == want["stats"]
    assert mr["views"] == 4 and mr["cull_back"] is cull and mr["render_ms"] > 0
    assert mr["covered_pixels"] > 0 and mr["triangles"] == len(pt) and (mr["culled_pairs"] > 0) == cull
    # and the reference agrees on the written mesh
    cams = MR.Cameras([v.P for v in pm.views], [160] * 4, [120] * 4)
    ref_out = MR.render(cams, pv, pt, views=[1], cull_back=cull)
    assert MR.same_bits(ref_out["depth"][0], want["depth"][1]) and MR.same_bits(ref_out["normal"][0], want["normal"][1])


def test_only_depth_and_refusals(scene, tmp_path):
    from test_cli import run

    out, maps = str(tmp_path / "mesh.ply"), tmp_path / "maps"
    run(*scene["base"], "--mesh", out, "--mesh-depth-maps", str(maps))
    assert sorted(os.listdir(maps)) == ["mesh_depth_%04d.pfm" % v for v in range(4)]
    sj = os.path.join(scene["dir"], "scene.json")
    r = run("-i", sj, "--mesh-depth-maps", str(maps), check=False)
    assert r.returncode == 2 and "need --mesh" in r.stderr
    for flag in ("--mesh-depth-normals", "--mesh-cull-back"):
        r = run("-i", sj, "--mesh", out, flag, check=False)
        assert r.returncode == 2 and "need --mesh-depth-maps" in r.stderr
    with pytest.raises(ValueError):
        dp.PMVS().mesh_depth_maps([], [])
