"""densify --mesh with --mesh-colour [--mesh-colour-bilinear] [--mesh-colour-tol T]
[--mesh-colour-min-cos C] on the tiny synthetic scene the other mesh CLI tests
use: the PLY keeps its positions and faces, its colours equal Engine.mesh_colour
on that mesh, and the report carries the statistics."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import synth

import meshcolour_ref as CR

pytestmark = pytest.mark.gpu


def read_ply(path):
    """(x y z, red green blue, faces) of an ASCII mesh PLY as the CLI writes it"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    head = lines[:end]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    props = [h.split()[-1] for h in head[:[i for i, h in enumerate(head) if h.startswith("element face")][0]]
             if h.startswith("property")]
    rows = [ln.split() for ln in lines[end + 1:end + 1 + nv]]
    col = {p: [r[i] for r in rows] for i, p in enumerate(props)}
    pos = [(col["x"][i], col["y"][i], col["z"][i]) for i in range(nv)]
    rgb = np.array([[int(col[c][i]) for c in ("red", "green", "blue")] for i in range(nv)], np.uint8).reshape(-1, 3)
    faces = lines[end + 1 + nv:end + 1 + nv + nf]
    return pos, rgb, faces, props


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the scene on disk, its plain mesh by the CLI, and an engine with its views"""
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
    verts, tris = pm.mesh(dim=40)
    return dict(dir=d, base=base, plain=plain, report=report, pm=pm, verts=verts, tris=tris)


@pytest.mark.parametrize("detail", [False, True], ids=["defaults", "bilinear_tol_cos"])
def test_cli_mesh_colour(scene, tmp_path, detail):
    from test_cli import run

    out = str(tmp_path / "mesh.ply")
    flags = ("--mesh-colour",) + (("--mesh-colour-bilinear", "--mesh-colour-tol", "0.05", "--mesh-colour-min-cos",
                                   "0.5") if detail else ())
    report = json.loads(run(*scene["base"], "--mesh", out, *flags).stdout)
    pos, rgb, faces, props = read_ply(out)
    pos0, rgb0, faces0, props0 = read_ply(scene["plain"])
    # the geometry is the plain run's, which is PMVS.mesh's; no normals are written
    assert pos == pos0 and faces == faces0 and props == props0 and len(faces) == len(scene["tris"]) > 0
    assert "mesh_colour" not in scene["report"] and (rgb0 == scene["verts"]["rgb"]).all()
    kw = dict(bilinear=True, depth_tol=0.05, min_cos=0.5) if detail else {}
    with dp.Engine(device=0) as eng:
        eng.set_views(scene["pm"].views)
        nrm, _ = eng.mesh_normals(scene["verts"], scene["tris"])
        want = eng.mesh_colour(scene["verts"], triangles=scene["tris"], normals=nrm, **kw)
    assert CR.same_bits(rgb, want["vertices"]["rgb"]) and not CR.same_bits(rgb, rgb0)
    mc = report["mesh_colour"]
    assert {c: mc[c] for c in CR.COUNTS} == {c: want["stats"][c] for c in CR.COUNTS}
    assert mc["views"] == 4 and mc["bilinear"] is detail and mc["colour_ms"] > 0
    assert abs(mc["depth_tol"] - (0.05 if detail else 0.01)) < 1e-6 and abs(mc["min_cos"] - (0.5 if detail else 0.2)) < 1e-6
    assert mc["coloured_vertices"] > len(pos) // 2


def test_shared_planes_written_normals_and_refusals(scene, tmp_path):
    from test_cli import run

    out, maps = str(tmp_path / "mesh.ply"), tmp_path / "maps"
    both = str(tmp_path / "both.ply")
    report = json.loads(run(*scene["base"], "--mesh", both, "--mesh-colour", "--mesh-depth-maps", str(maps),
                            "--mesh-normals").stdout)
    run(*scene["base"], "--mesh", out, "--mesh-colour")
    # the planes rendered once serve both; the normals are written only with --mesh-normals
    assert sorted(os.listdir(maps)) == ["mesh_depth_%04d.pfm" % v for v in range(4)]
    pos, rgb, faces, props = read_ply(both)
    pos1, rgb1, faces1, props1 = read_ply(out)
    assert "nx" in props and "nx" not in props1 and pos == pos1 and faces == faces1 and CR.same_bits(rgb, rgb1)
    assert "mesh_render" in report and "mesh_colour" in report
    sj = os.path.join(scene["dir"], "scene.json")
    r = run("-i", sj, "--mesh-colour", check=False)
    assert r.returncode == 2 and "need --mesh" in r.stderr
    r = run("-i", sj, "--mesh", out, "--mesh-colour-bilinear", check=False)
    assert r.returncode == 2 and "need --mesh-colour" in r.stderr
