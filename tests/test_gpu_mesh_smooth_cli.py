"""densify --mesh with --mesh-smooth and --mesh-normals, and PMVS.mesh with
smooth= and normals=, on a tiny synthetic scene: the written vertices and
normals are the library's smoothing and normals of the mesh a run without the
flags writes (the calls PMVS.mesh makes after its clean-up), PMVS.mesh's are the
reference's, and without the flags the PLY keeps its bytes."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import MESH_VERTEX_DTYPE

import meshsmooth_ref as SR

pytestmark = pytest.mark.gpu


def parse_normals_ply(path):
    """(vertices n x 9 as float64, faces n x 4) of a mesh PLY with normals"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    props = [h.split()[1:] for h in lines[:end] if h.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"],
                     ["uchar", "blue"], ["float", "nx"], ["float", "ny"], ["float", "nz"],
                     ["list", "uchar", "int", "vertex_indices"]]
    nv = int([h for h in lines[:end] if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in lines[:end] if h.startswith("element face")][0].split()[2])
    body = lines[end + 1:]
    assert body[-1] == "" and len(body) == nv + nf + 1
    return (np.array([ln.split() for ln in body[:nv]], dtype=np.float64).reshape(nv, 9),
            np.array([ln.split() for ln in body[nv:nv + nf]], dtype=np.int64).reshape(nf, 4))


def test_cli_mesh_smooth_and_normals(tmp_path):
    from test_cli import run
    from test_tsdf_cpu import parse_ply

    d = str(tmp_path / "scene")
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    ply, plain, smooth, again = (tmp_path / n for n in ("points.ply", "plain.ply", "smooth.ply", "again.ply"))
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o", str(ply), "--mesh-dim",
            "40")
    r0 = json.loads(run(*base, "--mesh", str(plain)).stdout)
    v0, f0 = parse_ply(str(plain))
    assert len(v0) > 0 and "smooth" not in r0["mesh"] and "normals" not in r0["mesh"]
    r1 = json.loads(run(*base, "--mesh", str(smooth), "--mesh-smooth", "3", "--mesh-normals").stdout)
    v1, f1 = parse_normals_ply(str(smooth))
    assert np.array_equal(f1, f0) and r1["mesh"]["smooth"]["steps"] == 6
    # the library on the plain mesh: what PMVS.mesh(smooth=dict(iterations=3), normals=True) runs after the extraction
    verts = np.zeros(len(v0), MESH_VERTEX_DTYPE)
    verts["pos"], verts["rgb"] = v0[:, :3].astype(np.float32), v0[:, 3:6].astype(np.uint8)
    tris = f0[:, 1:].astype(np.int32)
    with dp.Engine(device=0) as eng:
        sv, sst = eng.mesh_smooth(verts, tris, iterations=3)
        nrm, nst = eng.mesh_normals(sv, tris)
    assert np.array_equal(v1[:, :3].astype(np.float32), sv["pos"]) and np.array_equal(v1[:, 3:6], v0[:, 3:6])
    assert np.array_equal(v1[:, 6:].astype(np.float32), nrm)
    assert not np.array_equal(sv["pos"], verts["pos"])
    for k in ("steps", "movable_vertices", "pinned_vertices", "edges", "boundary_edges", "max_valence"):
        assert r1["mesh"]["smooth"][k] == sst[k], k
    assert r1["mesh"]["normals"]["zero_normals"] == nst["zero_normals"]
    # without the flags: the same bytes as before
    run(*base, "--mesh", str(again))
    assert again.read_bytes() == plain.read_bytes()
    for bad in (("--mesh-smooth", "1001"), ("--mesh-smooth", "1", "--mesh-smooth-lambda", "0"),
                ("--mesh-smooth", "1", "--mesh-smooth-mu", "0.5")):
        r = run("-i", os.path.join(d, "scene.json"), "--mesh", str(smooth), *bad, check=False)
        assert r.returncode == 2 and "expects" in r.stderr
    r = run("-i", os.path.join(d, "scene.json"), "--mesh-normals", check=False)
    assert r.returncode == 2 and "need --mesh" in r.stderr


def test_pmvs_mesh_smooth_and_normals():
    """PMVS.mesh(smooth=..., normals=True) is the reference's smoothing and normals of PMVS.mesh()"""
    from test_gpu_parity import scene

    sc = scene("hf6")
    pm = dp.PMVS()
    for v in sc.views:
        pm.add_camera(v)
    assert pm.run(sc.seeds)
    verts, tris = pm.mesh(dim=24)
    assert "smooth" not in pm.stats["mesh"] and "normals" not in pm.stats["mesh"] and len(tris) > 0
    sv, st, nrm = pm.mesh(dim=24, smooth=dict(iterations=2, lam=0.4), normals=True)
    assert st.tobytes() == tris.tobytes()
    want = SR.smooth(verts, tris, iterations=2, lam=0.4)
    assert sv.tobytes() == want["vertices"].tobytes()
    assert {k: pm.stats["mesh"]["smooth"][k] for k in SR.SMOOTH_COUNTS} == want["stats"]
    wn = SR.normals(sv, tris)
    assert nrm.tobytes() == wn["normals"].tobytes()
    assert {k: pm.stats["mesh"]["normals"][k] for k in SR.NORMAL_COUNTS} == wn["stats"]
    with pytest.raises(ValueError):
        pm.mesh(dim=24, smooth=dict(lam=2.0))
