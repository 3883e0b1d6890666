"""The mesh clean-up without a GPU: the numpy reference (tests/mesh_ref.py)
against a plain breadth-first search on the hand mesh and the deep strip, the
selection rules on the reference, Engine's argument validation, the CLI's three
options through a stand-alone program under ASan + UBSan, and the volume
property the GPU test relies on, on the CPU references alone."""
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest

import densepoints_amd as dp

import mesh_ref as MR
import tsdf_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bfs_components(tris, nv):
    """(vertex_component, triangle_component, rows of (root, vertices, triangles)) by a plain search"""
    valid = [all(0 <= int(i) < nv for i in t) for t in tris]
    adj = [set() for _ in range(nv)]
    used = [False] * nv
    for t, ok in zip(tris, valid):
        if ok:
            for i in t:
                used[int(i)] = True
                adj[int(i)].update(int(j) for j in t)
    vc, rows = [-1] * nv, []
    for v in range(nv):  # ascending: the first vertex met of a set is its smallest
        if not used[v] or vc[v] >= 0:
            continue
        vc[v] = len(rows)
        queue, size = deque([v]), 0
        while queue:
            u = queue.popleft()
            size += 1
            for w in adj[u]:
                if vc[w] < 0:
                    vc[w] = len(rows)
                    queue.append(w)
        rows.append([v, size, 0])
    tc = [vc[int(t[0])] if ok else -1 for t, ok in zip(tris, valid)]
    for c in tc:
        if c >= 0:
            rows[c][2] += 1
    return vc, tc, rows


def check_against_bfs(tris, nv):
    got = MR.components(tris, nv)
    vc, tc, rows = bfs_components(tris, nv)
    assert got["vertex_component"].tolist() == vc and got["triangle_component"].tolist() == tc
    table = got["components"]
    assert [[int(r["root"]), int(r["vertices"]), int(r["triangles"])] for r in table] == rows
    T = [r[2] for r in rows]
    want_rank = [sum(1 for d in range(len(T)) if T[d] > T[c] or (T[d] == T[c] and d < c)) for c in range(len(T))]
    assert table["rank"].tolist() == want_rank
    return got


def test_hand_mesh_against_bfs():
    tris, nv = MR.hand_mesh()
    got = check_against_bfs(tris, nv)
    # the premises of the hand mesh, on the reference
    assert got["stats"]["invalid_triangles"] == 5 and got["stats"]["unused_vertices"] == 3
    assert got["vertex_component"][[0, 6, 15]].tolist() == [-1, -1, -1]
    table = got["components"]
    assert table["root"].tolist() == [1, 4, 10, 14] and table["triangles"].tolist() == [2, 2, 2, 1]
    assert table["vertices"].tolist() == [3, 5, 4, 1] and table["rank"].tolist() == [0, 1, 2, 3]
    assert got["triangle_component"][2] == 1 and tris[2, 0] == 9  # (9, 4, 7): the root is not its first index
    assert got["vertex_component"][3] != got["vertex_component"][4]  # the invalid (3, 4, -1) joined nothing


def test_deep_mesh_against_bfs():
    tris, nv = MR.deep_mesh(strip=400, singles=150, seed=5)
    got = check_against_bfs(tris, nv)
    assert got["stats"]["components"] == 151 and got["stats"]["largest_triangles"] == 400


def test_empty_inputs():
    for tris, nv in ((np.zeros((0, 3), np.int32), 5), (np.array([[0, 1, 2]], np.int32), 0), (np.zeros((0, 3), np.int32), 0)):
        got = MR.components(tris, nv)
        assert got["stats"]["components"] == 0 and got["stats"]["largest_triangles"] == 0
        assert (got["vertex_component"] == -1).all() and (got["triangle_component"] == -1).all()
        out = MR.clean(MR.random_vertices(nv, 1), tris)
        assert len(out["vertices"]) == 0 and out["triangles"].shape == (0, 3)


def test_selection_rules_and_idempotence():
    # components of 8, 4, 4, 1 triangles: fans around their first vertex
    sizes, tris, base = (8, 4, 4, 1), [], 0
    for n in sizes:
        tris += [(base, base + 1 + i, base + 2 + i) for i in range(n)]
        base += n + 2
    tris = np.array(tris, np.int32)
    verts = MR.random_vertices(base, 2)
    assert MR.components(tris, base)["components"]["triangles"].tolist() == list(sizes)

    def kept(**kw):
        return MR.clean(verts, tris, **kw)["kept"].tolist()

    assert kept() == [True] * 4 and kept(min_triangles=0) == [True] * 4
    assert kept(min_fraction=0.5) == [True, True, True, False]  # 4 >= 0.5 * 8: the comparison is >=
    assert kept(max_components=2) == [True, True, False, False]  # the tie goes to the lower number
    assert kept(max_components=3, min_triangles=5) == [True, False, False, False]
    assert kept(min_triangles=9) == [False] * 4
    for kw in (dict(min_fraction=0.5), dict(max_components=2), dict(min_triangles=2)):
        once = MR.clean(verts, tris, **kw)
        again = MR.clean(once["vertices"], once["triangles"], **kw)
        assert again["vertices"].tobytes() == once["vertices"].tobytes()
        assert again["triangles"].tobytes() == once["triangles"].tobytes()
        assert (again["vertex_map"] == np.arange(len(once["vertices"]))).all()


def test_check_mesh_clean_args():
    o = dp.check_mesh_clean_args()
    assert (o.min_triangles, o.min_fraction, o.max_components, o.flags, o.reserved) == (1, 0.0, 0, 0, 0)
    o = dp.check_mesh_clean_args(7, 0.25, 3)
    assert (o.min_triangles, o.min_fraction, o.max_components) == (7, 0.25, 3)
    assert dp.check_mesh_clean_args(0, 1, np.int32(2)).max_components == 2
    for bad in (dict(min_triangles=-1), dict(min_triangles=1.5), dict(min_triangles=True), dict(min_triangles=None),
                dict(min_fraction=-0.01), dict(min_fraction=1.01), dict(min_fraction=float("nan")),
                dict(min_fraction="0.5"), dict(max_components=-1), dict(max_components=2**31), dict(max_components=0.5)):
        with pytest.raises(ValueError):
            dp.check_mesh_clean_args(**bad)


def test_cli_options_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cli_mesh_clean_args_check")
    cli = os.path.join(ROOT, "programs", "densify")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", cli,
                    os.path.join(ROOT, "tests", "cli_mesh_clean_args_check.cpp"), os.path.join(cli, "cli_args.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def test_blob_volume_cleans_to_the_sphere():
    """the property test_gpu_mesh_clean checks on the device, on the references:
    the sphere with six planted blobs, meshed, then cleaned with max_components =
    1, is the mesh of the sphere alone, byte for byte"""
    sphere, planted, weight = MR.blob_volumes()
    vol = {k: MR.BLOB_VOLUME[k] for k in ("origin", "voxel", "dim")}
    want = TR.mesh(sphere, weight, None, **vol)
    full = TR.mesh(planted, weight, None, **vol)
    assert (len(want["vertices"]), len(want["triangles"])) == MR.SPHERE_COUNTS
    lab = MR.components(full["triangles"], len(full["vertices"]))
    assert tuple(sorted(lab["components"]["triangles"].tolist(), reverse=True)) == MR.BLOB_TRIANGLES
    assert lab["stats"]["invalid_triangles"] == 0 and lab["stats"]["unused_vertices"] == 0
    out = MR.clean(full["vertices"].astype(MR.VERTEX_DTYPE), full["triangles"], max_components=1)
    assert out["vertices"].tobytes() == want["vertices"].astype(MR.VERTEX_DTYPE).tobytes()
    assert out["triangles"].tobytes() == want["triangles"].tobytes()
    # the equal sizes are tie cases: the cut inside a tie keeps the lower numbers
    for k in (2, 4):
        kept = MR.clean(full["vertices"].astype(MR.VERTEX_DTYPE), full["triangles"], max_components=k)["kept"]
        T = lab["components"]["triangles"]
        order = sorted(range(len(T)), key=lambda c: (-int(T[c]), c))[:k]
        assert sorted(np.flatnonzero(kept).tolist()) == sorted(order)
