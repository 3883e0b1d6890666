"""The CPU reference of dp_mesh_render (tests/meshrender_ref.py) against what the
header promises, without a GPU: analytic depths, coverage of a closed surface,
the facing rule, culling, the planted edge cases the GPU test relies on, the
Python argument checks and the ctypes binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs

import meshrender_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted():
    P, W, H = MR.planted_cameras()
    verts, tris, names = MR.planted_mesh()
    cams = MR.Cameras(P, W, H)
    return dict(verts=verts, tris=tris, names=names, cams=cams,
                out={c: MR.render(cams, verts, tris, cull_back=c) for c in (False, True)})


@pytest.fixture(scope="module")
def sphere():
    verts, tris, centre, voxel = MR.tsdf_sphere()
    P = MR.sphere_cameras(centre)
    cams = MR.Cameras(P, [s[0] for s in MR.SPHERE_SIZES], [s[1] for s in MR.SPHERE_SIZES])
    return dict(verts=verts, tris=tris, centre=centre, voxel=voxel, cams=cams,
                out={c: MR.render(cams, verts, tris, cull_back=c) for c in (False, True)})


def rays(cams, v):
    """camera centre and the direction of every pixel's ray, scaled so that a
    point C + z d has depth row_2 = z"""
    P = np.array(cams.P[v])
    C = cams.centre(v)
    ys, xs = np.mgrid[0:cams.H[v], 0:cams.W[v]]
    px = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64)
    return C, px @ np.linalg.inv(P[:, :3]).T


def test_quad_depth_is_the_ray_plane_depth():
    verts, tris, p0, n = MR.quad()
    P, W, H = MR.planted_cameras()
    cams = MR.Cameras(P, W, H)
    out = MR.render(cams, verts, tris)
    for k in range(cams.V):
        C, d = rays(cams, k)
        with np.errstate(divide="ignore"):
            z = ((p0 - C) @ n) / (d @ n)
        hit = out["depth"][k] > 0
        assert hit.sum() > 200
        assert (np.abs(out["depth"][k][hit] - z[hit]) <= 1e-5 * z[hit]).all()
        # both triangles win pixels, and the pixels between them are covered: every
        # row of the quad's interior is one run
        assert set(np.unique(out["index"][k][hit])) == {0, 1}
        for row in hit:
            xs = np.nonzero(row)[0]
            assert len(xs) == 0 or len(xs) == xs[-1] - xs[0] + 1
        assert MR.same_bits(out["normal"][k][hit], np.broadcast_to(n.astype(np.float32), (hit.sum(), 3)))


def test_sphere_is_covered_where_its_rays_hit(sphere):
    cams, out = sphere["cams"], sphere["out"][False]
    r = 0.3 - sphere["voxel"]
    for k in range(cams.V):
        C, d = rays(cams, k)
        oc = C - sphere["centre"]
        b = d @ oc
        disc = b * b - (d * d).sum(-1) * (oc @ oc - r * r)
        inside = disc > 0
        assert inside.sum() > cams.W[k] * cams.H[k] // 8
        assert (out["depth"][k][inside] > 0).all()
    assert out["stats"]["triangles"] == len(sphere["tris"]) and out["stats"]["clipped_pairs"] == 0


def test_front_facing_is_the_geometric_rule(sphere, planted):
    for case in (sphere, planted):
        pos = case["verts"]["pos"].astype(np.float64)
        for pr in case["out"][False]["pairs"]:
            X = pos[case["tris"][pr["triangle"]]]
            C = case["cams"].centre(pr["view"])
            s = np.cross(X[1] - X[0], X[2] - X[0]) @ (C - X[0])
            assert abs(s) > 1e-9 and pr["front"] == (s > 0)
    # the mirrored camera's determinant is negative: there the sign of D alone is wrong
    mirrored = [pr for pr in planted["out"][False]["pairs"] if pr["view"] == 2]
    assert MR.view_det(planted["cams"].P[2]) < 0 and any(pr["front"] and pr["D"] > 0 for pr in mirrored)


def test_culling_keeps_a_closed_meshes_depth(sphere):
    a, b = sphere["out"][False], sphere["out"][True]
    assert all(MR.same_bits(x, y) for x, y in zip(a["depth"], b["depth"]))
    assert all(MR.same_bits(x, y) for x, y in zip(a["index"], b["index"]))
    assert b["stats"]["culled_pairs"] == a["stats"]["pairs"] - b["stats"]["pairs"] > b["stats"]["pairs"] // 2


def test_planted_cases(planted):
    names, out, cull = planted["names"], planted["out"][False], planted["out"][True]
    idx, depth = out["index"][0], out["depth"][0]
    tri_pairs = lambda label, o=out: [p for p in o["pairs"] if p["triangle"] in names[label]]  # noqa: E731
    # the shared diagonal and its end vertices go to the lower index, once
    q0, q1 = names["quad"]
    assert all(idx[k, k] == q0 for k in range(8, 25))
    assert idx[8, 24] == q1 and idx[24, 8] == q0 and idx[8, 8] == q0 and idx[24, 24] == q0
    # the quad is exactly its 17 x 17 pixels at depth 2, edges included, and no
    # pixel next to it is covered
    assert np.isin(idx[8:25, 8:25], (q0, q1)).all() and (depth[8:25, 8:25] == 2.0).all()
    assert (idx[7, 7:27] == -1).all() and (idx[25, 7:27] == -1).all() and (idx[7:27, 7] == -1).all()
    assert (idx[7:27, 25] == -1).all()
    # coincident: the lower index everywhere, both counted; 99 = the lattice points of
    # the closed triangle (Pick: area 84, 28 on the boundary, 71 inside)
    c0, c1 = names["coincident"]
    assert (idx == c0).sum() == 99 and (idx == c1).sum() == 0 and len(tri_pairs("coincident")) == 6
    # D == 0: no pair; behind: clipped when a vertex is in front, else nothing
    assert not tri_pairs("edge_on") and not tri_pairs("one_behind") and not tri_pairs("on_plane")
    assert not tri_pairs("all_behind")
    assert out["stats"]["clipped_pairs"] == 2 * 3
    # back-facing: drawn without culling, culled with it
    b = names["back"][0]
    assert (idx == b).sum() > 0 and (cull["index"][0] == b).sum() == 0
    assert all(not p["front"] for p in tri_pairs("back")) and len(tri_pairs("back")) == 3
    assert cull["stats"]["culled_pairs"] == 3 and cull["stats"]["pairs"] == out["stats"]["pairs"] - 3
    # outside: an empty box in every view; partly outside: a clipped box
    assert not tri_pairs("outside")
    assert any(p["x0"] == 0 and p["y1"] == 63 for p in tri_pairs("partly_outside"))
    # a box narrower than a wave
    assert any((p["x1"] - p["x0"] + 1) * (p["y1"] - p["y0"] + 1) == 9 for p in tri_pairs("tiny"))
    # invalid and NaN triangles: counted, never drawn
    assert out["stats"]["invalid_triangles"] == 4
    assert out["stats"]["triangles"] == len(planted["tris"]) - 4 - 1
    assert not tri_pairs("nan") and not tri_pairs("invalid")


def test_full_view_triangle_and_box_widths(planted):
    fv, ft = MR.full_view_triangle()
    out = MR.render(planted["cams"], fv, ft)
    assert all((d == 8.0).all() for d in out["depth"])
    assert [(p["x0"], p["x1"], p["y0"], p["y1"]) for p in out["pairs"]] == [(0, 95, 0, 63), (0, 66, 0, 44), (0, 95, 0, 63)]
    # wider than a wave's 64 lanes and larger than one band
    assert out["stats"]["pixel_tests"] == 2 * 96 * 64 + 67 * 45


def test_check_mesh_render_args():
    mro, vid = pmvs.check_mesh_render_args(10, 20, 4, None, True)
    assert mro.flags == N.DP_MESH_RENDER_CULL_BACK and vid.dtype == np.int32 and vid.tolist() == [0, 1, 2, 3]
    assert pmvs.check_mesh_render_args(0, 0, 4, [3, 1])[1].tolist() == [3, 1]
    assert pmvs.check_mesh_render_args(0, 0, 4)[0].flags == 0
    for bad in (dict(n_vertices=-1), dict(n_triangles=-1), dict(n_vertices=2**31), dict(n_triangles=2**31),
                dict(n_vertices=1.5), dict(n_triangles=True), dict(views=[]), dict(views=[0, 0]), dict(views=[4]),
                dict(views=[-1]), dict(views=[0, 1, 2, 3, 0]), dict(cull_back=1), dict(cull_back=None), dict(V=0)):
        kw = dict(dict(n_vertices=3, n_triangles=1, V=4, views=None, cull_back=False), **bad)
        with pytest.raises(ValueError):
            pmvs.check_mesh_render_args(**kw)


def test_header_declares_and_ctypes_binds():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    bound = {name: args for name, _, args in N.SIGNATURES}
    for sym, n_args in (("dp_default_mesh_render_options", 1), ("dp_mesh_render", 12), ("dp_mesh_render_device", 13)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, text)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args == len(bound[sym]), sym
        assert hasattr(N.lib, sym)
    assert "#define DP_MESH_RENDER_CULL_BACK 1" in text and N.DP_MESH_RENDER_CULL_BACK == MR.CULL_BACK == 1
    assert "#define DP_ABI_VERSION 2" in text
    assert ctypes.sizeof(N.DpMeshRenderOptions) == 4 and ctypes.sizeof(N.DpMeshRenderStats) == 64
    assert [n for n, _ in N.DpMeshRenderStats._fields_] == list(MR.COUNTS) + ["render_ms"]
    o = N.DpMeshRenderOptions(7)
    N.lib.dp_default_mesh_render_options(ctypes.byref(o))
    assert o.flags == 0
