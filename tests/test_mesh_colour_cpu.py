"""The CPU reference of dp_mesh_colour (tests/meshcolour_ref.py) against what the
header promises, without a GPU: the planted verdicts the GPU test relies on, the
statistics' identities, a constant image, the sphere's visibility, the Python
argument checks and the ctypes binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from densepoints_amd import _native as N
from densepoints_amd import pmvs

import meshcolour_ref as CR
import meshrender_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = dict(depth_tol=0.25, min_cos=0.0)


@pytest.fixture(scope="module")
def planted():
    s = CR.planted()
    s["plain"] = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], **PLANTED)
    s["weighted"] = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], normals=s["normals"], **PLANTED)
    return s


def bits(out, s, label):
    return int(out["seen"][s["names"][label]])


def test_planted_verdicts_without_normals(planted):
    s, out = planted, planted["plain"]
    # <= against <, one-sided, in view 0 (bit 0) and the mirrored view (bit 2)
    assert bits(out, s, "tol_edge") == 0b101
    assert bits(out, s, "tol_over") == 0
    assert bits(out, s, "behind_surface") == 0b101
    # half-even: both land on the even pixel that holds a depth
    assert bits(out, s, "half_even_down") == 1 and bits(out, s, "half_even_up") == 1
    i, j = s["names"]["half_even_down"], s["names"]["half_even_up"]
    assert list(out["vertices"]["rgb"][i]) == list(s["images"][0][10, 20, ::-1])
    assert list(out["vertices"]["rgb"][j]) == list(s["images"][0][10, 22, ::-1])
    for label in ("outside", "behind_camera", "empty_pixel", "nan", "inf"):
        assert bits(out, s, label) == 0 and out["best"][s["names"][label]] == -1
        assert list(out["vertices"]["rgb"][s["names"][label]]) == [9, 8, 7]
    # without normals every weight is 1: the first view is the best
    assert bits(out, s, "right_angle") == 0b101 and out["best"][s["names"]["right_angle"]] == 0
    assert bits(out, s, "two_views") == 0b011
    assert list(out["vertices"]["rgb"][s["names"]["two_views"]]) == [2, 2, 2]
    assert bits(out, s, "corner_8x8") == 0b0010 and bits(out, s, "wide_last_column") == 0b1000
    st = out["stats"]
    assert st["vertices"] == len(s["vertices"]) - 2  # nan and inf take no part
    assert st["projected_pairs"] == st["occluded_pairs"] + st["grazing_pairs"] + st["visible_pairs"]
    assert st["vertices"] == st["coloured_vertices"] + st["unseen_vertices"]
    assert st["occluded_pairs"] == 2 and st["grazing_pairs"] == 0
    assert st["visible_pairs"] == sum(bin(int(m)).count("1") for m in out["seen"])


def test_planted_verdicts_with_normals(planted):
    s, out = planted, planted["weighted"]
    assert bits(out, s, "right_angle") == 0 and bits(out, s, "facing_away") == 0  # c == 0 and c < 0, at min_cos = 0
    assert bits(out, s, "zero_normal") == 0b101 and bits(out, s, "two_views") == 0b011
    assert list(out["vertices"]["rgb"][s["names"]["two_views"]]) == [2, 2, 2]
    assert out["stats"]["grazing_pairs"] == 4  # two vertices, views 0 and 2
    # a steeper min_cos drops the oblique vertices that min_cos = 0 kept
    steep = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], normals=s["normals"], depth_tol=0.25,
                      min_cos=0.9)
    assert bits(steep, s, "tol_edge") == 0 and bits(out, s, "tol_edge") == 0b101
    assert steep["stats"]["grazing_pairs"] > out["stats"]["grazing_pairs"]


def test_clear_unseen_and_untouched_fields(planted):
    s = planted
    out = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], clear_unseen=True, **PLANTED)
    for label in ("outside", "behind_camera", "empty_pixel", "tol_over"):
        assert list(out["vertices"]["rgb"][s["names"][label]]) == [0, 0, 0]
    for label in ("nan", "inf"):  # copied byte for byte
        assert out["vertices"][s["names"][label]].tobytes() == s["vertices"][s["names"][label]].tobytes()
    assert CR.same_bits(out["vertices"]["pos"], s["vertices"]["pos"]) and (out["vertices"]["pad"] == 0).all()
    assert CR.same_bits(out["seen"], planted["plain"]["seen"])


def test_view_subset_numbers_bits_by_position(planted):
    s = planted
    out = CR.colour(s["P"], s["images"], s["vertices"], [s["depth"][2], s["depth"][0]], views=[2, 0], **PLANTED)
    assert bits(out, s, "tol_edge") == 0b11 and bits(out, s, "two_views") == 0b10
    assert out["best"][s["names"]["two_views"]] == 1 and out["views"] == [2, 0]


def test_last_of_64_sets_bit_63():
    s = CR.last_of_64()
    out = CR.colour(s["P"], s["images"], s["vertices"], s["depth"])
    assert int(out["seen"][0]) == 1 << 63 and out["best"][0] == 63
    assert list(out["vertices"]["rgb"][0]) == list(s["images"][63][4, 4, ::-1])


def test_constant_images_give_their_colour_nearest_and_bilinear():
    s = CR.planted()
    imgs = [np.full_like(im, 0) + np.array([30, 20, 10], np.uint8) for im in s["images"]]  # B, G, R
    for bilinear in (False, True):
        out = CR.colour(s["P"], imgs, s["vertices"], s["depth"], normals=s["normals"], bilinear=bilinear, **PLANTED)
        col = out["vertices"]["rgb"][out["seen"] != 0]
        assert len(col) > 5 and (col == [10, 20, 30]).all()


def test_bilinear_weights_the_four_taps():
    s = CR.planted()
    i = s["names"]["half_even_down"]  # u = 20.5, v = 10: the mean of columns 20 and 21 of row 10
    out = CR.colour(s["P"], s["images"], s["vertices"], s["depth"], bilinear=True, **PLANTED)
    a, b = s["images"][0][10, 20, ::-1].astype(np.float64), s["images"][0][10, 21, ::-1].astype(np.float64)
    assert list(out["vertices"]["rgb"][i]) == [int(np.rint(0.5 * x + 0.5 * y)) for x, y in zip(a, b)]
    # at the last column the tap beyond it is clamped: the texel itself
    j = s["names"]["wide_last_column"]
    assert list(out["vertices"]["rgb"][j]) == list(s["images"][3][3, 15, ::-1])


def test_sphere_far_side_is_unseen():
    verts, tris, centre, _ = MR.tsdf_sphere()
    P = MR.sphere_cameras(centre)
    W, H = [w for w, _ in MR.SPHERE_SIZES], [h for _, h in MR.SPHERE_SIZES]
    cams = MR.Cameras(P, W, H)
    depth = MR.render(cams, verts, tris, views=[0, 2])["depth"]
    imgs = [CR.hash_image(v, w, h) for v, (w, h) in enumerate(MR.SPHERE_SIZES)]
    out = CR.colour(P, imgs, verts, depth, views=[0, 2])
    st = out["stats"]
    assert st["vertices"] == len(verts) and st["occluded_pairs"] > len(verts) // 4
    for k, v in enumerate((0, 2)):
        towards = ((verts["pos"].astype(np.float64) - centre) @ (cams.centre(v) - centre)) > 0.1 * 0.3 * 1.1
        sees = (out["seen"] >> np.uint64(k)) & np.uint64(1) != 0
        # the cap a camera at distance D sees of a sphere of radius r holds (1 - r / D) / 2 = 0.36 of
        # it; the nearest-pixel test at depth_tol = 0.01 loses the slanted rim: a third of the cap is asked for
        assert sees.sum() > len(verts) * 0.12
        assert not (sees & ~towards).any()  # nothing on the far side is seen


def test_check_mesh_colour_args_refuses_every_listed_error():
    ok = pmvs.check_mesh_colour_args(3, 4, [2, 0], [1, 2], 0.5, 0.25, True, True)
    assert (ok[0].depth_tol, ok[0].min_cos, ok[0].flags) == (0.5, 0.25, 3) and ok[1].tolist() == [2, 0]
    assert ok[1].dtype == np.int32
    d = pmvs.check_mesh_colour_args(0, 2)
    assert abs(d[0].depth_tol - 0.01) < 1e-9 and abs(d[0].min_cos - 0.2) < 1e-8 and d[0].flags == 0
    bad = [
        dict(n_vertices=-1), dict(n_vertices=2**31), dict(n_vertices=1.5), dict(n_vertices=True),
        dict(views=[]), dict(views=[0, 0]), dict(views=[4]), dict(views=[-1]), dict(V=65, views=list(range(65))),
        dict(depth=[]), dict(depth=[1, None, 3, 4]), dict(depth=[1, 2, 0, 4]), dict(depth=[1, 2, 3]),
        dict(depth_tol=-0.5), dict(depth_tol=float("inf")), dict(depth_tol=float("nan")), dict(depth_tol=1e39),
        dict(depth_tol="1"), dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos=float("nan")), dict(min_cos=None),
        dict(bilinear=1), dict(clear_unseen=2), dict(bilinear=None),
        dict(inputs=(100, 200), outputs=(200,)), dict(depth=[1, 2, 3, 4], outputs=(50, 3)),
    ]
    for kw in bad:
        args = dict(dict(n_vertices=3, V=4, views=None), **kw)
        with pytest.raises(ValueError):
            pmvs.check_mesh_colour_args(**args)
    # legal neighbours of the refused values
    pmvs.check_mesh_colour_args(2**31 - 1, 64, None, None, 0.0, 0.0)
    pmvs.check_mesh_colour_args(0, 4, [3], [7], 1.0, 1.0, inputs=(100, 0, None), outputs=(300, 0, None))


def test_binding_matches_the_header():
    with open(os.path.join(ROOT, "include", "densepoints.h")) as f:
        text = f.read()
    m = re.search(r"typedef struct dp_mesh_colour_options \{(.*?)\} dp_mesh_colour_options;", text, re.S)
    names = re.findall(r"(?:float|int32_t)\s+(\w+);", m.group(1))
    assert names == [n for n, _ in N.DpMeshColourOptions._fields_]
    m = re.search(r"typedef struct dp_mesh_colour_stats \{(.*?)\} dp_mesh_colour_stats;", text, re.S)
    fields = [w for w in re.findall(r"\w+", m.group(1)) if w not in ("int64_t", "double")]
    assert fields == [n for n, _ in N.DpMeshColourStats._fields_] == list(CR.COUNTS) + ["colour_ms"]
    assert int(re.search(r"#define DP_MESH_COLOUR_BILINEAR (\d+)", text).group(1)) == N.DP_MESH_COLOUR_BILINEAR
    assert int(re.search(r"#define DP_MESH_COLOUR_CLEAR_UNSEEN (\d+)", text).group(1)) == N.DP_MESH_COLOUR_CLEAR_UNSEEN
    sigs = dict((s[0], s) for s in N.SIGNATURES)
    for name in ("dp_mesh_colour", "dp_mesh_colour_device"):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(sigs[name][2])
    assert ctypes.sizeof(N.DpMeshColourOptions) == 12
