"""dp_render_maps on the GPU against the CPU reference (tests/render_ref.py,
restated from the header's spec): depth and index bit for bit, normal and score
the winners' gathers, the device-counted statistics equal to the reference's."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp

import render_ref as RR
from test_gpu_iterate import planted, to_device
from test_gpu_parity import SceneCase, scene
from test_render_cpu import WIDE_CASES, wide_patches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("patches", "pairs", "pixel_tests", "covered_pixels")


def cams_of(orc, sc, level=0):
    P, imgs = (sc.P, sc.imgs) if level == 0 else orc.level_scene(sc.P, sc.imgs, level)
    return RR.Cameras(orc, P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs])


def assert_equal(got, want, normals=True):
    assert got["views"] == want["views"]
    for k in range(len(want["views"])):
        assert RR.same_bits(got["index"][k], want["index"][k]), f"index, view {want['views'][k]}"
        assert RR.same_bits(got["depth"][k], want["depth"][k]), f"depth, view {want['views'][k]}"
        if normals:
            assert RR.same_bits(got["normal"][k], want["normal"][k])
            assert RR.same_bits(got["score"][k], want["score"][k])
    assert {c: got["stats"][c] for c in COUNTS} == want["stats"]


@pytest.fixture(scope="module")
def hf6(orc):
    """the planted hf6 store, its cameras, an engine with the views set, and the
    reference renders (computed once, never modified)"""
    ref = planted(orc, "parity", 1)
    sc = scene("hf6")
    cams = cams_of(orc, sc)
    want = {True: RR.render(cams, ref["pat"], keep=ref["keep"]), False: RR.render(cams, ref["pat"])}
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        yield dict(pat=ref["pat"], keep=ref["keep"], n_orig=ref["n_orig"], cams=cams, want=want, eng=eng, sc=sc)


def render_device(eng, pat, keep, views, sizes, **kw):
    """render_maps_device into torch tensors; the same dict as render_maps"""
    import torch

    dpat = to_device(pat)
    dkeep = to_device(keep) if keep is not None else None
    t = {"depth": [torch.full((h, w), 7.0, dtype=torch.float32, device="cuda") for w, h in sizes],
         "index": [torch.full((h, w), 7, dtype=torch.int32, device="cuda") for w, h in sizes],
         "normal": [torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda") for w, h in sizes],
         "score": [torch.full((h, w), 7.0, dtype=torch.float32, device="cuda") for w, h in sizes]}
    torch.cuda.synchronize()
    st = eng.render_maps_device(dpat.data_ptr(), len(pat), dkeep.data_ptr() if dkeep is not None else 0, views,
                                *[[x.data_ptr() for x in t[k]] for k in ("depth", "index", "normal", "score")], **kw)
    out = {k: [x.cpu().numpy() for x in v] for k, v in t.items()}
    out["views"], out["stats"] = [int(v) for v in views], st
    return out


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("with_keep", [True, False])
def test_hf6_equals_reference_bit_for_bit(hf6, with_keep, form):
    pat, keep, want = hf6["pat"], hf6["keep"] if with_keep else None, hf6["want"][with_keep]
    if form == "host":
        got = hf6["eng"].render_maps(pat, keep=keep, normals=True, scores=True)
    else:
        got = render_device(hf6["eng"], pat, keep, range(6), [(320, 240)] * 6)
    assert_equal(got, want)
    # not vacuous: an occlusion was resolved (some pixel's winner is not the
    # patch whose projected centre is nearest to it), a box was clipped at an
    # image edge, and the keep flags matter
    v = 0
    prs = [p for p in want["pairs"] if p["view"] == v]
    cu = np.array([p["cu"] for p in prs])
    cv = np.array([p["cv"] for p in prs])
    ids = np.array([p["index"] for p in prs])
    ys, xs = np.nonzero(want["index"][0] >= 0)
    nearest = ids[np.argmin((xs[:, None] - cu[None, :]) ** 2 + (ys[:, None] - cv[None, :]) ** 2, axis=1)]
    assert (nearest != want["index"][0][ys, xs]).any()
    assert any(p["clipped"] for p in want["pairs"])
    assert not RR.same_bits(hf6["want"][True]["index"][0], hf6["want"][False]["index"][0])
    # planted occluders (indices >= n_orig) win pixels when they are not filtered
    assert (hf6["want"][False]["index"][0] >= hf6["n_orig"]).any()


def test_repeat_and_subset_stability(hf6):
    eng, pat, want = hf6["eng"], hf6["pat"], hf6["want"][False]
    a = eng.render_maps(pat, normals=True, scores=True)
    b = eng.render_maps(pat, normals=True, scores=True)
    assert_equal(a, want)
    assert_equal(b, want)
    sub = eng.render_maps(pat, views=[4, 1], normals=True, scores=True)
    assert sub["views"] == [4, 1]
    for k, v in enumerate([4, 1]):
        for name in ("depth", "index", "normal", "score"):
            assert RR.same_bits(sub[name][k], a[name][v]), (name, v)
    ref = RR.render(hf6["cams"], pat, views=[4, 1])
    assert {c: sub["stats"][c] for c in COUNTS} == ref["stats"]
    # a smaller z-buffer after a larger one, then the full set again
    assert_equal(eng.render_maps(pat, normals=True, scores=True), want)


def test_all_facing_and_null_outputs(hf6):
    eng, pat = hf6["eng"], hf6["pat"][:300]
    want = RR.render(hf6["cams"], pat, all_facing=True)
    got = eng.render_maps(pat, all_facing=True, normals=True, scores=True)
    assert_equal(got, want)
    assert want["stats"]["pairs"] > RR.render(hf6["cams"], pat)["stats"]["pairs"]
    assert_equal(eng.render_maps(pat, all_facing=True), want, normals=False)
    # an empty patch set clears every plane
    none = eng.render_maps(pat[:0], normals=True, scores=True)
    assert all((d == 0).all() for d in none["depth"]) and all((i == -1).all() for i in none["index"])
    assert all((x == 0).all() for x in none["normal"]) and none["stats"]["covered_pixels"] == 0


def test_several_chunks_of_the_pair_list(hf6, monkeypatch):
    """DP_RENDER_PAIR_CAP bounds the pair list: the patches go through in
    chunks, each raster sized from its own device-held count"""
    monkeypatch.setenv("DP_RENDER_PAIR_CAP", "600")  # 100 patches per chunk with 6 views
    got = hf6["eng"].render_maps(hf6["pat"], normals=True, scores=True)
    assert_equal(got, hf6["want"][False])


def test_level_one(orc, hf6):
    sc, pat = hf6["sc"], hf6["pat"]
    want = RR.render(cams_of(orc, sc, 1), pat)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        eng.build_pyramid(2)
        eng.set_level(1)
        got = eng.render_maps(pat, normals=True, scores=True)
    assert all(d.shape == (120, 160) for d in got["depth"])
    assert_equal(got, want)
    assert want["stats"]["covered_pixels"] > 0


def test_boxes_smaller_than_a_wave(hf6):
    want = RR.render(hf6["cams"], hf6["pat"], splat_scale=0.25, max_radius_px=1)
    # B = 1: floor(c - 1) .. ceil(c + 1) is 3 or 4 pixels per side, far below a wave's 64
    assert all((p["x1"] - p["x0"] + 1) * (p["y1"] - p["y0"] + 1) <= 16 for p in want["pairs"])
    got = hf6["eng"].render_maps(hf6["pat"], splat_scale=0.25, max_radius_px=1, normals=True, scores=True)
    assert_equal(got, want)
    assert want["stats"]["covered_pixels"] > 0


def test_boxes_wider_than_a_wave(orc):
    """2 views of 64 x 48, three hand-made patches whose boxes exceed 64 pixels
    (test_render_cpu.py checks the premises): the lane loop takes several trips"""
    sc = SceneCase(V=2, W=64, H=48, kind=0)
    cams = cams_of(orc, sc)
    pat = wide_patches(sc.cfg)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        for kw in WIDE_CASES:
            want = RR.render(cams, pat, **kw)
            assert want["stats"]["pairs"] == 6
            assert all((p["x1"] - p["x0"] + 1) * (p["y1"] - p["y0"] + 1) > 64 for p in want["pairs"])
            assert_equal(eng.render_maps(pat, normals=True, scores=True, **kw), want)


def test_device_resident_densify_iterate_then_render(hf6):
    """densify_iterate -> densify_store_device -> filter flags -> render_maps_device
    never visits the host; it equals the host form on the copied-out survivors"""
    import torch

    sc = hf6["sc"]
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        surv, _ = eng.densify_iterate(sc.seeds, 2)
        d_store, n = eng.densify_store_device()
        assert n >= len(surv) > 0
        keep_t = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.filter_patches_device(d_store, n, keep_t.data_ptr(), 3)
        planes = {"depth": [torch.empty((240, 320), dtype=torch.float32, device="cuda") for _ in range(6)],
                  "index": [torch.empty((240, 320), dtype=torch.int32, device="cuda") for _ in range(6)]}
        torch.cuda.synchronize()
        st = eng.render_maps_device(d_store, n, keep_t.data_ptr(), range(6), [x.data_ptr() for x in planes["depth"]],
                                    [x.data_ptr() for x in planes["index"]])
        keep = keep_t.cpu().numpy()
        assert int(keep.sum()) == len(surv)
        host = eng.render_maps(surv)
    # the store's index -> the survivor's rank
    rank = np.cumsum(keep != 0) - 1
    for k in range(6):
        assert RR.same_bits(planes["depth"][k].cpu().numpy(), host["depth"][k])
        idx = planes["index"][k].cpu().numpy()
        assert np.array_equal(np.where(idx >= 0, rank[np.maximum(idx, 0)], -1), host["index"][k])
    assert {c: st[c] for c in COUNTS} == {c: host["stats"][c] for c in COUNTS}
    assert st["covered_pixels"] > 0 and st["render_ms"] > 0


def test_cli_depth_maps(tmp_path):
    """densify --filter --depth-maps: the PLY is the filtered store, the PFM
    files equal Engine.render_maps of that store, the report carries depth_maps"""
    from test_cli import run

    d = str(tmp_path / "scene")
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    ply, maps = tmp_path / "points.ply", tmp_path / "maps"
    report = json.loads(run("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o",
                            str(ply), "--filter", "--depth-maps", str(maps), "--depth-normals").stdout)
    sc = SceneCase(V=4, W=160, H=120, kind=1)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        store, _ = eng.densify(sc.seeds)
        store = store[eng.filter_patches(store) == 1]
        want = eng.render_maps(store, normals=True)
    ref = tmp_path / "ref.ply"
    dp.write_ply(str(ref), store)
    assert ply.read_bytes() == ref.read_bytes() and len(store) > 0
    for v in range(4):
        assert RR.same_bits(dp.read_pfm(str(maps / ("depth_%04d.pfm" % v))), want["depth"][v])
        assert RR.same_bits(dp.read_pfm(str(maps / ("normal_%04d.pfm" % v))), want["normal"][v])
    dm = report["depth_maps"]
    assert dm["views"] == 4 and dm["covered_pixels"] == want["stats"]["covered_pixels"] > 0
    assert dm["render_ms"] > 0
