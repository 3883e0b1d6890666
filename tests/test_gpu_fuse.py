"""dp_fuse_maps on the GPU against the CPU reference (tests/fuse_ref.py, restated
from the header's spec): every field of every point, the order, n_out and the
five integer statistics, bit for bit."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import FUSED_DTYPE

import fuse_ref as FR
from test_gpu_iterate import planted, to_device
from test_gpu_parity import SceneCase, scene

pytestmark = pytest.mark.gpu

COUNTS = ("depth_pixels", "matched_pairs", "consistent_pairs", "fusable", "emitted")
SENTINEL = 0xA5


def views_of(orc, sc, level=0):
    P, imgs = (sc.P, sc.imgs) if level == 0 else orc.level_scene(sc.P, sc.imgs, level)
    return FR.Views(P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], imgs)


def assert_equal(got, want):
    pts, st = got
    assert {c: st[c] for c in COUNTS} == want["stats"]
    assert pts.dtype == FUSED_DTYPE and len(pts) == len(want["points"])
    for f in FUSED_DTYPE.names:
        assert FR.same_bytes(pts[f], want["points"][f]), f
    assert pts.tobytes() == want["points"].astype(FUSED_DTYPE).tobytes()


def fuse_device(eng, depth, normal, views=None, cap=None, **kw):
    """fuse_maps_device on torch tensors: (points, stats, n_out, the whole
    sentinel-filled point buffer as bytes)"""
    import torch

    views = list(range(len(depth))) if views is None else list(views)
    dd = [to_device(d) for d in depth]
    dn = [to_device(n) for n in normal] if normal is not None else None
    total = sum(d.size for d in depth)
    cap = total if cap is None else cap
    buf = torch.full((max(cap + 3, 1) * FUSED_DTYPE.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, st = eng.fuse_maps_device(views, [t.data_ptr() for t in dd], [t.data_ptr() for t in dn] if dn else None,
                                 buf.data_ptr() if cap else None, cap, **kw)
    raw = buf.cpu().numpy()
    pts = raw[:min(n, cap) * FUSED_DTYPE.itemsize].view(FUSED_DTYPE).copy()
    return pts, st, n, raw


@pytest.fixture(scope="module")
def hf6(orc):
    """the planted hf6 store rendered on the device (Engine.render_maps, itself
    pinned by test_gpu_render.py), the reference fusions of those planes
    (computed once, never modified), and an engine with the views set"""
    ref = planted(orc, "parity", 1)
    sc = scene("hf6")
    vw = views_of(orc, sc)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        maps = eng.render_maps(ref["pat"], normals=True)
        depth, normal = maps["depth"], maps["normal"]
        want = {True: FR.fuse(vw, depth, normal), False: FR.fuse(vw, depth, None)}
        yield dict(sc=sc, vw=vw, eng=eng, depth=depth, normal=normal, want=want, pat=ref["pat"])


def test_hf6_premises(hf6):
    """checked on the reference's output, before any GPU fusion: the case
    exercises the suppression, a rejection and several view counts"""
    for with_normals in (True, False):
        want = hf6["want"][with_normals]
        st = want["stats"]
        assert st["emitted"] > 0
        assert st["fusable"] > st["emitted"]                   # suppression acted
        assert st["matched_pairs"] > st["consistent_pairs"]    # a disagreement was rejected
        assert len(set(want["points"]["n_views"].tolist())) > 1
    # the normal test rejects pairs that the depth test alone accepts
    assert hf6["want"][True]["stats"]["consistent_pairs"] < hf6["want"][False]["stats"]["consistent_pairs"]
    assert len({tuple(c) for c in hf6["want"][True]["points"]["rgb"][:2000].tolist()}) > 10


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("with_normals", [True, False])
def test_hf6_equals_reference_bit_for_bit(hf6, with_normals, form):
    normal = hf6["normal"] if with_normals else None
    want = hf6["want"][with_normals]
    if form == "host":
        got = hf6["eng"].fuse_maps(hf6["depth"], normal)
    else:
        pts, st, n, _ = fuse_device(hf6["eng"], hf6["depth"], normal)
        assert n == len(pts)
        got = (pts, st)
    assert_equal(got, want)
    assert got[1]["fuse_ms"] > 0


def test_width_that_is_no_multiple_of_the_wave(orc):
    """3 views of 70 x 50: a plane is 3500 pixels = 54 waves and 44 pixels, and a
    wave spans image rows; the patches are the unrefined seed patches of a dense
    seed grid (the scene is too small for the densify to grow a store)"""
    sc = SceneCase(V=3, W=70, H=50, kind=1, seed_stride_px=6.0)
    vw = views_of(orc, sc)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        maps = eng.render_maps(eng.seeds_to_patches(sc.seeds), normals=True, splat_scale=2.0)
        for normal in (maps["normal"], None):
            for kw in (dict(min_views=1), dict(min_views=0, suppress=False)):
                want = FR.fuse(vw, maps["depth"], normal, min_views=kw["min_views"],
                               flags=0 if kw.get("suppress", True) else FR.NO_SUPPRESS)
                assert want["stats"]["emitted"] > 0 and want["stats"]["consistent_pairs"] > 0
                assert_equal(eng.fuse_maps(maps["depth"], normal, **kw), want)


def test_level_one(orc, hf6):
    sc = hf6["sc"]
    vw = views_of(orc, sc, 1)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        eng.build_pyramid(2)
        eng.set_level(1)
        maps = eng.render_maps(hf6["pat"], normals=True)
        assert all(d.shape == (120, 160) for d in maps["depth"])
        want = FR.fuse(vw, maps["depth"], maps["normal"])
        assert want["stats"]["emitted"] > 0 and want["stats"]["fusable"] > want["stats"]["emitted"]
        assert_equal(eng.fuse_maps(maps["depth"], maps["normal"]), want)


@pytest.mark.parametrize("kw", [dict(min_views=0), dict(min_views=1), dict(min_views=5), dict(depth_tol=0.0),
                                dict(suppress=False), dict(views=[4, 1, 2]), dict(min_normal_cos=0.999)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_options(hf6, kw):
    views = kw.get("views", range(6))
    depth, normal = [hf6["depth"][v] for v in views], [hf6["normal"][v] for v in views]
    ref_kw = {k: v for k, v in kw.items() if k != "suppress"}
    want = FR.fuse(hf6["vw"], depth, normal, flags=0 if kw.get("suppress", True) else FR.NO_SUPPRESS, **ref_kw)
    assert want["stats"]["depth_pixels"] > 0 and want["stats"]["matched_pairs"] > 0
    if kw.get("suppress", True) is False:
        assert want["stats"]["emitted"] == want["stats"]["fusable"] > hf6["want"][True]["stats"]["emitted"]
    if "views" in kw:
        rank = np.array([views.index(v) for v in want["points"]["view"]])
        assert rank[0] == 0 and len(set(rank.tolist())) > 1 and (np.diff(rank) >= 0).all()
    if kw.get("min_views") == 0:
        assert want["stats"]["fusable"] == want["stats"]["depth_pixels"]
    assert_equal(hf6["eng"].fuse_maps(depth, normal, **kw), want)


@pytest.fixture(scope="module")
def adversarial(hf6):
    """planes with no scene meaning: each depth plane its render times a seeded
    random factor in [0.97, 1.03] with a sprinkling of 0, NaN, +inf and negative
    values, and random unit normals -- every rejection branch and rounding
    boundary"""
    rng = np.random.default_rng(20261019)
    depth, normal = [], []
    for d in hf6["depth"]:
        z = (d * rng.uniform(0.97, 1.03, d.shape).astype(np.float32)).astype(np.float32)
        for value in (0.0, np.nan, np.inf, -1.5, -np.inf):
            z[rng.random(d.shape) < 0.01] = value
        n = rng.normal(size=d.shape + (3,))
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        n = n.astype(np.float32)
        n[rng.random(d.shape) < 0.01] = 0.0
        n[rng.random(d.shape) < 0.005] = np.nan
        depth.append(z)
        normal.append(n)
    return depth, normal


@pytest.mark.parametrize("kw", [dict(depth_tol=0.02, min_views=1, min_normal_cos=0.0),
                                dict(depth_tol=0.05, min_views=2, min_normal_cos=0.3),
                                dict(depth_tol=0.02, min_views=1, normals=False)],
                         ids=["cos0", "cos0.3", "plain"])
def test_adversarial_planes(hf6, adversarial, kw):
    depth, normal = adversarial
    kw = dict(kw)
    if not kw.pop("normals", True):
        normal = None
    want = FR.fuse(hf6["vw"], depth, normal, **kw)
    st = want["stats"]
    assert st["matched_pairs"] > st["consistent_pairs"] > 0 and st["fusable"] > st["emitted"] > 0
    assert st["depth_pixels"] < sum(int((d > 0).sum()) for d in hf6["depth"])
    assert_equal(hf6["eng"].fuse_maps(depth, normal, **kw), want)
    pts, dst, n, _ = fuse_device(hf6["eng"], depth, normal, **kw)
    assert n == len(pts)
    assert_equal((pts, dst), want)


def test_device_form_with_a_small_cap(hf6):
    want = hf6["want"][True]
    total = want["stats"]["emitted"]
    size = FUSED_DTYPE.itemsize
    for cap in (total - 1, 1000, 1):
        pts, st, n, raw = fuse_device(hf6["eng"], hf6["depth"], hf6["normal"], cap=cap)
        assert n == total and {c: st[c] for c in COUNTS} == want["stats"]
        assert pts.tobytes() == want["points"][:cap].astype(FUSED_DTYPE).tobytes()
        assert len(raw) == (cap + 3) * size and (raw[cap * size:] == SENTINEL).all()
    # cap = 0 with no buffer at all: the counts only
    pts, st, n, _ = fuse_device(hf6["eng"], hf6["depth"], hf6["normal"], cap=0)
    assert n == total and len(pts) == 0 and st["emitted"] == total


def test_empty_planes_reuse_and_repeatability(hf6):
    eng, want = hf6["eng"], hf6["want"][True]
    zero = [np.zeros_like(d) for d in hf6["depth"]]
    pts, st = eng.fuse_maps(zero, hf6["normal"])
    assert len(pts) == 0 and all(st[c] == 0 for c in COUNTS)
    pts, st, n, _ = fuse_device(eng, zero, None)
    assert n == 0 and len(pts) == 0 and all(st[c] == 0 for c in COUNTS)
    # a smaller view set after a larger one, then the full set again
    a = eng.fuse_maps(hf6["depth"], hf6["normal"])
    sub = [3, 0]
    sub_want = FR.fuse(hf6["vw"], [hf6["depth"][v] for v in sub], [hf6["normal"][v] for v in sub], views=sub,
                       min_views=1)
    assert sub_want["stats"]["emitted"] > 0
    assert_equal(eng.fuse_maps([hf6["depth"][v] for v in sub], [hf6["normal"][v] for v in sub], views=sub,
                               min_views=1), sub_want)
    b = eng.fuse_maps(hf6["depth"], hf6["normal"])
    assert_equal(a, want)
    assert_equal(b, want)
    assert a[0].tobytes() == b[0].tobytes()


def test_device_resident_chain_and_fused_cloud(hf6):
    """densify_iterate -> densify_store_device -> filter_patches_device ->
    render_maps_device -> fuse_maps_device never visits the host; it equals the
    host chain on the copied-out survivors, and so does PMVS.fused_cloud()"""
    import torch

    sc = hf6["sc"]
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        surv, _ = eng.densify_iterate(sc.seeds, 2)
        d_store, n = eng.densify_store_device()
        assert n >= len(surv) > 0
        keep_t = torch.empty(n, dtype=torch.uint8, device="cuda")
        depth = [torch.empty((240, 320), dtype=torch.float32, device="cuda") for _ in range(6)]
        normal = [torch.empty((240, 320, 3), dtype=torch.float32, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        eng.filter_patches_device(d_store, n, keep_t.data_ptr(), 3)
        rst = eng.render_maps_device(d_store, n, keep_t.data_ptr(), range(6), [t.data_ptr() for t in depth], None,
                                     [t.data_ptr() for t in normal])
        cap = rst["covered_pixels"]
        buf = torch.empty(cap * FUSED_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n_out, st = eng.fuse_maps_device(range(6), [t.data_ptr() for t in depth], [t.data_ptr() for t in normal],
                                         buf.data_ptr(), cap)
        assert 0 < n_out <= cap
        chain = buf.cpu().numpy()[:n_out * FUSED_DTYPE.itemsize].view(FUSED_DTYPE)
        maps = eng.render_maps(surv, normals=True)
        host, hst = eng.fuse_maps(maps["depth"], maps["normal"])
    assert chain.tobytes() == host.tobytes() and {c: st[c] for c in COUNTS} == {c: hst[c] for c in COUNTS}
    want = FR.fuse(hf6["vw"], maps["depth"], maps["normal"])
    assert_equal((host, hst), want)
    p = dp.PMVS()
    for v in sc.views:
        p.add_camera(v)
    assert p.run(sc.seeds, filter_passes=3, iterations=2)
    assert p.patches.tobytes() == surv.tobytes()
    cloud = p.fused_cloud()
    assert cloud.dtype == FUSED_DTYPE and cloud.tobytes() == host.tobytes()
    assert p.stats["fused"]["emitted"] == len(cloud)


def test_cli_fuse(tmp_path):
    """densify --filter --fuse: the fused PLY equals write_ply of Engine.fuse_maps
    on the filtered store's maps byte for byte, and the report counts it"""
    from test_cli import run

    d = str(tmp_path / "scene")
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    ply, fused = tmp_path / "points.ply", tmp_path / "fused.ply"
    report = json.loads(run("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o",
                            str(ply), "--filter", "--fuse", str(fused)).stdout)
    sc = SceneCase(V=4, W=160, H=120, kind=1)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        store, _ = eng.densify(sc.seeds)
        store = store[eng.filter_patches(store) == 1]
        maps = eng.render_maps(store, normals=True)
        pts, st = eng.fuse_maps(maps["depth"], maps["normal"])
    ref = tmp_path / "ref.ply"
    dp.write_ply(str(ref), pts)
    assert fused.read_bytes() == ref.read_bytes()
    f = report["fused"]
    assert f["points"] == len(pts) > 0 and f["fusable"] == st["fusable"] and f["depth_pixels"] == st["depth_pixels"]
    assert f["fuse_ms"] > 0
    # the options reach the fusion, and bad values are refused with a message
    report = json.loads(run("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o",
                            str(ply), "--filter", "--fuse", str(fused), "--fuse-min-views", "1", "--fuse-depth-tol",
                            "0.02").stdout)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        pts2, _ = eng.fuse_maps(maps["depth"], maps["normal"], min_views=1, depth_tol=0.02)
    assert report["fused"]["points"] == len(pts2) > len(pts)
    for bad in (("--fuse-min-views", "64"), ("--fuse-depth-tol", "-1"), ("--fuse-depth-tol", "x")):
        r = run("-i", os.path.join(d, "scene.json"), "--fuse", str(fused), *bad, check=False)
        assert r.returncode == 2 and "expects" in r.stderr
