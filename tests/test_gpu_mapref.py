"""dp_refine_maps on the GPU against the CPU reference (tests/mapref_ref.py,
restated from the header's spec): every output plane (depth, normal, score,
choice) and the six integer statistics, bit for bit."""
import numpy as np
import pytest

import densepoints_amd as dp

import mapref_ref as MR
from test_gpu_iterate import planted, to_device
from test_gpu_parity import SceneCase, scene

pytestmark = pytest.mark.gpu

PLANES = ("depth", "normal", "score", "choice")
SENTINEL = 0xA5
# the hf6 case: every candidate kind at a cost the reference pays in seconds
HF6 = dict(window=3, sweep=1, reach=(2, 0), max_sources=3, top_k=2)


def views_of(orc, sc, level=0):
    P, imgs = (sc.P, sc.imgs) if level == 0 else orc.level_scene(sc.P, sc.imgs, level)
    return MR.Views(orc, P, imgs)


def reference(vw, depth, normal, **kw):
    kw = dict(kw)
    flags = MR.KEEP_UNSCORED if kw.pop("keep_unscored", False) else 0
    return MR.refine(vw, depth, normal, flags=flags, **kw)


def assert_equal(got, want):
    assert {c: got["stats"][c] for c in MR.COUNTS} == want["stats"]
    for key in PLANES:
        assert len(got[key]) == len(want[key])
        for k, (a, b) in enumerate(zip(got[key], want[key])):
            assert MR.same_bytes(a, b), "%s plane %d: %d pixels differ" % (
                key, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def refine_device(eng, depth, normal, views=None, skip=(), pad=64, **kw):
    """refine_maps_device on torch tensors with sentinel-filled, padded output
    buffers; `skip`: (plane name, rank) entries passed as NULL.  Returns the
    result in refine_maps's form and the raw buffers."""
    import torch

    views = list(range(len(depth))) if views is None else list(views)
    dd, dn = [to_device(d) for d in depth], [to_device(n) for n in normal]
    words = dict(depth=1, normal=3, score=1, choice=1)
    bufs = {key: [torch.full((d.size * words[key] * 4 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
                  for d in depth] for key in PLANES}
    torch.cuda.synchronize()

    def table(key):
        return [None if (key, k) in skip else t.data_ptr() for k, t in enumerate(bufs[key])]

    st = eng.refine_maps_device(views, [t.data_ptr() for t in dd], [t.data_ptr() for t in dn], table("depth"),
                                table("normal"), table("score"), table("choice"), **kw)
    torch.cuda.synchronize()
    raw = {key: [t.cpu().numpy() for t in bufs[key]] for key in PLANES}
    out = dict(stats=st)
    for key in PLANES:
        out[key] = []
        for d, r in zip(depth, raw[key]):
            body = r[:len(r) - pad].view(np.int32 if key == "choice" else np.float32)
            out[key].append(body.reshape(d.shape + ((3,) if key == "normal" else ())).copy())
    return out, raw


@pytest.fixture(scope="module")
def hf6(orc):
    """the planted hf6 store rendered on the device (Engine.render_maps, itself
    pinned by test_gpu_render.py), its reference refinement (computed once, never
    modified) and an engine with the views set"""
    ref = planted(orc, "parity", 1)
    sc = scene("hf6")
    vw = views_of(orc, sc)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        maps = eng.render_maps(ref["pat"], normals=True)
        want = reference(vw, maps["depth"], maps["normal"], **HF6)
        yield dict(sc=sc, vw=vw, eng=eng, depth=maps["depth"], normal=maps["normal"], want=want, pat=ref["pat"])


@pytest.fixture(scope="module")
def small(orc):
    """3 views of 70 x 50 (the smallest scene of the suite: no side is a multiple
    of 16, a tile row is 5 tiles, the last 6 pixels wide): the unrefined seed
    patches of a dense seed grid, splatted at twice their radius"""
    sc = SceneCase(V=3, W=70, H=50, kind=1, seed_stride_px=6.0)
    vw = views_of(orc, sc)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        maps = eng.render_maps(eng.seeds_to_patches(sc.seeds), normals=True, splat_scale=2.0)
        want = reference(vw, maps["depth"], maps["normal"])
        yield dict(sc=sc, vw=vw, eng=eng, depth=maps["depth"], normal=maps["normal"], want=want)


def test_premises(hf6, small):
    """checked on the reference's output, before any GPU refinement: the cases
    exercise a moved choice, a filled pixel, a void candidate and a rejected pixel"""
    for case, kw in ((hf6, HF6), (small, dp.pmvs.MAPREF_DEFAULTS)):
        want, st = case["want"], case["want"]["stats"]
        ncands = 1 + 2 * kw["sweep"] + 4 * sum(d > 0 for d in kw["reach"])
        assert st["depth_pixels_in"] == sum(int((d > 0).sum()) for d in case["depth"]) > 0
        assert st["moved"] > 0 and st["filled"] > 0 and st["kept"] > st["moved"]
        assert st["candidates"] < ncands * sum(int((n > 0).sum()) for n in want["ncand"])  # a void candidate
        rejected = sum(int(((n > 0) & (c == -1)).sum()) for n, c in zip(want["ncand"], want["choice"]))
        assert rejected > 0
        assert st["source_scores"] > st["candidates"]
        assert len({int(c) for ch in want["choice"] for c in np.unique(ch)}) > 4


@pytest.mark.parametrize("form", ["host", "device"])
def test_hf6_equals_reference_bit_for_bit(hf6, form):
    if form == "host":
        got = hf6["eng"].refine_maps(hf6["depth"], hf6["normal"], **HF6)
    else:
        got, _ = refine_device(hf6["eng"], hf6["depth"], hf6["normal"], **HF6)
    assert_equal(got, hf6["want"])
    assert got["stats"]["refine_ms"] > 0


def test_small_defaults(small):
    assert_equal(small["eng"].refine_maps(small["depth"], small["normal"]), small["want"])


@pytest.mark.parametrize("kw", [
    dict(window=3, sweep=0, reach=(0, 0), top_k=1, min_ncc=-1.0),
    dict(window=11, sweep=2, reach=(16, 0), max_sources=2, top_k=2, min_ncc=1.0),
    dict(window=5, sweep=1, reach=(0, 3), sources=[[2], [0, 2], [1]], max_sources=2, top_k=1, keep_unscored=True),
    dict(window=7, sweep=0, reach=(1, 4), min_ncc=-1.0, keep_unscored=True),
    dict(window=9, sweep=2, reach=(1, 4), views=[2, 0], max_sources=1, top_k=1),
    dict(window=7, sweep=2, reach=(0, 0), step_px=0.5, max_sources=8, top_k=2, min_ncc=0.5),
], ids=["w3-own", "w11-reach16", "w5-sources-keep", "w7-reach-keep", "w9-subset", "w7-sweep-half"])
def test_options(small, kw):
    views = kw.get("views", range(3))
    depth, normal = [small["depth"][v] for v in views], [small["normal"][v] for v in views]
    want = reference(small["vw"], depth, normal, **kw)
    assert want["stats"]["candidates"] > 0 and want["stats"]["depth_pixels_in"] > 0
    if kw.get("keep_unscored"):
        assert any((c == -2).any() for c in want["choice"])
    if kw.get("min_ncc") == -1.0:
        assert want["stats"]["kept"] == sum(int((n > 0).sum()) for n in want["ncand"])
    if kw.get("min_ncc") == 1.0:
        assert want["stats"]["kept"] < want["stats"]["depth_pixels_in"] // 4
    assert_equal(small["eng"].refine_maps(depth, normal, **kw), want)
    got, _ = refine_device(small["eng"], depth, normal, **kw)
    assert_equal(got, want)


def test_level_one(orc, hf6):
    sc = hf6["sc"]
    vw = views_of(orc, sc, 1)
    views = [4, 1, 2]
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        eng.build_pyramid(2)
        eng.set_level(1)
        maps = eng.render_maps(hf6["pat"], views=views, normals=True)
        assert all(d.shape == (120, 160) for d in maps["depth"])
        want = reference(vw, maps["depth"], maps["normal"], views=views)
        assert want["stats"]["moved"] > 0 and want["stats"]["filled"] > 0
        assert_equal(eng.refine_maps(maps["depth"], maps["normal"], views=views), want)


def test_two_chained_passes(small):
    eng = small["eng"]
    one = small["want"]
    two = reference(small["vw"], one["depth"], one["normal"])
    assert two["stats"] != one["stats"] and two["stats"]["filled"] > 0
    g1 = eng.refine_maps(small["depth"], small["normal"])
    g2 = eng.refine_maps(g1["depth"], g1["normal"])
    assert_equal(g1, one)
    assert_equal(g2, two)


@pytest.fixture(scope="module")
def adversarial(small):
    """planes with no scene meaning: each depth plane its render times a seeded
    random factor in [0.97, 1.03] with a sprinkling of 0, NaN, +-inf and negative
    values; random unit normals with zeros and NaNs, and normals perpendicular
    to the pixel's ray (rounded to f32, so the plane's denominator at the pixel
    is zero or tiny with either sign)"""
    rng = np.random.default_rng(20261020)
    vw = small["vw"]
    depth, normal = [], []
    for v, d in enumerate(small["depth"]):
        z = (d * rng.uniform(0.97, 1.03, d.shape).astype(np.float32)).astype(np.float32)
        for value in (0.0, np.nan, np.inf, -1.5, -np.inf):
            z[rng.random(d.shape) < 0.01] = value
        n = rng.normal(size=d.shape + (3,))
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        y, x = np.mgrid[0:d.shape[0], 0:d.shape[1]].astype(np.float64)
        ray = np.einsum("ij,hwj->hwi", np.linalg.inv(np.array(vw.P[v])[:, :3]), np.stack([x, y, np.ones_like(x)], 2))
        perp = np.cross(ray, rng.normal(size=ray.shape))
        sel = rng.random(d.shape) < 0.05
        n[sel] = perp[sel]
        n = n.astype(np.float32)
        n[rng.random(d.shape) < 0.01] = 0.0
        n[rng.random(d.shape) < 0.005] = np.nan
        depth.append(z)
        normal.append(n)
    return depth, normal


@pytest.mark.parametrize("kw", [dict(min_ncc=-1.0), dict(min_ncc=0.2, keep_unscored=True, window=5)],
                         ids=["all", "keep"])
def test_adversarial_planes(small, adversarial, kw):
    depth, normal = adversarial
    want = reference(small["vw"], depth, normal, **kw)
    st = want["stats"]
    assert st["candidates"] > 0 and st["moved"] > 0 and st["filled"] > 0
    assert st["depth_pixels_in"] < sum(int((d > 0).sum()) for d in small["depth"])
    assert_equal(small["eng"].refine_maps(depth, normal, **kw), want)
    got, _ = refine_device(small["eng"], depth, normal, **kw)
    assert_equal(got, want)


def test_null_entries_and_padding_are_never_written(small):
    skip = {("depth", 1), ("normal", 0), ("score", 2), ("choice", 1)}
    got, raw = refine_device(small["eng"], small["depth"], small["normal"], skip=skip, pad=64)
    want = small["want"]
    assert {c: got["stats"][c] for c in MR.COUNTS} == want["stats"]
    for key in PLANES:
        for k, r in enumerate(raw[key]):
            assert (r[-64:] == SENTINEL).all()
            if (key, k) in skip:
                assert (r == SENTINEL).all()
            else:
                assert MR.same_bytes(got[key][k], want[key][k])
    # whole output arrays may be NULL too, and without stats the call returns None
    import torch

    dd, dn = [to_device(d) for d in small["depth"]], [to_device(n) for n in small["normal"]]
    out = [torch.full((d.size * 4,), SENTINEL, dtype=torch.uint8, device="cuda") for d in small["depth"]]
    torch.cuda.synchronize()
    assert small["eng"].refine_maps_device(range(3), [t.data_ptr() for t in dd], [t.data_ptr() for t in dn],
                                           d_score_out=[t.data_ptr() for t in out], stats=False) is None
    torch.cuda.synchronize()
    for t, w in zip(out, want["score"]):
        assert t.cpu().numpy().tobytes() == w.tobytes()


def test_library_refuses_aliased_and_missing_planes(small):
    import ctypes

    from densepoints_amd import _native as N

    eng = small["eng"]
    vid = np.arange(3, dtype=np.int32)
    tab = (ctypes.c_void_p * 3)(*[d.ctypes.data for d in small["depth"]])
    ntab = (ctypes.c_void_p * 3)(*[n.ctypes.data for n in small["normal"]])
    args = (eng._ctx, N.ptr(vid), 3, None, None)
    assert N.lib.dp_refine_maps(*args, tab, ntab, tab, None, None, None, None) == N.DP_E_ARG
    assert N.lib.dp_refine_maps(*args, tab, None, None, None, None, None, None) == N.DP_E_ARG
    src = np.array([[0, -1, -1, -1], [0, -1, -1, -1], [0, -1, -1, -1]], np.int32)
    assert N.lib.dp_refine_maps(eng._ctx, N.ptr(vid), 3, None, N.ptr(src), tab, ntab, None, None, None, None,
                                None) == N.DP_E_ARG


def test_pmvs_depth_maps_refine_reproduces_the_engine(hf6):
    sc = hf6["sc"]
    p = dp.PMVS()
    for v in sc.views:
        p.add_camera(v)
    assert p.run(sc.seeds, filter_passes=3)
    plain = p.depth_maps(normals=True)
    assert "choice" not in plain and p.depth_maps()["depth"][0].tobytes() == plain["depth"][0].tobytes()
    got = p.depth_maps(refine=1, **HF6)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        want = eng.refine_maps(plain["depth"], plain["normal"], **HF6)
        two = eng.refine_maps(want["depth"], want["normal"], **HF6)
    for key in PLANES:
        assert all(MR.same_bytes(a, b) for a, b in zip(got[key], want[key])), key
    assert {c: got["refine_stats"][0][c] for c in MR.COUNTS} == {c: want["stats"][c] for c in MR.COUNTS}
    assert all(MR.same_bytes(a, b) for a, b in zip(got["index"], plain["index"]))
    assert all(MR.same_bytes(a, b) for a, b in zip(p.depth_maps(refine=2, **HF6)["depth"], two["depth"]))
    # fused_cloud(refine=1) fuses the refined planes
    cloud = p.fused_cloud(refine=1, **HF6)
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        pts, _ = eng.fuse_maps(want["depth"], want["normal"])
    assert cloud.tobytes() == pts.tobytes() and len(cloud) > 0
    assert p.stats["refine"][0]["kept"] == want["stats"]["kept"]
    assert p.fused_cloud().tobytes() != cloud.tobytes()
