"""dp_render_maps, dp_refine_maps, dp_fuse_maps, dp_tsdf_integrate and
dp_tsdf_mesh in one call over views of unequal size (tests/mapcases.py "mixed")
and over views smaller than the work unit that owns them ("tiny"): a refine tile,
a wave of a fuse plane, a fuse block, the refine window.  Every stage against its
numpy reference, bit for bit, in the host and the device form; each stage reads
the reference's output of the stage before it, so one stage's failure is not
another's.  tests/test_mapcases_cpu.py asserts, on the references alone, that
the scenes put every per-view quantity (W, H, pitch, plane offset) to the test."""
import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import FUSED_DTYPE

import fuse_ref as FR
import mapcases as MC
import mapref_ref as MR
import render_ref as RR
import tsdf_ref as TR
from test_gpu_fuse import assert_equal as fuse_equal
from test_gpu_fuse import fuse_device
from test_gpu_iterate import to_device
from test_gpu_mapref import PLANES
from test_gpu_mapref import assert_equal as refine_equal
from test_gpu_mapref import refine_device
from test_gpu_render import assert_equal as render_equal
from test_gpu_render import render_device
from test_gpu_tsdf import SMALL_VOLUMES, VOLUME_KEYS, assert_mesh, assert_volume, integrate_device, mesh_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 64
FORMS = ["host", "device"]


class Case:
    """a scene, its reference chain (computed once, never modified) and an
    engine with the views set"""

    def __init__(self, orc, name, eng):
        self.sc, self.ch, self.eng, self.orc = MC.build(name), MC.chain(orc, name), eng, orc
        self.pat = self.ch["pat"]
        self.kw = dict(splat_scale=self.sc.splat_scale)


@pytest.fixture(scope="module")
def mixed(orc):
    with dp.Engine(device=0) as eng:
        eng.set_views(MC.build("mixed").views)
        yield Case(orc, "mixed", eng)


@pytest.fixture(scope="module")
def tiny(orc):
    with dp.Engine(device=0) as eng:
        eng.set_views(MC.build("tiny").views)
        yield Case(orc, "tiny", eng)


@pytest.fixture
def case(request, mixed, tiny):
    return {"mixed": mixed, "tiny": tiny}[request.param]


both = pytest.mark.parametrize("case", ["mixed", "tiny"], indirect=True)


def render_padded(eng, pat, views, sizes, **kw):
    """render_maps_device into one sentinel-filled buffer per view and plane,
    each of its own size plus PAD bytes; the same dict as render_maps, after
    asserting that no padding byte was written"""
    import torch

    words = dict(depth=1, index=1, normal=3, score=1)
    dpat = to_device(pat)
    bufs = {key: [torch.full((w * h * words[key] * 4 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
                  for w, h in sizes] for key in words}
    torch.cuda.synchronize()
    st = eng.render_maps_device(dpat.data_ptr(), len(pat), 0, views,
                                *[[t.data_ptr() for t in bufs[key]] for key in ("depth", "index", "normal", "score")],
                                **kw)
    out = dict(views=[int(v) for v in views], stats=st)
    for key in words:
        out[key] = []
        for (w, h), t in zip(sizes, bufs[key]):
            raw = t.cpu().numpy()
            assert (raw[-PAD:] == SENTINEL).all(), "%s: the padding after a %d x %d plane was written" % (key, w, h)
            body = raw[:-PAD].view(np.int32 if key == "index" else np.float32)
            out[key].append(body.reshape((h, w, 3) if key == "normal" else (h, w)).copy())
    return out


def render(case, form, views=None, level_sizes=None, **kw):
    sizes = case.sc.sizes if level_sizes is None else level_sizes
    ids = list(range(case.sc.V)) if views is None else list(views)
    kw = dict(case.kw, **kw)
    if form == "host":
        return case.eng.render_maps(case.pat, views=views, normals=True, scores=True, **kw)
    return render_padded(case.eng, case.pat, ids, [sizes[v] for v in ids], **kw)


def refine(case, form, depth, normal, views=None, **kw):
    if form == "host":
        return case.eng.refine_maps(depth, normal, views=views, **kw)
    got, raw = refine_device(case.eng, depth, normal, views=views, pad=PAD, **kw)
    for key in PLANES:
        assert all((r[-PAD:] == SENTINEL).all() for r in raw[key]), key
    return got


def fuse(case, form, depth, normal, views=None, **kw):
    if form == "host":
        return case.eng.fuse_maps(depth, normal, views=views, **kw)
    pts, st, n, raw = fuse_device(case.eng, depth, normal, views=views, **kw)
    assert n == len(pts) and (raw[n * FUSED_DTYPE.itemsize:] == SENTINEL).all()
    return pts, st


def integrate(case, form, depth, views=None):
    if form == "host":
        return case.eng.tsdf_integrate(depth, views, **MC.VOLUME)
    return integrate_device(case.eng, depth, views, **MC.VOLUME)


def mesh(case, form, volume):
    if form == "host":
        return case.eng.tsdf_mesh(volume)
    verts, tris, st, nv, nt, vraw, traw = mesh_device(case.eng, volume)
    assert (nv, nt) == (len(verts), len(tris))
    assert (vraw[nv * 16:] == SENTINEL).all() and (traw[nt * 12:] == SENTINEL).all()
    return verts, tris, st


def reference_mesh(vol):
    return TR.mesh(vol["tsdf"], vol["weight"], vol["rgb"], origin=MC.VOLUME["origin"], voxel=MC.VOLUME["voxel"],
                   dim=MC.VOLUME["dim"])


def test_the_scenes_reach_the_engine_as_built(mixed, tiny):
    assert MC.VOLUME == SMALL_VOLUMES["19x17x13"] and set(MC.VOLUME) == set(VOLUME_KEYS)
    for case in (mixed, tiny):
        assert case.eng.view_sizes() == case.sc.sizes
        # the device's seed conversion is the oracle's on these views too
        assert case.eng.seeds_to_patches(case.sc.seeds).tobytes() == case.pat.tobytes()


# ---------------------------------------------------------------------------
# the four stages on both scenes, host and device form
# ---------------------------------------------------------------------------
@both
@pytest.mark.parametrize("form", FORMS)
def test_render(case, form):
    want = case.ch["render"]
    assert want["stats"]["covered_pixels"] > 0
    render_equal(render(case, form), want)


@pytest.fixture(scope="module")
def wide_reference(orc):
    """MR.refine of the mixed scene with the widest window and reach (once)"""
    ch = MC.chain(orc, "mixed")
    return MR.refine(ch["mvw"], ch["render"]["depth"], ch["render"]["normal"], **MC.WIDE)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("options", ["defaults", "w11-reach16"])
def test_refine_mixed(mixed, wide_reference, options, form):
    rd = mixed.ch["render"]
    want, kw = (mixed.ch["refine"], {}) if options == "defaults" else (wide_reference, MC.WIDE)
    assert want["stats"]["kept"] > 0 and want["stats"]["moved"] > 0 and want["stats"]["filled"] > 0
    refine_equal(refine(mixed, form, rd["depth"], rd["normal"], **kw), want)


@pytest.fixture(scope="module")
def tiny_keep_reference(orc):
    ch = MC.chain(orc, "tiny")
    return MR.refine(ch["mvw"], ch["render"]["depth"], ch["render"]["normal"], window=11, flags=MR.KEEP_UNSCORED)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("options", ["defaults", "w11-keep"])
def test_refine_tiny(tiny, tiny_keep_reference, options, form):
    rd = tiny.ch["render"]
    if options == "defaults":
        want, kw = tiny.ch["refine"], {}
        assert want["stats"]["kept"] > 0
    else:
        want, kw = tiny_keep_reference, dict(window=11, keep_unscored=True)
        assert all((want["choice"][k] == -2).any() for k in (2, 3, 4))
    refine_equal(refine(tiny, form, rd["depth"], rd["normal"], **kw), want)


@both
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "plain"])
def test_fuse(case, with_normals, form):
    maps = case.ch["maps"]
    normal = maps["normal"] if with_normals else None
    want = case.ch["fuse"] if with_normals else FR.fuse(case.ch["fvw"], maps["depth"], None)
    assert want["stats"]["matched_pairs"] > 0
    if case.sc.name == "mixed":
        assert want["stats"]["emitted"] > 0
    fuse_equal(fuse(case, form, maps["depth"], normal), want)


@pytest.mark.parametrize("form", FORMS)
def test_fuse_tiny_every_depth_pixel_is_fusable(tiny, form):
    """min_views = 0: the planes of one row, of one column and of 15 pixels emit"""
    maps = tiny.ch["maps"]
    for suppress in (True, False):
        want = FR.fuse(tiny.ch["fvw"], maps["depth"], maps["normal"], min_views=0,
                       flags=0 if suppress else FR.NO_SUPPRESS)
        assert (np.bincount(want["points"]["view"], minlength=5) > 0).all()
        fuse_equal(fuse(tiny, form, maps["depth"], maps["normal"], min_views=0, suppress=suppress), want)


@both
@pytest.mark.parametrize("form", FORMS)
def test_tsdf_and_mesh(case, form):
    want = case.ch["tsdf"]
    assert want["stats"]["observed_voxels"] > 0
    assert_volume(integrate(case, form, case.ch["maps"]["depth"]), want)
    mwant = reference_mesh(want)
    if case.sc.name == "mixed":
        assert mwant["stats"]["triangles"] > 0
    assert_mesh(mesh(case, form, dict(want, **MC.VOLUME)), mwant)


@pytest.mark.parametrize("form", FORMS)
def test_tsdf_tiny_the_row_and_the_column_alone(tiny, form):
    views = [3, 2]  # 1 x 19, then 17 x 1
    depth = MC.pick(tiny.ch["maps"]["depth"], views)
    want = TR.integrate(tiny.ch["tvw"], depth, views, **MC.VOLUME)
    assert all(c.any() for c in want["counted"])
    assert_volume(integrate(tiny, form, depth, views), want)
    assert_mesh(mesh(tiny, form, dict(want, **MC.VOLUME)), reference_mesh(want))


# ---------------------------------------------------------------------------
# subsets in an order where the rank is not the id, explicit sources, level 1
# ---------------------------------------------------------------------------
_subsets = {}  # the reference chain of a subset, shared by the two forms
# two or three views: one score per candidate and one agreeing view, or nothing is kept or fused
SUBSET = dict(refine_kw=dict(top_k=1), fuse_kw=dict(min_views=1))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("views", [[4, 2, 0], [0, 4]], ids=["4-2-0", "0-4"])
def test_subset_and_order_through_every_stage(mixed, views, form):
    """small before large and large before small: each stage equals its
    reference called with the same `views`"""
    if tuple(views) not in _subsets:
        _subsets[tuple(views)] = MC.run_chain(mixed.orc, mixed.sc, views=views, patches=mixed.pat, **SUBSET)
    ch = _subsets[tuple(views)]
    assert ch["render"]["views"] == views and ch["refine"]["stats"]["kept"] > 0
    assert ch["fuse"]["stats"]["emitted"] > 0 and ch["tsdf"]["stats"]["observed_voxels"] > 0
    render_equal(render(mixed, form, views), ch["render"])
    rd, rf = ch["render"], ch["refine"]
    refine_equal(refine(mixed, form, rd["depth"], rd["normal"], views, **SUBSET["refine_kw"]), rf)
    fuse_equal(fuse(mixed, form, rf["depth"], rf["normal"], views, **SUBSET["fuse_kw"]), ch["fuse"])
    assert_volume(integrate(mixed, form, rf["depth"], views), ch["tsdf"])


def test_subset_with_fewer_sources_than_top_k_scores_nothing(mixed):
    """two views and the default top_k = 2: one source at most, so no candidate"""
    views = [0, 4]
    rd = _subsets[(0, 4)]["render"] if (0, 4) in _subsets else RR.render(mixed.ch["cams"], mixed.pat, views=views,
                                                                          splat_scale=mixed.sc.splat_scale)
    want = MR.refine(mixed.ch["mvw"], rd["depth"], rd["normal"], views=views)
    assert want["stats"]["candidates"] == 0 and want["stats"]["source_scores"] > 0
    refine_equal(refine(mixed, "host", rd["depth"], rd["normal"], views), want)


def test_subset_render_reads_the_imported_device_helper_too(mixed):
    views = [4, 2, 0]
    want = RR.render(mixed.ch["cams"], mixed.pat, views=views, splat_scale=mixed.sc.splat_scale)
    got = render_device(mixed.eng, mixed.pat, None, views, MC.pick(mixed.sc.sizes, views), **mixed.kw)
    render_equal(got, want)


@pytest.mark.parametrize("form", FORMS)
def test_refine_explicit_sources_smallest_against_largest(mixed, form):
    """rows that pair the 15 x 13 view with the 131 x 67 view in both directions"""
    rd = mixed.ch["render"]
    sources = [[4, 2], [2], [4], [4, 2], [2]]
    kw = dict(sources=sources, max_sources=2, top_k=1)
    want = MR.refine(mixed.ch["mvw"], rd["depth"], rd["normal"], **kw)
    assert (want["valid"][2] > 0).any() and (want["valid"][4] > 0).any() and want["stats"]["kept"] > 0
    refine_equal(refine(mixed, form, rd["depth"], rd["normal"], **kw), want)


def test_level_one(orc, mixed):
    sc, views = mixed.sc, [2, 1, 4]
    sizes = sc.level_sizes(orc, 1)
    assert len(set(sizes)) == 5
    ch = MC.run_chain(orc, sc, views=views, level=1, patches=mixed.pat, **SUBSET)
    assert ch["render"]["stats"]["covered_pixels"] > 0 and ch["refine"]["stats"]["kept"] > 0
    assert ch["fuse"]["stats"]["matched_pairs"] > 0
    with dp.Engine(device=0) as eng:
        eng.set_views(sc.views)
        eng.build_pyramid(2)
        eng.set_level(1)
        assert eng.view_sizes() == sizes
        at = Case.__new__(Case)
        at.sc, at.eng, at.pat, at.kw = sc, eng, mixed.pat, mixed.kw
        rd, rf = ch["render"], ch["refine"]
        for form in FORMS:
            render_equal(render(at, form, views, level_sizes=sizes), rd)
            refine_equal(refine(at, form, rd["depth"], rd["normal"], views, **SUBSET["refine_kw"]), rf)
            fuse_equal(fuse(at, form, rf["depth"], rf["normal"], views, **SUBSET["fuse_kw"]), ch["fuse"])


# ---------------------------------------------------------------------------
# the chain through PMVS
# ---------------------------------------------------------------------------
def test_pmvs_chain_reproduces_the_engine(mixed):
    """PMVS.depth_maps(refine=1), fused_cloud(refine=1) and mesh() over the mixed
    views equal the Engine composition byte for byte.  The store is the seed
    patches: views this small grow none (the oracle's densify keeps 2 patches)."""
    sc = mixed.sc
    p = dp.PMVS()
    for v in sc.views:
        p.add_camera(v)
    p.patches, p._ran = mixed.pat, True
    kw = mixed.kw
    got = p.depth_maps(refine=1, **kw)
    eng = mixed.eng
    plain = eng.render_maps(mixed.pat, normals=True, **kw)
    want = eng.refine_maps(plain["depth"], plain["normal"])
    for key in PLANES:
        assert all(MR.same_bytes(a, b) for a, b in zip(got[key], want[key])), key
    assert {c: got["refine_stats"][0][c] for c in MR.COUNTS} == {c: want["stats"][c] for c in MR.COUNTS}
    assert all(MR.same_bytes(a, b) for a, b in zip(got["index"], plain["index"]))
    refine_equal(want, mixed.ch["refine"])
    cloud = p.fused_cloud(refine=1, **kw)
    pts, _ = eng.fuse_maps(want["depth"], want["normal"])
    assert cloud.tobytes() == pts.tobytes() and len(cloud) == mixed.ch["fuse"]["stats"]["emitted"] > 0
    verts, tris = p.mesh(refine=1, dim=24, **kw)
    info = p.stats["mesh"]
    vol = {k: info[k] for k in VOLUME_KEYS}
    volume = eng.tsdf_integrate(want["depth"], **vol)
    v2, t2, mst = eng.tsdf_mesh(volume, info["min_weight"])
    assert verts.tobytes() == v2.tobytes() and tris.tobytes() == t2.tobytes() and len(tris) > 0
    ref = TR.integrate(mixed.ch["tvw"], want["depth"], **vol)
    assert_volume(volume, ref)
    assert_mesh((verts, tris, info["mesh"]), TR.mesh(ref["tsdf"], ref["weight"], ref["rgb"], origin=vol["origin"],
                                                     voxel=vol["voxel"], dim=vol["dim"], min_weight=info["min_weight"]))
