"""One table of every Engine method that takes a `stream`: for each form a small
real input, a poison input of the same dtype, shape and stride that is valid
input and gives another answer, the call, its output buffers and where the
expected result comes from.  tests/test_streamcases_cpu.py checks the table
itself (coverage, the poison's validity and its power); tests/
test_gpu_caller_stream.py runs every form on a caller's stream behind pending
work.

A Case has
  make(kind)      the inputs ("real", "poison" or "other": a second real input
                  for the back-to-back test) as a dict of numpy arrays
  outs            the bytes of every output buffer (written only by the call)
  inout           the inputs the call rewrites in place (read back as outputs)
  call(eng, p, stream, stats)   p: the device address of every buffer by name
  ref(I)          the CPU reference: (expected leading bytes of every output --
                  the rest of a buffer keeps its sentinel --, the integer
                  statistics, the values the call returns); None where the
                  expected result is the form's own run on the default stream
                  after a full synchronize (the forms that need the views: their
                  own tests pin that run to the oracle or to their reference)
  host(ret), counters(ret)   what the call returned, split the same way

No GPU use at import or in ref(); make() uses the engine it is given only in
the four cases marked gpu_inputs, whose planes are rendered (the GPU test
checks those inputs' validity instead of tests/test_streamcases_cpu.py)."""
import functools

import numpy as np

import densepoints_amd as dp
from densepoints_amd import _native as N
from densepoints_amd import synth

import cloudalign_ref as AR
import cloudknn_ref as KR
import cloudnearest_ref as CR
import cloudnormals_ref as NR
import mesh_ref as MC
import meshdecimate_ref as MD
import meshnearest_ref as MN
import meshsmooth_ref as MS
import tsdf_ref as TR

# every stream-taking method that is neither in CASES nor in CHAINED, with the reason (at most 3)
NOT_COVERED = {}

# The three forms of the multi-rank generation protocol read the context's own
# generation and each other's results, so they run as one chain (tests/
# test_gpu_caller_stream.py test_generation_protocol_on_a_callers_stream): the
# slot-exchange scene of tests/test_gpu_partition_edges.py, three ranks, every
# generation behind a delay.  What a caller hands over -- the item list of
# densify_refine_share_async -- is poisoned with other valid item indices.
CHAINED = {
    "densify_partition_async": "generation_protocol",
    "densify_refine_share_async": "generation_protocol",
    "densify_commit_gathered_device": "generation_protocol",
}

NPTS = 257  # one item past a block of 256
VERTEX = N.MESH_VERTEX_DTYPE
PATCH = N.PATCH_DTYPE


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Case:
    views = False      # needs the scene's views loaded
    no_wait = False    # queues without a host wait (with stats=False where it has stats)
    has_stats = False  # takes stats=
    inout = ()
    setup = None       # called with the fresh engine before the first call

    def __init__(self, name, make, outs, call, ref=None, host=None, counters=None, **kw):
        self.name, self.outs, self.call, self.ref = name, outs, call, ref
        # inputs made with an engine (gpu_inputs) are cached by the GPU test, not here
        self.make = make if kw.get("gpu_inputs") else functools.lru_cache(None)(make)
        self.host = host or (lambda ret: {})
        self.counters = counters or (lambda ret: {})
        self.__dict__.update(kw)


def cloud(seed, n=NPTS, scale=1.0, shift=0.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) * np.float32(scale) + np.float32(shift)).astype(np.float32)


SEEDS = {"real": 1, "poison": 2, "other": 3}
CASES = {}


def add(name, **kw):
    def deco(make):
        CASES[name] = Case(name, make, **kw)
        return make
    return deco


def counts_of(names):
    return lambda st: {k: st[k] for k in names}


# ---- clouds ------------------------------------------------------------------------

@add("cloud_nearest_device", outs=dict(index=4 * NPTS, dist=4 * NPTS), no_wait=True, has_stats=True,
     call=lambda eng, p, stream, stats: eng.cloud_nearest_device(p["q"], NPTS, 12, p["t"], 130, 12, 0.2, p["index"],
                                                                 p["dist"], stream=stream, stats=stats),
     ref=lambda I: (lambda r: (dict(index=r["index"], dist=r["dist"]), r["stats"], {}))(CR.nearest(I["q"], I["t"], 0.2)),
     counters=counts_of(CR.COUNTS))
def _(kind):
    return dict(q=cloud(100 + SEEDS[kind]), t=cloud(200 + SEEDS[kind], 130))


K = 5


@add("cloud_knn_device", outs=dict(index=4 * NPTS * K, dist=4 * NPTS * K, count=4 * NPTS), no_wait=True,
     has_stats=True,
     call=lambda eng, p, stream, stats: eng.cloud_knn_device(p["q"], NPTS, 12, p["t"], 130, 12, K, 0.3, p["index"],
                                                             p["dist"], p["count"], stream=stream, stats=stats),
     ref=lambda I: (lambda r: (dict(index=r["index"], dist=r["dist"], count=r["count"]), r["stats"], {}))(
         KR.knn(I["q"], I["t"], K, 0.3)),
     counters=counts_of(KR.KNN_COUNTS))
def _(kind):
    return dict(q=cloud(300 + SEEDS[kind]), t=cloud(400 + SEEDS[kind], 130))


def _clean_ref(I):
    r = KR.clean(I["points"], K, 0.3)
    return (dict(keep=r["keep"], mean_dist=r["mean_dist"], map=r["map"], out=r["points"],
                 n_out=np.int64([len(r["points"])])), r["stats"], {})


@add("cloud_clean_device", outs=dict(keep=NPTS, mean_dist=4 * NPTS, map=4 * NPTS, out=12 * NPTS, n_out=8),
     no_wait=True, has_stats=True,
     call=lambda eng, p, stream, stats: eng.cloud_clean_device(p["points"], NPTS, 12, K, 0.3, p["keep"], p["mean_dist"],
                                                               p["map"], p["out"], p["n_out"], stream=stream,
                                                               stats=stats),
     ref=_clean_ref, counters=counts_of(KR.CLEAN_COUNTS))
def _(kind):
    return dict(points=cloud(500 + SEEDS[kind]))


def _normals_ref(I):
    r = NR.normals(I["points"], 8, 0.3)
    return dict(normal=r["normal"], variation=r["variation"], count=r["count"]), r["stats"], {}


@add("cloud_normals_device", outs=dict(normal=12 * NPTS, variation=4 * NPTS, count=4 * NPTS), no_wait=True,
     has_stats=True,
     call=lambda eng, p, stream, stats: eng.cloud_normals_device(p["points"], NPTS, 12, 8, 0.3, p["normal"],
                                                                 p["variation"], p["count"], stream=stream,
                                                                 stats=stats),
     ref=_normals_ref, counters=counts_of(NR.COUNTS))
def _(kind):
    return dict(points=cloud(600 + SEEDS[kind]))


MATRIX = np.array([[0.0, -1.25, 0.0, 0.5], [1.25, 0.0, 0.0, -0.25], [0.0, 0.0, 1.25, 2.0]])


@add("cloud_transform_device", outs=dict(out=12 * NPTS), no_wait=True,
     call=lambda eng, p, stream, stats: eng.cloud_transform_device(p["points"], NPTS, 12, MATRIX, p["out"],
                                                                   stream=stream),
     ref=lambda I: (dict(out=AR.transform(I["points"], MATRIX)), None, {}))
def _(kind):
    return dict(points=cloud(700 + SEEDS[kind]))


ALIGN = dict(max_dist=0.5, iterations=4)


def _align_ref(I):
    r = AR.align(I["source"], I["target"], correspondences=True, **ALIGN)
    return (dict(index=r["index"], dist=r["dist"]), r["stats"],
            dict(matrix=r["matrix"].tobytes(), scale=r["scale"], trace=r["trace"].tobytes()))


@add("cloud_align_device", outs=dict(index=4 * NPTS, dist=4 * NPTS),
     call=lambda eng, p, stream, stats: eng.cloud_align_device(p["source"], NPTS, 12, p["target"], NPTS, 12,
                                                               d_index=p["index"], d_dist=p["dist"], stream=stream,
                                                               **ALIGN),
     ref=_align_ref,
     host=lambda r: dict(matrix=r["matrix"].tobytes(), scale=r["scale"], trace=r["trace"].tobytes()),
     counters=lambda r: {k: r["stats"][k] for k in AR.COUNTS})
def _(kind):
    t = cloud(800 + SEEDS[kind])
    shift = np.float32([0.02, -0.01, 0.015]) * np.float32(SEEDS[kind])
    return dict(source=(t[::-1] + shift).astype(np.float32), target=t)


# ---- meshes ------------------------------------------------------------------------

NV = NPTS


def mesh(kind):
    """257 vertex records under a fan (real; other: around vertex 256) or a strip (poison): 255
    triangles either way, every index inside 0 .. 256"""
    tris, nv = MS.strip(NV) if kind == "poison" else MS.fan(NV - 1)
    assert nv == NV and len(tris) == NV - 2
    if kind == "other":  # the fan around the last vertex
        tris = (NV - 1) - tris
    v = MC.random_vertices(NV, 900 + SEEDS[kind])
    a = 2 * np.pi * np.arange(NV) / NV
    rng = np.random.default_rng(950 + SEEDS[kind])
    pos = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)], 1) + 0.05 * rng.standard_normal((NV, 3))
    pos[0] = (0.0, 0.0, 0.3)
    v["pos"] = pos.astype(np.float32)
    return dict(vertices=v, triangles=np.ascontiguousarray(tris, np.int32))


NT = NV - 2


def clean_mesh(kind):
    """the mesh with triangles cut out so that it falls into components"""
    t = MS.strip(NV)[0].copy()
    cut = np.arange(NT) % (11 + SEEDS[kind]) < 2  # two triangles in a row made degenerate: the strip falls apart
    t[cut] = t[cut][:, [0, 0, 0]]
    return dict(vertices=mesh(kind)["vertices"], triangles=np.ascontiguousarray(t, np.int32))


def _components_ref(I):
    r = MC.components(I["triangles"], NV)
    return (dict(vertex_component=r["vertex_component"], triangle_component=r["triangle_component"],
                 components=r["components"]), r["stats"], dict(count=len(r["components"])))


@add("mesh_components_device", outs=dict(vertex_component=4 * NV, triangle_component=4 * NT, components=16 * NV),
     call=lambda eng, p, stream, stats: eng.mesh_components_device(p["triangles"], NT, NV, p["vertex_component"],
                                                                   p["triangle_component"], p["components"], NV,
                                                                   stream=stream),
     ref=_components_ref, host=lambda r: dict(count=r[0]), counters=lambda r: {k: r[1][k] for k in MC.COUNTS})
def _(kind):
    return dict(triangles=clean_mesh(kind)["triangles"])


CLEAN = dict(min_triangles=12)


def _mesh_clean_ref(I):
    r = MC.clean(I["vertices"], I["triangles"], **CLEAN)
    return (dict(vertices_out=r["vertices"], triangles_out=r["triangles"], vertex_map=r["vertex_map"],
                 triangle_map=r["triangle_map"]), r["stats"], dict(nv=len(r["vertices"]), nt=len(r["triangles"])))


@add("mesh_clean_device", outs=dict(vertices_out=16 * NV, triangles_out=12 * NT, vertex_map=4 * NV, triangle_map=4 * NT),
     call=lambda eng, p, stream, stats: eng.mesh_clean_device(p["vertices"], NV, p["triangles"], NT, p["vertices_out"], NV,
                                                              p["triangles_out"], NT, p["vertex_map"], p["triangle_map"],
                                                              stream=stream, **CLEAN),
     ref=_mesh_clean_ref, host=lambda r: dict(nv=r[0], nt=r[1]), counters=lambda r: {k: r[2][k] for k in MC.COUNTS})
def _(kind):
    return clean_mesh(kind)


ENTRIES = 6 * NT


def _adjacency_ref(I):
    r = MS.adjacency(I["triangles"], NV)
    return (dict(offsets=r["offsets"], neighbours=r["neighbours"], edge_triangles=r["edge_triangles"],
                 vertex_flags=r["vertex_flags"]), r["stats"], dict(entries=len(r["neighbours"])))


@add("mesh_adjacency_device", outs=dict(offsets=4 * (NV + 1), neighbours=4 * ENTRIES, edge_triangles=4 * ENTRIES,
                                        vertex_flags=NV),
     call=lambda eng, p, stream, stats: eng.mesh_adjacency_device(p["triangles"], NT, NV, p["offsets"], p["neighbours"],
                                                                  p["edge_triangles"], ENTRIES, p["vertex_flags"],
                                                                  stream=stream),
     ref=_adjacency_ref, host=lambda r: dict(entries=r[0]), counters=lambda r: {k: r[1][k] for k in MS.ADJ_COUNTS})
def _(kind):
    return dict(triangles=mesh(kind)["triangles"])


SMOOTH = dict(iterations=3, free_boundary=True)


@add("mesh_smooth_device", outs=dict(vertices_out=16 * NV), no_wait=True, has_stats=True,
     call=lambda eng, p, stream, stats: eng.mesh_smooth_device(p["vertices"], NV, p["triangles"], NT, p["vertices_out"],
                                                               stats=stats, stream=stream, **SMOOTH),
     ref=lambda I: (lambda r: (dict(vertices_out=r["vertices"]), r["stats"], {}))(
         MS.smooth(I["vertices"], I["triangles"], **SMOOTH)),
     counters=counts_of(MS.SMOOTH_COUNTS))
def _(kind):
    return mesh(kind)


@add("mesh_normals_device", outs=dict(normals=12 * NV), no_wait=True, has_stats=True,
     call=lambda eng, p, stream, stats: eng.mesh_normals_device(p["vertices"], NV, p["triangles"], NT, p["normals"],
                                                                stats=stats, stream=stream),
     ref=lambda I: (lambda r: (dict(normals=r["normals"]), r["stats"], {}))(MS.normals(I["vertices"], I["triangles"])),
     counters=counts_of(MS.NORMAL_COUNTS))
def _(kind):
    return mesh(kind)


DECIMATE = dict(cell=0.25, origin=(0.01, 0.02, 0.03))


def _decimate_ref(I):
    r = MD.decimate(I["vertices"], I["triangles"], **DECIMATE)
    return (dict(vertices_out=r["vertices"], triangles_out=r["triangles"], vertex_map=r["vertex_map"],
                 triangle_map=r["triangle_map"]), r["stats"], dict(nv=len(r["vertices"]), nt=len(r["triangles"])))


@add("mesh_decimate_device", outs=dict(vertices_out=16 * NV, triangles_out=12 * NT, vertex_map=4 * NV,
                                       triangle_map=4 * NT), has_stats=True,  # returns the counts: always one wait
     call=lambda eng, p, stream, stats: eng.mesh_decimate_device(p["vertices"], NV, p["triangles"], NT, p["vertices_out"],
                                                                 NV, p["triangles_out"], NT, d_vertex_map=p["vertex_map"],
                                                                 d_triangle_map=p["triangle_map"], stats=stats,
                                                                 stream=stream, **DECIMATE),
     ref=_decimate_ref, host=lambda r: dict(nv=r[0], nt=r[1]), counters=lambda r: {k: r[2][k] for k in MD.COUNTS})
def _(kind):
    return mesh(kind)


def _mesh_nearest_ref(I):
    r = MN.nearest(I["q"], I["vertices"], I["triangles"], 0.3)
    return dict(index=r["index"], dist=r["dist"]), {k: r["stats"][k] for k in MN.COUNTS}, {}


@add("mesh_nearest_device", outs=dict(index=4 * NPTS, dist=4 * NPTS), no_wait=True, has_stats=True,
     call=lambda eng, p, stream, stats: eng.mesh_nearest_device(p["q"], NPTS, 12, p["vertices"], NV, p["triangles"], NT,
                                                                0.3, p["index"], p["dist"], stream=stream, stats=stats),
     ref=_mesh_nearest_ref, counters=counts_of(MN.COUNTS))
def _(kind):
    return dict(q=cloud(1000 + SEEDS[kind], scale=2.0, shift=-1.0), **mesh(kind))


# ---- the TSDF mesh: an analytic sphere volume ---------------------------------------

DIM = 8
VOLUME = dict(origin=(-0.4, -0.4, -0.4), voxel=0.1, dim=(DIM, DIM, DIM), trunc=0.4)
VCAP, TCAP = 1024, 2048


def _tsdf_mesh_ref(I):
    r = TR.mesh(I["tsdf"], I["weight"], I["rgb"], origin=VOLUME["origin"], voxel=VOLUME["voxel"], dim=VOLUME["dim"])
    assert len(r["vertices"]) <= VCAP and len(r["triangles"]) <= TCAP
    return (dict(vertices=r["vertices"], triangles=r["triangles"]), r["stats"],
            dict(nv=len(r["vertices"]), nt=len(r["triangles"])))


@add("tsdf_mesh_device", outs=dict(vertices=16 * VCAP, triangles=12 * TCAP),
     call=lambda eng, p, stream, stats: eng.tsdf_mesh_device(p["tsdf"], p["weight"], p["rgb"], p["vertices"], VCAP,
                                                             p["triangles"], TCAP, stream=stream, **VOLUME),
     ref=_tsdf_mesh_ref, host=lambda r: dict(nv=r[0], nt=r[1]),
     counters=lambda r: {k: r[2][k] for k in ("active_cells", "vertices", "triangles")})
def _(kind):
    s = SEEDS[kind]
    vol, _ = MS.sphere_volume(DIM, radius=0.2 + 0.03 * s, centre=(0.013 * s, -0.021, 0.008))
    rng = np.random.default_rng(1100 + s)
    return dict(tsdf=vol["tsdf"], weight=vol["weight"], rgb=rng.integers(0, 1 << 24, (DIM,) * 3).astype(np.uint32))


# ---- the forms that need views: 3 views of 70 x 50 ----------------------------------
# Their expected result is their own run on the default stream after a full
# synchronize, which their own tests pin to the oracle or to the reference.

NPAT = 48


@functools.lru_cache(None)
def scene():
    cfg = synth.config(3, 70, 50, 1, seed_stride_px=6.0)
    P, imgs, seeds = synth.scene_host(cfg)
    return dict(P=P, imgs=imgs, seeds=seeds, views=[dp.View(P[v], imgs[v]) for v in range(3)],
                sizes=[(70, 50)] * 3)


@functools.lru_cache(None)
def seed_patches(kind, n=NPAT):
    """n unrefined seed patches of the scene by the oracle (no GPU): other seeds per kind"""
    from oracle import pyoracle as orc

    sc = scene()
    at = {"real": 0, "poison": 1, "other": 2}[kind]
    s = sc["seeds"]
    # the scene has fewer seeds than a block: they repeat with a jitter on the surface's scale
    jitter = np.random.default_rng(1400 + at).standard_normal((n, 3)) * 2e-3 * float((s.max(axis=0) - s.min(axis=0)).max())
    seeds = np.ascontiguousarray(s[(3 * np.arange(n) + at) % len(s)] + jitter)
    return orc.Scene(sc["P"], sc["imgs"]).seeds_to_patches(seeds)


def _patches(kind):
    return dict(patches=seed_patches(kind))


CASES["refine_device"] = Case(
    "refine_device", _patches, dict(accept=NPAT), views=True, no_wait=True, inout=("patches",),
    call=lambda eng, p, stream, stats: eng.refine_device(p["patches"], NPAT, 11, N.MODE_EXPAND, p["accept"], stream))
CASES["expand_device"] = Case(
    "expand_device", _patches, dict(children=4 * NPAT * PATCH.itemsize, accept=4 * NPAT), views=True, no_wait=True,
    call=lambda eng, p, stream, stats: eng.expand_device(p["patches"], NPAT, p["children"], p["accept"], stream))
CASES["fast_expand_device"] = Case(
    "fast_expand_device", _patches, dict(children=4 * NPAT * PATCH.itemsize, accept=4 * NPAT), views=True, no_wait=True,
    setup=lambda eng: eng.set_fast_options(dp.FastOptions()),
    call=lambda eng, p, stream, stats: eng.fast_expand_device(p["patches"], NPAT, p["children"], p["accept"], stream))


def _keep(kind, n):
    return (np.random.default_rng(1200 + SEEDS[kind]).random(n) < 0.7).astype(np.uint8)


NF = NPTS
CASES["filter_patches_device"] = Case(
    "filter_patches_device", lambda kind: dict(patches=seed_patches(kind, NF)), dict(keep=NF), views=True, no_wait=True,
    call=lambda eng, p, stream, stats: eng.filter_patches_device(p["patches"], NF, p["keep"], 3, stream=stream))


def _gen(g):
    return dict(items=g.items, head=g.head, per_item=g.per_item, cell=g.cell, index=g.index)


CASES["densify_resume_device"] = Case(
    "densify_resume_device", lambda kind: dict(patches=seed_patches(kind, NF), keep=_keep(kind, NF)), {}, views=True,
    call=lambda eng, p, stream, stats: eng.densify_resume_device(p["patches"], NF, p["keep"], stream),
    host=lambda g: _gen(g), store=True)

PX = 70 * 50
VIEWS = [0, 1, 2]


def _planes(p, key):
    return [p["%s%d" % (key, v)] for v in VIEWS]


def _plane_outs(**words):
    return {"%s%d" % (key, v): 4 * w * PX for key, w in words.items() for v in VIEWS}


CASES["render_maps_device"] = Case(
    "render_maps_device", lambda kind: dict(patches=seed_patches(kind, NF), keep=_keep(kind, NF)),
    _plane_outs(depth=1, index=1, normal=3, score=1), views=True, no_wait=True, has_stats=True,
    call=lambda eng, p, stream, stats: eng.render_maps_device(
        p["patches"], NF, p["keep"], VIEWS, _planes(p, "depth"), _planes(p, "index"), _planes(p, "normal"),
        _planes(p, "score"), splat_scale=2.0, stream=stream, stats=stats),
    counters=lambda st: {k: v for k, v in st.items() if not k.endswith("_ms")})


def rendered(kind, eng):
    """the depth and normal planes of the kind's seed patches: rendered by the
    engine (render_maps, pinned by its own tests), so made in the GPU test"""
    m = eng.render_maps(seed_patches(kind, NF), normals=True, splat_scale=2.0)
    out = {}
    for v in VIEWS:
        out["depth%d" % v], out["normal%d" % v] = m["depth"][v], m["normal"][v]
    return out


def _no_ms(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


FCAP = 3 * PX
CASES["fuse_maps_device"] = Case(
    "fuse_maps_device", rendered, dict(points=FCAP * dp.pmvs.FUSED_DTYPE.itemsize), views=True, gpu_inputs=True,
    call=lambda eng, p, stream, stats: eng.fuse_maps_device(VIEWS, _planes(p, "depth"), _planes(p, "normal"), p["points"],
                                                            FCAP, stream=stream),
    host=lambda r: dict(n=r[0]), counters=lambda r: _no_ms(r[1]))
CASES["refine_maps_device"] = Case(
    "refine_maps_device", rendered, _plane_outs(odepth=1, onormal=3, oscore=1, ochoice=1), views=True, gpu_inputs=True,
    no_wait=True, has_stats=True,
    call=lambda eng, p, stream, stats: eng.refine_maps_device(
        VIEWS, _planes(p, "depth"), _planes(p, "normal"), _planes(p, "odepth"), _planes(p, "onormal"),
        _planes(p, "oscore"), _planes(p, "ochoice"), stream=stream, stats=stats, window=3, sweep=1, reach=(2, 0)),
    counters=_no_ms)

TDIM = (12, 11, 10)
TVOL = 4 * TDIM[0] * TDIM[1] * TDIM[2]


def tsdf_box(eng):
    """a volume around the scene's seeds"""
    s = scene()["seeds"]
    lo, hi = s.min(axis=0), s.max(axis=0)
    voxel = float((hi - lo).max() / 9.0)
    return dict(origin=tuple(float(x) for x in lo - voxel), voxel=voxel, dim=TDIM, trunc=3.0 * voxel)


CASES["tsdf_integrate_device"] = Case(
    "tsdf_integrate_device", lambda kind, eng: {k: v for k, v in rendered(kind, eng).items() if k.startswith("depth")},
    dict(tsdf=TVOL, weight=TVOL, rgb=TVOL), views=True, gpu_inputs=True, no_wait=True, has_stats=True,
    call=lambda eng, p, stream, stats: eng.tsdf_integrate_device(VIEWS, _planes(p, "depth"), p["tsdf"], p["weight"],
                                                                 p["rgb"], stream=stream, stats=stats, **tsdf_box(eng)),
    counters=_no_ms)


def view_mesh(kind):
    """a 16 x 16 sheet (plus one unused vertex: 257) through the scene's seeds"""
    s = scene()["seeds"]
    c, span = s.mean(axis=0), (s.max(axis=0) - s.min(axis=0))
    tris, nv = MS.grid_sheet(16)
    v = MC.random_vertices(NV, 1300 + SEEDS[kind])
    rng = np.random.default_rng(1350 + SEEDS[kind])
    y, x = np.mgrid[0:16, 0:16]
    pos = np.zeros((NV, 3))
    pos[:256, 0] = c[0] + (x.ravel() / 15.0 - 0.5) * span[0]
    pos[:256, 1] = c[1] + (y.ravel() / 15.0 - 0.5) * span[1]
    pos[:256, 2] = c[2]
    pos[256] = c
    pos += 0.02 * span.max() * rng.standard_normal((NV, 3))
    v["pos"] = pos.astype(np.float32)
    if kind == "poison":
        tris = tris[::-1][:, [0, 2, 1]]
    return dict(vertices=v, triangles=np.ascontiguousarray(tris, np.int32))


VT = 2 * 15 * 15
CASES["mesh_render_device"] = Case(
    "mesh_render_device", view_mesh, _plane_outs(depth=1, index=1, normal=3), views=True, no_wait=True, has_stats=True,
    call=lambda eng, p, stream, stats: eng.mesh_render_device(p["vertices"], NV, p["triangles"], VT, VIEWS,
                                                              _planes(p, "depth"), _planes(p, "index"),
                                                              _planes(p, "normal"), stream=stream, stats=stats),
    counters=_no_ms)


def colour_inputs(kind, eng):
    m = view_mesh(kind)
    depth = eng.mesh_render(m["vertices"], m["triangles"], views=VIEWS)["depth"]
    out = dict(vertices=m["vertices"])
    for v in VIEWS:
        out["depth%d" % v] = depth[v]
    return out


CASES["mesh_colour_device"] = Case(
    "mesh_colour_device", colour_inputs, dict(vertices_out=16 * NV, seen=8 * NV, best=4 * NV), views=True,
    gpu_inputs=True, no_wait=True, has_stats=True,
    call=lambda eng, p, stream, stats: eng.mesh_colour_device(p["vertices"], NV, VIEWS, _planes(p, "depth"),
                                                              p["vertices_out"], None, p["seen"], p["best"],
                                                              stream=stream, stats=stats),
    counters=_no_ms)

for _c in CASES.values():
    _c.__dict__.setdefault("gpu_inputs", False)
    _c.__dict__.setdefault("store", False)


def stream_methods():
    """the public Engine methods whose signature has a `stream` parameter"""
    import inspect

    return sorted(name for name, fn in inspect.getmembers(dp.Engine, inspect.isfunction)
                  if not name.startswith("_") and "stream" in inspect.signature(fn).parameters)
