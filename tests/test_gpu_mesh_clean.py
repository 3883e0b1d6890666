"""dp_mesh_components and dp_mesh_clean on the GPU against the CPU reference
(tests/mesh_ref.py, restated from the header's spec): every byte of the labels,
the table, the kept vertices and triangles and the maps, the counts and the
integer statistics, in the host and the device form."""
import json
import os

import numpy as np
import pytest

import densepoints_amd as dp
from densepoints_amd import MESH_COMPONENT_DTYPE, MESH_VERTEX_DTYPE
from densepoints_amd import _native as N

import mesh_ref as MR
import tsdf_ref as TR
from test_gpu_iterate import to_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FORMS = ["host", "device"]


@pytest.fixture(scope="module")
def eng():
    # no views are set: neither call reads one
    with dp.Engine(device=0) as e:
        yield e


def counts(stats):
    return {c: stats[c] for c in MR.COUNTS}


def device_buffer(records, size):
    import torch

    return torch.full(((records + 3) * size,), SENTINEL, dtype=torch.uint8, device="cuda")


def components(eng, form, tris, nv, ccap=None):
    """mesh_components in either form: the host form's dict, and for the device
    form also the whole sentinel-filled table buffer"""
    tris = MR.as_triangles(tris)
    if form == "host":
        return eng.mesh_components(tris, nv)
    import torch

    nt = len(tris)
    ccap = nv if ccap is None else ccap
    dt = to_device(tris) if nt else None
    vc, tc, cb = device_buffer(nv, 4), device_buffer(nt, 4), device_buffer(ccap, 16)
    torch.cuda.synchronize()
    nc, st = eng.mesh_components_device(dt.data_ptr() if nt else None, nt, nv, vc.data_ptr(), tc.data_ptr(),
                                        cb.data_ptr() if ccap else None, ccap)
    vraw, traw, craw = vc.cpu().numpy(), tc.cpu().numpy(), cb.cpu().numpy()
    assert (vraw[nv * 4:] == SENTINEL).all() and (traw[nt * 4:] == SENTINEL).all()
    assert (craw[min(nc, ccap) * 16:] == SENTINEL).all()
    return dict(vertex_component=vraw[:nv * 4].view(np.int32).copy(), triangle_component=traw[:nt * 4].view(np.int32).copy(),
                components=craw[:min(nc, ccap) * 16].view(MESH_COMPONENT_DTYPE).copy(), stats=st, n_components=nc)


def clean(eng, form, verts, tris, vcap=None, tcap=None, maps=True, **opts):
    """mesh_clean in either form: dict(vertices, triangles, vertex_map,
    triangle_map, stats, counts = the counts the call returned)"""
    verts, tris = np.ascontiguousarray(verts, dtype=MESH_VERTEX_DTYPE), MR.as_triangles(tris)
    nv, nt = len(verts), len(tris)
    if form == "host":
        vo, to, st, vm, tm = eng.mesh_clean(verts, tris, maps=True, **opts)
        return dict(vertices=vo, triangles=to, vertex_map=vm, triangle_map=tm, stats=st, counts=(len(vo), len(to)))
    import torch

    vcap = nv if vcap is None else vcap
    tcap = nt if tcap is None else tcap
    dv, dt = (to_device(verts) if nv else None), (to_device(tris) if nt else None)
    vb, tb = device_buffer(vcap, 16), device_buffer(tcap, 12)
    vm, tm = device_buffer(nv, 4), device_buffer(nt, 4)
    torch.cuda.synchronize()
    no, to, st = eng.mesh_clean_device(dv.data_ptr() if nv else None, nv, dt.data_ptr() if nt else None, nt,
                                       vb.data_ptr() if vcap else None, vcap, tb.data_ptr() if tcap else None, tcap,
                                       vm.data_ptr() if maps else None, tm.data_ptr() if maps else None, **opts)
    vraw, traw, vmraw, tmraw = vb.cpu().numpy(), tb.cpu().numpy(), vm.cpu().numpy(), tm.cpu().numpy()
    # nothing beyond min(cap, count) records, nothing beyond the maps
    assert (vraw[min(no, vcap) * 16:] == SENTINEL).all() and (traw[min(to, tcap) * 12:] == SENTINEL).all()
    assert (vmraw[(nv if maps else 0) * 4:] == SENTINEL).all() and (tmraw[(nt if maps else 0) * 4:] == SENTINEL).all()
    return dict(vertices=vraw[:min(no, vcap) * 16].view(MESH_VERTEX_DTYPE).copy(),
                triangles=traw[:min(to, tcap) * 12].view(np.int32).reshape(-1, 3).copy(),
                vertex_map=vmraw[:nv * 4].view(np.int32).copy(), triangle_map=tmraw[:nt * 4].view(np.int32).copy(),
                stats=st, counts=(no, to))


def assert_components(got, want):
    assert counts(got["stats"]) == want["stats"]
    assert got["vertex_component"].dtype == np.int32 and got["components"].dtype == MESH_COMPONENT_DTYPE
    assert got["vertex_component"].tobytes() == want["vertex_component"].tobytes()
    assert got["triangle_component"].tobytes() == want["triangle_component"].tobytes()
    assert got["components"].tobytes() == want["components"].tobytes()


def assert_clean(got, want, maps=True):
    assert counts(got["stats"]) == want["stats"]
    assert got["counts"] == (want["stats"]["vertices_out"], want["stats"]["triangles_out"])
    assert got["vertices"].tobytes() == want["vertices"].tobytes()
    assert got["triangles"].tobytes() == want["triangles"].tobytes()
    if maps:
        assert got["vertex_map"].tobytes() == want["vertex_map"].tobytes()
        assert got["triangle_map"].tobytes() == want["triangle_map"].tobytes()


def check_both(eng, form, verts, tris, **opts):
    want_c, want = MR.components(tris, len(verts)), MR.clean(verts, tris, **opts)
    assert_components(components(eng, form, tris, len(verts)), want_c)
    got = clean(eng, form, verts, tris, **opts)
    assert_clean(got, want)
    return got, want


@pytest.mark.parametrize("form", FORMS)
def test_hand_mesh(eng, form):
    """two disjoint triangles, a bow-tie, repeated indices, a triangle whose root
    is not its first index, unused vertices at the start, in the middle and at
    the end, and invalid triangles (indices -1 and n_vertices only)"""
    tris, nv = MR.hand_mesh()
    verts = MR.random_vertices(nv, 11)
    got, want = check_both(eng, form, verts, tris)
    assert want["stats"]["invalid_triangles"] == 5 and want["stats"]["components"] == 4
    assert got["stats"]["clean_ms"] > 0
    for opts in (dict(max_components=2), dict(min_triangles=2), dict(min_fraction=1.0), dict(min_triangles=0)):
        check_both(eng, form, verts, tris, **opts)


@pytest.fixture(scope="module")
def deep():
    tris, nv = MR.deep_mesh()
    verts = MR.random_vertices(nv, 12)
    return tris, verts, MR.components(tris, nv), {k: MR.clean(verts, tris, max_components=k) for k in (0, 1)}


@pytest.mark.parametrize("form", FORMS)
def test_deep_component(eng, deep, form):
    """a strip of 5,000 triangles under a random permutation among 3,000 single
    triangles: long find paths, compare-and-swap retries, the wave-aggregated
    counts, and 3,001 components (no multiple of a block)"""
    tris, verts, want_c, want = deep
    assert want_c["stats"]["components"] == 3001 and want_c["stats"]["largest_triangles"] == 5000
    assert_components(components(eng, form, tris, len(verts)), want_c)
    for k in (0, 1):
        assert_clean(clean(eng, form, verts, tris, max_components=k), want[k])
    assert want[1]["stats"]["triangles_out"] == 5000 and want[1]["stats"]["vertices_out"] == 5002


def edge_mesh(nv, nt, seed):
    """nt random triangles over nv vertices, some sharing vertices, some with an
    index of -1 or nv"""
    rng = np.random.default_rng(seed)
    tris = rng.integers(0, max(nv, 1), size=(nt, 3)).astype(np.int32)
    if nv == 0:
        tris[:] = 0  # every index is n_vertices: all invalid
    bad = rng.random(nt) < 0.1
    tris[bad, rng.integers(0, 3, size=int(bad.sum()))] = rng.choice([-1, nv], size=int(bad.sum()))
    return tris


@pytest.mark.parametrize("form", FORMS)
def test_block_and_wave_edges(eng, form):
    sizes = (1, 63, 64, 65, 255, 256, 257)
    for nv in sizes:
        verts = MR.random_vertices(nv, 100 + nv)
        for nt in sizes:
            check_both(eng, form, verts, edge_mesh(nv, nt, 1000 * nv + nt), max_components=3)
    # sparse: many components, so the numbering crosses blocks
    tris = (3 * np.arange(85, dtype=np.int32))[:, None] + np.arange(3, dtype=np.int32)[None, :]
    check_both(eng, form, MR.random_vertices(257, 3), tris, max_components=70)


@pytest.mark.parametrize("form", FORMS)
def test_empty_inputs(eng, form):
    for nv, nt in ((0, 0), (5, 0), (0, 4)):
        got, want = check_both(eng, form, MR.random_vertices(nv, 4), edge_mesh(nv, nt, 5))
        assert got["counts"] == (0, 0) and want["stats"]["components"] == 0
        assert want["stats"]["invalid_triangles"] == nt and want["stats"]["unused_vertices"] == nv


def fans(sizes):
    tris, base = [], 0
    for n in sizes:
        tris += [(base, base + 1 + i, base + 2 + i) for i in range(n)]
        base += n + 2
    return np.array(tris, np.int32), base


@pytest.mark.parametrize("form", FORMS)
def test_selection(eng, form):
    tris, nv = fans((4, 8, 4, 1, 4))
    verts = MR.random_vertices(nv, 6)
    # ties in T_c with max_components cutting inside the tie: the lower number wins
    for k, kept in ((1, [1]), (2, [0, 1]), (3, [0, 1, 2]), (4, [0, 1, 2, 4])):
        got, want = check_both(eng, form, verts, tris, max_components=k)
        assert np.flatnonzero(want["kept"]).tolist() == kept
    # T = 4 against Tmax = 8 at min_fraction 0.5: kept, the comparison is >=
    got, want = check_both(eng, form, verts, tris, min_fraction=0.5)
    assert want["kept"].tolist() == [True, True, True, False, True]
    check_both(eng, form, verts, tris, min_triangles=0)
    check_both(eng, form, verts, tris, min_triangles=8)
    got, want = check_both(eng, form, verts, tris, min_triangles=9)  # Tmax + 1
    assert got["counts"] == (0, 0) and len(got["vertices"]) == 0 and got["triangles"].shape == (0, 3)
    assert (got["vertex_map"] == -1).all() and (got["triangle_map"] == -1).all()
    if form == "host":  # an empty result is NULL pointers and zero counts
        ct = N.ctypes
        o = dp.check_mesh_clean_args(min_triangles=9)
        pv, pt, no, to = ct.c_void_p(1), ct.c_void_p(1), ct.c_int64(-1), ct.c_int64(-1)
        assert N.lib.dp_mesh_clean(eng.handle, ct.byref(o), N.ptr(verts), nv, N.ptr(tris), len(tris), ct.byref(pv),
                                   ct.byref(no), ct.byref(pt), ct.byref(to), None, None, None) == N.DP_OK
        assert (pv.value, pt.value, no.value, to.value) == (None, None, 0, 0)


def test_caps(eng, deep):
    tris, verts, want_c, wants = deep
    want = wants[0]
    nvo, nto, C = want["stats"]["vertices_out"], want["stats"]["triangles_out"], want_c["stats"]["components"]
    for vcap, tcap in ((nvo - 1, nto - 1), (1000, 3), (1, nto), (nvo, 1)):
        got = clean(eng, "device", verts, tris, vcap=vcap, tcap=tcap)
        assert got["counts"] == (nvo, nto) and counts(got["stats"]) == want["stats"]
        assert got["vertices"].tobytes() == want["vertices"][:vcap].tobytes()
        assert got["triangles"].tobytes() == want["triangles"][:tcap].tobytes()
        assert got["vertex_map"].tobytes() == want["vertex_map"].tobytes()
    # caps of 0 with no buffers and no maps: the counts only
    got = clean(eng, "device", verts, tris, vcap=0, tcap=0, maps=False)
    assert got["counts"] == (nvo, nto) and len(got["vertices"]) == 0 and len(got["triangles"]) == 0
    for ccap in (C - 1, 1, 0):
        got = components(eng, "device", tris, len(verts), ccap=ccap)
        assert got["n_components"] == C and counts(got["stats"]) == want_c["stats"]
        assert got["components"].tobytes() == want_c["components"][:ccap].tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_idempotence(eng, deep, form):
    tris, verts = deep[0], deep[1]
    for opts in (dict(min_triangles=2), dict(max_components=40), dict()):
        once = clean(eng, form, verts, tris, **opts)
        again = clean(eng, form, once["vertices"], once["triangles"], **opts)
        assert again["vertices"].tobytes() == once["vertices"].tobytes()
        assert again["triangles"].tobytes() == once["triangles"].tobytes()
        assert again["counts"] == once["counts"]


def test_volume_end_to_end_on_the_device(eng):
    """the sphere volume with six planted blobs: dp_tsdf_mesh_device, then
    dp_mesh_clean_device with max_components = 1 on its output where it lies, is
    dp_tsdf_mesh of the sphere alone, byte for byte"""
    import torch

    sphere, planted, weight = MR.blob_volumes()
    vol = MR.BLOB_VOLUME
    want_v, want_t, _ = eng.tsdf_mesh(dict(vol, tsdf=sphere, weight=weight, rgb=None))
    assert (len(want_v), len(want_t)) == MR.SPHERE_COUNTS
    d_tsdf, d_weight = to_device(planted), to_device(weight)
    vcap, tcap = 4000, 8000
    vb, tb = device_buffer(vcap, 16), device_buffer(tcap, 12)
    torch.cuda.synchronize()
    nv, nt, _ = eng.tsdf_mesh_device(d_tsdf.data_ptr(), d_weight.data_ptr(), None, vb.data_ptr(), vcap, tb.data_ptr(),
                                     tcap, **vol)
    assert nt == sum(MR.BLOB_TRIANGLES) and nv <= vcap
    tc, cb = device_buffer(nt, 4), device_buffer(16, 16)
    torch.cuda.synchronize()
    nc, st = eng.mesh_components_device(tb.data_ptr(), nt, nv, None, tc.data_ptr(), cb.data_ptr(), 16)
    table = cb.cpu().numpy()[:nc * 16].view(MESH_COMPONENT_DTYPE)
    assert nc == 7 and tuple(sorted(table["triangles"].tolist(), reverse=True)) == MR.BLOB_TRIANGLES
    assert st["invalid_triangles"] == 0 and st["unused_vertices"] == 0
    vo, to = device_buffer(vcap, 16), device_buffer(tcap, 12)
    torch.cuda.synchronize()
    no, nto, st = eng.mesh_clean_device(vb.data_ptr(), nv, tb.data_ptr(), nt, vo.data_ptr(), vcap, to.data_ptr(), tcap,
                                        max_components=1)
    assert (no, nto) == MR.SPHERE_COUNTS and st["components"] == 7 and st["components_kept"] == 1
    assert vo.cpu().numpy()[:no * 16].tobytes() == want_v.tobytes()
    assert to.cpu().numpy()[:nto * 12].tobytes() == want_t.tobytes()
    # the equal sizes are the tie cases of max_components = 2 and 4
    full_v = vb.cpu().numpy()[:nv * 16].view(MESH_VERTEX_DTYPE)
    full_t = tb.cpu().numpy()[:nt * 12].view(np.int32).reshape(-1, 3)
    for k in (2, 4):
        want = MR.clean(full_v, full_t, max_components=k)
        assert_clean(clean(eng, "device", full_v, full_t, max_components=k), want)
        assert want["stats"]["components_kept"] == k


def test_errors():
    ct, lib = N.ctypes, N.lib
    tris, nv = MR.hand_mesh()
    nt = len(tris)
    verts = MR.random_vertices(nv, 7)
    vc, tc, vm, tm = np.zeros(nv, np.int32), np.zeros(nt, np.int32), np.zeros(nv, np.int32), np.zeros(nt, np.int32)
    pc, nc, pv, pt, no, to = ct.c_void_p(), ct.c_int64(), ct.c_void_p(), ct.c_void_p(), ct.c_int64(), ct.c_int64()
    with dp.Engine(device=0) as e:  # a context with no views set is accepted
        h = e.handle

        def comp(t=tris, n_t=nt, n_v=nv, v_c=vc, t_c=tc, table=True, count=True):
            return lib.dp_mesh_components(h, N.ptr(t) if t is not None else None, n_t, n_v,
                                          v_c.ctypes.data if v_c is not None else None,
                                          t_c.ctypes.data if t_c is not None else None,
                                          ct.byref(pc) if table else None, ct.byref(nc) if count else None, None)

        def cln(o=None, v=verts, n_v=nv, t=tris, n_t=nt, v_m=None, t_m=None, results=True, nvo=True, nto=True):
            return lib.dp_mesh_clean(h, ct.byref(o) if o is not None else None, N.ptr(v) if v is not None else None, n_v,
                                     N.ptr(t) if t is not None else None, n_t, ct.byref(pv) if results else None,
                                     ct.byref(no) if nvo else None, ct.byref(pt), ct.byref(to) if nto else None,
                                     v_m, t_m, None)

        def bad(rc):
            assert rc == N.DP_E_ARG and lib.dp_last_error(h)

        assert comp() == N.DP_OK and nc.value == 4 and cln() == N.DP_OK
        assert comp(v_c=None, t_c=None) == N.DP_OK and cln(v_m=vm.ctypes.data, t_m=tm.ctypes.data) == N.DP_OK
        # counts: negative, above 2^31 - 1; a NULL input with a non-zero count
        for kw in (dict(n_t=-1), dict(n_v=-1), dict(n_t=2**31), dict(n_v=2**31), dict(t=None)):
            bad(comp(**kw))
            bad(cln(**kw))
        bad(cln(v=None))
        assert comp(t=None, n_t=0) == N.DP_OK and cln(v=None, n_v=0) == N.DP_OK
        # options
        for kw in (dict(min_triangles=-1), dict(min_fraction=-0.5), dict(min_fraction=1.5),
                   dict(min_fraction=float("nan")), dict(max_components=-1), dict(flags=1)):
            o = N.DpMeshCleanOptions(1, 0.0, 0, 0, 0)
            for key, value in kw.items():
                setattr(o, key, value)
            bad(cln(o))
        # a NULL count or result pointer
        bad(comp(count=False))
        bad(comp(table=False))
        bad(cln(nvo=False))
        bad(cln(nto=False))
        bad(cln(results=False))
        # an output that is an input
        bad(comp(t_c=tris))
        bad(cln(v_m=verts.ctypes.data))
        bad(cln(t_m=tris.ctypes.data))
        # the device form: caps, counts, aliases
        import torch

        dv, dt = to_device(verts), to_device(tris)
        buf = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def cdev(vb, vcap, tb, tcap, nvo=True, o=None, vmap=None):
            return lib.dp_mesh_clean_device(h, ct.byref(o) if o is not None else None, dv.data_ptr(), nv, dt.data_ptr(),
                                            nt, vb, vcap, ct.byref(no) if nvo else None, tb, tcap, ct.byref(to), vmap,
                                            None, None, None)

        def kdev(cb, ccap, count=True, tcomp=None):
            return lib.dp_mesh_components_device(h, dt.data_ptr(), nt, nv, None, tcomp, cb, ccap,
                                                 ct.byref(nc) if count else None, None, None)

        assert cdev(buf.data_ptr(), 16, buf.data_ptr() + 512, 16) == N.DP_OK and (no.value, to.value) == (13, 7)
        assert cdev(None, 0, None, 0) == N.DP_OK and kdev(buf.data_ptr(), 4) == N.DP_OK and kdev(None, 0) == N.DP_OK
        for args in ((buf.data_ptr(), -1, buf.data_ptr(), 4), (buf.data_ptr(), 4, buf.data_ptr(), -1),
                     (None, 4, buf.data_ptr(), 4), (buf.data_ptr(), 4, None, 4)):
            bad(cdev(*args))
        bad(cdev(buf.data_ptr(), 4, buf.data_ptr(), 4, nvo=False))
        bad(cdev(dv.data_ptr(), 4, buf.data_ptr(), 4))
        bad(cdev(buf.data_ptr(), 4, dt.data_ptr(), 4))
        bad(cdev(buf.data_ptr(), 4, buf.data_ptr(), 4, vmap=dv.data_ptr()))
        bad(cdev(buf.data_ptr(), 4, buf.data_ptr(), 4, o=N.DpMeshCleanOptions(1, 0.0, 0, 2, 0)))
        bad(kdev(buf.data_ptr(), -1))
        bad(kdev(None, 3))
        bad(kdev(buf.data_ptr(), 4, count=False))
        bad(kdev(buf.data_ptr(), 4, tcomp=dt.data_ptr()))
        # the Python mirror refuses before any device call
        for kw in (dict(min_triangles=-1), dict(min_fraction=2.0), dict(max_components=-1)):
            with pytest.raises(ValueError):
                e.mesh_clean(verts, tris, **kw)
        with pytest.raises(ValueError):
            e.mesh_components(np.zeros((2, 4), np.int32), 4)
        with pytest.raises(ValueError):
            e.mesh_clean_device(dv.data_ptr(), nv, dt.data_ptr(), nt, None, 4, None, 0)


def test_cli_mesh_clean(tmp_path):
    """densify --mesh with --mesh-keep-largest 1: the PLY's counts equal the
    report's, the clean-up saw the mesh a run without the flag writes, and a run
    without the flags writes what it always wrote"""
    from test_cli import run
    from test_tsdf_cpu import parse_ply

    d = str(tmp_path / "scene")
    run("--synthetic", "4,160,120,1", "--write-scene", d)
    ply, plain, cleaned = tmp_path / "points.ply", tmp_path / "plain.ply", tmp_path / "clean.ply"
    base = ("-i", os.path.join(d, "scene.json"), "--seeds", os.path.join(d, "seeds.xyz"), "-o", str(ply), "--mesh-dim",
            "40")
    r0 = json.loads(run(*base, "--mesh", str(plain)).stdout)
    v0, f0 = parse_ply(str(plain))
    assert r0["mesh"]["vertices"] == len(v0) > 0 and r0["mesh"]["triangles"] == len(f0) > 0
    # no flag: the report has the members it had before the clean-up existed
    assert list(r0["mesh"]) == ["vertices", "triangles", "ms", "dim", "voxel", "trunc", "observed_voxels",
                                "active_cells", "integrate_ms", "mesh_ms"]
    r1 = json.loads(run(*base, "--mesh", str(cleaned), "--mesh-keep-largest", "1").stdout)
    v1, f1 = parse_ply(str(cleaned))
    m, c = r1["mesh"], r1["mesh"]["clean"]
    assert m["vertices"] == len(v1) > 0 and m["triangles"] == len(f1) > 0
    assert c["triangles_in"] == len(f0) and c["vertices_in"] == len(v0) and c["components_kept"] == 1
    assert (c["vertices_out"], c["triangles_out"]) == (len(v1), len(f1)) and c["largest_triangles"] == len(f1)
    assert f1[:, 1:].max() == len(v1) - 1
    # the written mesh is the reference's clean of the plain one
    want = MR.components(f0[:, 1:], len(v0))
    assert c["components"] == want["stats"]["components"]
    assert len(f1) == int(want["components"]["triangles"].max())
    # a second run without the flags: the same bytes
    again = tmp_path / "again.ply"
    run(*base, "--mesh", str(again))
    assert again.read_bytes() == plain.read_bytes()
    for badv in (("--mesh-min-component", "-1"), ("--mesh-min-component-frac", "1.5"), ("--mesh-keep-largest", "0"),
                 ("--mesh-keep-largest", "x")):
        r = run("-i", os.path.join(d, "scene.json"), "--mesh", str(cleaned), *badv, check=False)
        assert r.returncode == 2 and "expects" in r.stderr


def test_pmvs_mesh_clean():
    """PMVS.mesh(clean=...) is mesh_ref's clean of PMVS.mesh()"""
    from test_gpu_parity import scene

    sc = scene("hf6")
    pm = dp.PMVS()
    for v in sc.views:
        pm.add_camera(v)
    assert pm.run(sc.seeds)
    verts, tris = pm.mesh(dim=48)
    assert "clean" not in pm.stats["mesh"] and len(tris) > 0
    cv, ctri = pm.mesh(dim=48, clean=dict(max_components=1))
    want = MR.clean(verts, tris, max_components=1)
    assert cv.tobytes() == want["vertices"].tobytes() and ctri.tobytes() == want["triangles"].tobytes()
    assert counts(pm.stats["mesh"]["clean"]) == want["stats"]
    with pytest.raises(ValueError):
        pm.mesh(dim=48, clean=dict(min_fraction=2))
