"""CPU reference of dp_mesh_components / dp_mesh_clean, restated in numpy from
the spec in include/densepoints.h: a vectorised minimum-propagation labeller,
integer counts, the rank by (triangles descending, number ascending), the
selection and the two compactions.  Also the meshes the CPU and the GPU tests
share: the hand mesh, the deep strip, and the sphere volume with planted blobs."""
import numpy as np

VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("rgb", "u1", 3), ("pad", "u1")])
COMPONENT_DTYPE = np.dtype([("root", "<i4"), ("vertices", "<i4"), ("triangles", "<i4"), ("rank", "<i4")])
COUNTS = ("vertices_in", "triangles_in", "invalid_triangles", "unused_vertices", "components", "largest_triangles",
          "components_kept", "vertices_out", "triangles_out")


def as_triangles(triangles):
    t = np.asarray(triangles, dtype=np.int32)
    return t.reshape(-1, 3) if t.size else np.zeros((0, 3), np.int32)


def components(triangles, n_vertices):
    """dict(vertex_component, triangle_component, components, valid, used, stats)"""
    tris, nv = as_triangles(triangles), int(n_vertices)
    valid = ((tris >= 0) & (tris < nv)).all(axis=1)
    vt = tris[valid].astype(np.int64)
    used = np.zeros(nv, bool)
    used[vt.ravel()] = True
    # label(v) = the smallest index of v's set: every triangle hands its smallest
    # label to its three vertices, then every vertex takes its label's label
    label = np.arange(nv, dtype=np.int64)
    while len(vt):
        new = label.copy()
        np.minimum.at(new, vt.ravel(), np.repeat(label[vt].min(axis=1), 3))
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    roots = np.flatnonzero(used & (label == np.arange(nv)))
    C = len(roots)
    number = np.full(nv, -1, np.int64)
    number[roots] = np.arange(C)
    vc = np.where(used, number[label], -1).astype(np.int32)
    tc = np.full(len(tris), -1, np.int32)
    tc[valid] = vc[vt[:, 0]]
    table = np.zeros(C, COMPONENT_DTYPE)
    table["root"] = roots
    table["vertices"] = np.bincount(vc[used], minlength=C)
    table["triangles"] = T = np.bincount(tc[valid], minlength=C)
    rank = np.zeros(C, np.int64)
    rank[np.lexsort((np.arange(C), -T))] = np.arange(C)
    table["rank"] = rank
    stats = dict(vertices_in=nv, triangles_in=len(tris), invalid_triangles=int((~valid).sum()),
                 unused_vertices=int((~used).sum()), components=C, largest_triangles=int(T.max()) if C else 0,
                 components_kept=C, vertices_out=int(used.sum()), triangles_out=int(valid.sum()))
    return dict(vertex_component=vc, triangle_component=tc, components=table, valid=valid, used=used, stats=stats)


def clean(vertices, triangles, min_triangles=1, min_fraction=0.0, max_components=0):
    """dict(vertices, triangles, vertex_map, triangle_map, kept, stats)"""
    verts, tris = np.asarray(vertices, dtype=VERTEX_DTYPE).reshape(-1), as_triangles(triangles)
    lab = components(tris, len(verts))
    table = lab["components"]
    T = table["triangles"].astype(np.int64)
    tmax = lab["stats"]["largest_triangles"]
    kept = (T >= int(min_triangles)) & (T.astype(np.float64) >= np.float64(np.float32(min_fraction)) * np.float64(tmax))
    if max_components:
        kept &= table["rank"] < int(max_components)
    vc, tc = lab["vertex_component"], lab["triangle_component"]
    keepv = lab["used"] & kept[np.maximum(vc, 0)] if len(kept) else np.zeros(len(verts), bool)
    keept = lab["valid"] & kept[np.maximum(tc, 0)] if len(kept) else np.zeros(len(tris), bool)
    vmap = np.where(keepv, np.cumsum(keepv) - 1, -1).astype(np.int32)
    tmap = np.where(keept, np.cumsum(keept) - 1, -1).astype(np.int32)
    tout = vmap[tris[keept]].astype(np.int32).reshape(-1, 3)
    assert (tout >= 0).all()
    stats = dict(lab["stats"], components_kept=int(kept.sum()), vertices_out=int(keepv.sum()),
                 triangles_out=int(keept.sum()))
    return dict(vertices=verts[keepv], triangles=tout, vertex_map=vmap, triangle_map=tmap, kept=kept, stats=stats)


def random_vertices(n, seed):
    """n vertex records with every byte random (the pad byte too: it is copied)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=16 * n, dtype=np.uint8)
    v = raw.view(VERTEX_DTYPE).copy()
    v["pos"] = rng.standard_normal((n, 3)).astype(np.float32)  # no NaN payloads to compare
    return v


HAND_NV = 16


def hand_mesh():
    """One mesh of 16 vertices: 0, 6 and 15 unused; two disjoint triangles; a
    bow-tie through vertex 7 whose first triangle (9, 4, 7) does not start at its
    root; triangles with repeated indices, one of them a component of its own;
    invalid triangles with the indices -1 and n_vertices, one of which would join
    two components if it were not refused.  Returns (triangles, n_vertices)."""
    n = HAND_NV
    tris = [(1, 2, 3), (10, 11, 12), (9, 4, 7), (7, 5, 8), (2, 2, 1), (14, 14, 14), (-1, 1, 2), (1, n, 2), (n, n, n),
            (3, 4, -1), (13, 12, 12), (-1, -1, -1)]
    return np.array(tris, np.int32), n


def deep_mesh(strip=5000, singles=3000, seed=20261101):
    """A strip of `strip` triangles (i, i+1, i+2) and `singles` single-triangle
    components, the vertex indices through a random permutation and the triangle
    order shuffled.  Returns (triangles, n_vertices)."""
    rng = np.random.default_rng(seed)
    i = np.arange(strip)
    a = np.stack([i, i + 1, i + 2], axis=1)
    j = strip + 2 + 3 * np.arange(singles)
    b = np.stack([j, j + 1, j + 2], axis=1)
    nv = strip + 2 + 3 * singles
    tris = rng.permutation(nv)[np.concatenate([a, b])]
    return np.ascontiguousarray(rng.permutation(tris), dtype=np.int32), nv


# the sphere volume of the end-to-end test: a clipped distance field, weight 1
BLOB_VOLUME = dict(origin=(-1.0, -0.9, -0.8), voxel=2.0 / 24.0, dim=(24, 21, 19), trunc=3.0 * 2.0 / 24.0)
BLOB_RADIUS = 0.45
BLOBS = ((1, 1, 1, 1), (1, 1, 5, 1), (1, 6, 1, 2), (15, 17, 20, 2), (1, 15, 18, 1), (16, 1, 1, 1))  # k, j, i, size
BLOB_TRIANGLES = (3300, 144, 144, 24, 24, 24, 24)  # of the components, descending
SPHERE_COUNTS = (1652, 3300)  # vertices, triangles of the sphere alone


def blob_volumes():
    """(sphere-only tsdf, tsdf with the blobs planted, weight), each [nz][ny][nx]"""
    nx, ny, nz = BLOB_VOLUME["dim"]
    o, h = BLOB_VOLUME["origin"], BLOB_VOLUME["voxel"]
    x = o[0] + (np.arange(nx) + 0.5) * h
    y = o[1] + (np.arange(ny) + 0.5) * h
    z = o[2] + (np.arange(nz) + 0.5) * h
    d = np.sqrt(x[None, None, :] ** 2 + y[None, :, None] ** 2 + z[:, None, None] ** 2)
    sphere = np.clip((d - BLOB_RADIUS) / BLOB_VOLUME["trunc"], -1.0, 1.0).astype(np.float32)
    planted = sphere.copy()
    for k, j, i, s in BLOBS:
        shell = sphere[k - 1:k + s + 1, j - 1:j + s + 1, i - 1:i + s + 1]
        assert shell.shape == (s + 2,) * 3 and (shell == 1.0).all(), (k, j, i, s)
        planted[k:k + s, j:j + s, i:i + s] = -0.5
    return sphere, planted, np.ones((nz, ny, nx), np.int32)
