"""The inputs of the dp_cloud_normals tests: the builders test_gpu_cloud_normals.py
runs on the device, and the list of (name, points, k, max_dist) of every cloud it
estimates, over which test_cloud_normals_cpu.py measures the sweeps the
reference's Jacobi needs."""
import numpy as np


def surface(n, seed, noise=0.01):
    """n points of the height field z = 0.2 sin(3x) cos(2y) over the unit square, with noise"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    z = 0.2 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + noise * rng.standard_normal(n)
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


def holed(n, seed):
    """the surface with points that are not finite"""
    p = surface(n, seed)
    p[::97, 1] = np.float32(np.nan)
    p[5::211] = np.float32([np.inf, 0, 0])
    return p


def sphere(n, seed, centre):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return (np.float64(centre) + v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def lattice(m, z=0.0):
    """an m x m integer lattice in the plane z = const"""
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, np.float32([z]), indexing="ij"), axis=-1).reshape(-1, 3)


TILT_A, TILT_B = np.float64([1, 0.5, 0.25]), np.float64([-0.5, 1, 0.75])


def tilted(n, seed):
    """n points of the plane spanned by TILT_A and TILT_B"""
    uv = np.random.default_rng(seed).random((n, 2))
    return (uv[:, :1] * TILT_A + uv[:, 1:] * TILT_B).astype(np.float32)


LINE_DIR = np.float64([1, 2, -1])


def line(n):
    t = np.arange(n, dtype=np.float64) * 0.01
    return (t[:, None] * LINE_DIR).astype(np.float32)


def duplicated(n, seed):
    """the surface with every third point three times"""
    p = surface(n, seed)
    return np.concatenate([p, p[::3], p[::3]])


def far(n, seed):
    """the surface scaled by 8 and moved by 10^4: a float32 step is 2^-10 there"""
    return (surface(n, seed).astype(np.float64) * 8 + 1e4).astype(np.float32)


def cube_with_centre():
    """the corners of the cube [-1, 1]^3 and its centre"""
    c = [[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    return np.float32(c + [[0, 0, 0]])


SPHERE_CENTRE = np.float32([0.5, -0.25, 2.0])


def cases():
    """every cloud the GPU tests estimate, with its k and max_dist"""
    out = [("tiny", surface(4, 5), 3, 2.0)]
    out += [("widths k=%d" % k, surface(301, 40 + k), k, 0.1) for k in (3, 8, 9, 16, 17, 32)]
    out += [("holed", holed(2003, 7), 16, 0.03), ("strides", surface(300, 11), 8, 0.12),
            ("duplicated", duplicated(150, 13), 8, 0.15), ("line", line(40), 8, 0.2), ("lattice", lattice(12), 9, 1.5),
            ("tilted", tilted(200, 14), 16, 0.3), ("far", far(300, 15), 16, 1.0),
            ("sphere", sphere(400, 16, SPHERE_CENTRE), 12, 0.5), ("directions", surface(300, 17), 10, 0.15),
            ("lattice z=2", lattice(6, 2.0), 9, 1.5), ("shared scratch", holed(500, 19), 16, 0.1),
            ("cube", cube_with_centre(), 9, 4.0)]
    return out
