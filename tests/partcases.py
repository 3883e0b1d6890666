"""Planted items for the multi-rank partition (dp_densify_owners /
dp_densify_partition_async; spec in include/densepoints.h): tile_keys_kernel's
floor and clamps, the 2e9 guard, the host's count of key bits, the stable sort
and the cuts floor(r n / world).  On rendered scenes no item projects behind
its camera, onto a tile boundary or into a clamp tile, and no key range is a
power of two.  Here every case is built for one edge.

Generation 0's items are the seed patches of dp_densify_begin(seeds): pos = the
seed (as f32), ref = the nearest camera.  So an item is planted at a chosen
projection by choosing the seed.  The arithmetic is exact by construction:
cameras K [I | -C] with integer centres and power-of-two focal length and
principal point, seeds on a dyadic grid that f32 holds.  Every term of
((p0 x + p1 y) + p2 z) + p3, every quotient h0 / h2, h1 / h2 and every
division by tile_px is then exactly representable, which build() verifies in
rational arithmetic (_verify): the intended tile is not a matter of rounding.

build(name) returns a Case (cached): P (V x 3 x 4), imgs (BGR8, tiny), seeds
(n x 3), tile_px, and per item the intended ref, ty, tx (after clamping) and
the classes it was planted for (Case.classes: label -> item indices).  No GPU
use.  tests/test_partcases_cpu.py asserts on the oracle and on a restatement
of the header's formula that every case reaches what it is named for;
tests/test_gpu_partition_edges.py runs the kernels on them."""
import functools
from fractions import Fraction

import numpy as np

WORLDS = (1, 2, 3, 7, 8, 63, 64)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
SPACING = 64  # between camera centres, along x: far more than any seed's offset from its camera


class Cam:
    """K [I | -C]: looking down +z from the integer centre C"""

    def __init__(self, index, W=128, H=128, f=64.0, cx=64.0, cy=64.0):
        self.C = (float(SPACING * index), 0.0, 0.0)
        self.W, self.H, self.f, self.cx, self.cy = W, H, f, cx, cy

    @property
    def P(self):
        C, f, cx, cy = self.C, self.f, self.cx, self.cy
        return np.array([[f, 0.0, cx, -(f * C[0] + cx * C[2])],
                         [0.0, f, cy, -(f * C[1] + cy * C[2])],
                         [0.0, 0.0, 1.0, -C[2]]])

    def at(self, u, v, depth=1.0):
        """the point at `depth` along +z that projects to pixel (u, v); a
        negative depth is behind the camera"""
        return (self.C[0] + (u - self.cx) * depth / self.f, self.C[1] + (v - self.cy) * depth / self.f,
                self.C[2] + depth)


class Case:
    def __init__(self, name, cams, tile_px, items):
        self.name, self.cams, self.tile_px = name, cams, int(tile_px)
        self.V = len(cams)
        self.P = np.stack([c.P for c in cams])
        self.sizes = [(c.W, c.H) for c in cams]
        self.imgs = [np.full((c.H, c.W, 3), 31 + 40 * v, dtype=np.uint8) for v, c in enumerate(cams)]
        self.TX = -(-max(c.W for c in cams) // self.tile_px)
        self.TY = -(-max(c.H for c in cams) // self.tile_px)
        self.seeds = np.array([it[1] for it in items], dtype=np.float64).reshape(-1, 3)
        self.ref = np.array([it[0] for it in items], dtype=np.int64)
        self.ty = np.array([it[2] for it in items], dtype=np.int64)
        self.tx = np.array([it[3] for it in items], dtype=np.int64)
        self.classes = {}
        for i, it in enumerate(items):
            for label in it[4]:
                self.classes.setdefault(label, []).append(i)
        assert np.all((self.ty >= -1) & (self.ty <= self.TY) & (self.tx >= -1) & (self.tx <= self.TX)), name
        _verify(self)

    @property
    def n(self):
        return len(self.seeds)

    @property
    def key(self):
        """the intended dense keys (python ints)"""
        return [(int(r) * (self.TY + 2) + int(y) + 1) * (self.TX + 2) + int(x) + 1
                for r, y, x in zip(self.ref, self.ty, self.tx)]

    @property
    def key_range(self):
        return self.V * (self.TY + 2) * (self.TX + 2)


def _double(fr):
    x = float(fr)
    assert Fraction(x) == fr, "not a double: %s" % fr
    return fr


def _verify(case):
    """every seed is an f32 with one nearest camera, the intended one, and every
    step of its projection and its tile quotients is exact in fp64"""
    for i, X in enumerate(case.seeds):
        assert all(float(np.float32(c)) == c for c in X), (case.name, i, "seed is not an f32")
        Xf = [Fraction(float(c)) for c in X]
        d2 = [sum((a - Fraction(c)) ** 2 for a, c in zip(Xf, cam.C)) for cam in case.cams]
        assert d2.count(min(d2)) == 1 and d2.index(min(d2)) == case.ref[i], (case.name, i, "nearest camera")
        h = []
        for row in case.P[case.ref[i]]:
            p = [Fraction(float(c)) for c in row]
            s = _double(_double(p[0] * Xf[0]) + _double(p[1] * Xf[1]))
            s = _double(s + _double(p[2] * Xf[2]))
            h.append(_double(s + p[3]))
        if h[2] != 0:
            for a in h[:2]:
                _double(_double(a / h[2]) / case.tile_px)


class _Items(list):
    """the items of a case under construction: (ref, seed, ty, tx, labels)"""

    def __init__(self, cams, tile_px):
        super().__init__()
        self.cams, self.tile = cams, tile_px

    def pixel(self, ref, u, v, ty, tx, *labels, depth=1.0):
        self.append((ref, self.cams[ref].at(u, v, depth), ty, tx, labels))

    def point(self, ref, xyz, ty, tx, *labels):
        self.append((ref, tuple(float(c) for c in xyz), ty, tx, labels))

    def tile_item(self, ref, ty, tx, fv, fu, *labels):
        """inside tile (ty, tx) at the fractions (fv, fu) of a tile"""
        self.pixel(ref, (tx + fu) * self.tile, (ty + fv) * self.tile, ty, tx, *labels)


def _boundaries():
    """items strictly inside tiles; u / tile and v / tile exactly integer (the
    higher tile); one ulp below an integer (the lower one)"""
    cams = [Cam(0), Cam(1)]
    it = _Items(cams, 64)
    for r in (1, 0):
        it.pixel(r, 100.0, 70.0, 1, 1, "interior")
        it.pixel(r, 10.5, 20.25, 0, 0, "interior")
        it.pixel(r, 64.0, 64.0, 1, 1, "integer_u", "integer_v")
        it.pixel(r, 64.0, 10.0, 0, 1, "integer_u")
        it.pixel(r, 10.0, 64.0, 1, 0, "integer_v")
        it.pixel(r, 0.0, 0.0, 0, 0, "integer_u", "integer_v", "zero")
        it.pixel(r, 128.0, 128.0, 2, 2, "integer_u", "integer_v")
        it.pixel(r, -64.0, -64.0, -1, -1, "integer_u", "integer_v", "negative_integer")
    # camera 0 stands at the origin: x = -2^-53 at depth 1 is u = 64 - 2^-47,
    # the double below 64, and u / 64 the double below 1
    e = 2.0 ** -53
    it.point(0, (-e, 0.5, 1.0), 1, 0, "ulp_below_u")
    it.point(0, (0.5, -e, 1.0), 0, 1, "ulp_below_v")
    it.point(0, (-e, -e, 1.0), 0, 0, "ulp_below_u", "ulp_below_v")
    return Case("boundaries", cams, 64, it)


def _clamps():
    """150 x 140 at tile 64: TX = TY = 3 with a partial last tile; the clamp
    tiles -1 and TX / TY on both axes, and the corner (TY, TX) of the last view"""
    cams = [Cam(0, 150, 140), Cam(1, 150, 140)]
    it = _Items(cams, 64)
    for r in (0, 1):
        it.pixel(r, -32.0, 70.0, 1, -1, "u_first_below")        # [-tile, 0)
        it.pixel(r, -200.0, 70.0, 1, -1, "u_far_below")         # < -tile
        it.pixel(r, 140.0, 70.0, 1, 2, "u_last_partial")        # [128, 150)
        it.pixel(r, 170.0, 70.0, 1, 2, "u_past_image")          # past the image, before TX * tile
        it.pixel(r, 192.0, 70.0, 1, 3, "u_at_TX")               # == TX * tile
        it.pixel(r, 300.0, 70.0, 1, 3, "u_above")
        it.pixel(r, 70.0, -32.0, -1, 1, "v_first_below")
        it.pixel(r, 70.0, -200.0, -1, 1, "v_far_below")
        it.pixel(r, 70.0, 135.0, 2, 1, "v_last_partial")
        it.pixel(r, 70.0, 170.0, 2, 1, "v_past_image")
        it.pixel(r, 70.0, 192.0, 3, 1, "v_at_TY")
        it.pixel(r, 70.0, 300.0, 3, 1, "v_above")
        it.pixel(r, -100.0, -100.0, -1, -1, "corner_low")
    it.pixel(1, 250.0, 250.0, 3, 3, "largest_key")
    it.pixel(0, 70.0, 70.0, 1, 1)
    return Case("clamps", cams, 64, it)


def _non_numbers():
    """0/0, x/0, a negative depth, and quotients at, beyond and just inside
    +-2e9.  Camera 0 stands at the origin with its principal point at 8192 =
    128 tiles: at depth 2^-31 the quotient is x 2^31 + 128, and x = (15625000
    - 1) 2^-24 (an f32) makes it exactly 2e9 = 15625000 * 128; one f32 step of
    x is 128 tiles."""
    cams = [Cam(0, cx=8192.0, cy=8192.0), Cam(1)]
    it = _Items(cams, 64)
    TX = TY = 2
    for r in (0, 1):
        C = cams[r].C
        it.point(r, C, 0, 0, "centre")                                        # 0/0, 0/0
        it.point(r, (C[0] + 1.0, C[1] - 1.0, C[2]), 0, 0, "principal_plane")  # +inf, -inf
        it.point(r, (C[0], C[1] + 2.0, C[2]), 0, 0, "principal_plane")        # 0/0, +inf
    # behind the camera the image is mirrored: a point to the right of and
    # below the axis projects to the left of and above the principal point
    it.pixel(1, -32.0, 70.0, 1, -1, "behind", depth=-1.0)
    it.pixel(1, 100.0, 20.0, 0, 1, "behind", depth=-2.0)
    assert it[-1][1][0] < cams[1].C[0] and it[-1][1][2] < 0.0
    d = 2.0 ** -31
    s = 2.0 ** -24
    mid = (100.0 - 8192.0) * d / 64.0  # the other coordinate: pixel 100, tile 1

    def big(m, axis, t, *labels):
        # quotient m * 128 + 128 on `axis` (0: u, 1: v), tile 1 on the other
        xyz = [mid, mid, d]
        xyz[axis] = m * s
        it.point(0, xyz, *((1, t) if axis == 0 else (t, 1)), *labels)

    for axis, tmax in ((0, TX), (1, TY)):
        big(15625000 - 1, axis, 0, "at_+2e9")
        big(-15625000 - 1, axis, 0, "at_-2e9")
        big(15625000, axis, 0, "beyond_+2e9")
        big(-15625000 - 2, axis, 0, "beyond_-2e9")
        big(16777215, axis, 0, "beyond_+2e9")  # 2^31 + 0: past the int32 range
        big(15625000 - 2, axis, tmax, "inside_+2e9")
        big(-15625000, axis, -1, "inside_-2e9")
    it.pixel(0, 70.0, 70.0, 1, 1)
    it.pixel(1, 250.0, 250.0, 2, 2, "largest_key")
    return Case("non_numbers", cams, 64, it)


def _key_width(name, W):
    """4 views of W x 128 at tile 64.  W = 128: V (TY + 2) (TX + 2) = 4 * 4 * 4
    = 64, an exact power of two, so the largest key 63 needs all 6 bits; W =
    129: 4 * 4 * 5 = 80.  Every tile of every view once, highest key first."""
    cams = [Cam(v, W, 128) for v in range(4)]
    it = _Items(cams, 64)
    TX = -(-W // 64)
    for r in reversed(range(4)):
        for ty in reversed(range(-1, 3)):
            for tx in reversed(range(-1, TX + 1)):
                labels = ("largest_key",) if (r, ty, tx) == (3, 2, TX) else ()
                it.tile_item(r, ty, tx, 0.25, 0.5, *labels)
    return Case(name, cams, 64, it)


def _nine_keys():
    """one 128 x 128 view at tile 128: TX = TY = 1 and 1 * 3 * 3 = 9 keys, one
    above a power of two, so the largest key 8 is the only one with bit 3"""
    cams = [Cam(0)]
    it = _Items(cams, 128)
    for ty in (1, 0, -1):
        for tx in (1, 0, -1):
            it.tile_item(0, ty, tx, 0.5, 0.25, *(("largest_key",) if (ty, tx) == (1, 1) else ()))
    return Case("nine_keys", cams, 128, it)


def _tile1():
    """tile_px = 1 on 8 x 6 views: every pixel a tile, every integer pixel a
    boundary"""
    cams = [Cam(0, 8, 6, cx=4.0, cy=2.0), Cam(1, 8, 6, cx=4.0, cy=2.0)]
    it = _Items(cams, 1)
    for r in (1, 0):
        for ty in (6, 3, 0, -1):
            for tx in (8, 7, 1, 0, -1):
                it.pixel(r, float(tx), float(ty), ty, tx, "integer_u", "integer_v")
                it.pixel(r, tx + 0.5, ty + 0.25, ty, tx, "interior")
        it.pixel(r, -3.0, -2.0, -1, -1, "u_far_below")
        it.pixel(r, 11.0, 9.0, 6, 8, "u_above")
    it.pixel(1, 20.0, 20.0, 6, 8, "largest_key")
    return Case("tile1", cams, 1, it)


def _tile_huge():
    """tile_px = 256 on 128 x 128 views: TX = TY = 1, tiles -1, 0 and 1 only"""
    cams = [Cam(0), Cam(1)]
    it = _Items(cams, 256)
    for r in (1, 0):
        it.pixel(r, -300.0, 64.0, 0, -1, "u_far_below")
        it.pixel(r, -1.0, -1.0, -1, -1, "u_first_below")
        it.pixel(r, 0.0, 0.0, 0, 0, "integer_u")
        it.pixel(r, 127.0, 127.0, 0, 0, "interior")
        it.pixel(r, 255.5, 200.0, 0, 0, "u_past_image")
        it.pixel(r, 256.0, 64.0, 0, 1, "u_at_TX")
        it.pixel(r, 1000.0, 1000.0, 1, 1, "u_above")
    it.pixel(1, 256.0, 256.0, 1, 1, "largest_key")
    return Case("tile_huge", cams, 256, it)


def _unequal():
    """TX = 4 and TY = 2 come from the 200-wide and the 128-high view; the
    items of the 40 x 24 view are clamped to those, not to its own 1 x 1 tiles"""
    cams = [Cam(0), Cam(1, 40, 24, cx=16.0, cy=8.0), Cam(2, 200, 72)]
    it = _Items(cams, 64)
    small = 1
    for ty in (2, 1, 0, -1):
        for tx in (4, 3, 2, 1, 0, -1):
            labels = ["smallest_view"]
            if tx > 1 or ty > 1:
                labels.append("past_own_tiles")
            it.tile_item(small, ty, tx, 0.5, 0.125, *labels)
    it.pixel(small, 1000.0, 70.0, 1, 4, "smallest_view", "past_own_tiles", "u_above")
    it.pixel(small, 10.0, 1000.0, 2, 0, "smallest_view", "past_own_tiles", "v_above")
    it.pixel(0, 300.0, 100.0, 1, 4, "past_own_tiles")
    it.pixel(2, 150.0, 100.0, 1, 2)
    it.pixel(2, 400.0, 400.0, 2, 4, "largest_key")
    return Case("unequal", cams, 64, it)


# ties: the runs of equal keys in key order: [0, 24), [24, 56), [56, 70),
# [70, 112), [112, 150), [150, 168).  n = 168 is a multiple of 2, 3, 7 and 8:
#   world 2   84                 inside [70, 112)
#   world 3   56, 112            both on a run's edge: no tile is split
#   world 7   24 on an edge; 48, 72, 96, 120, 144 inside
#   world 8   21, 42, 63, 84, 105, 126, 147 all inside
TIE_RUNS = (24, 32, 14, 42, 38, 18)


def _ties():
    cams = [Cam(0), Cam(1), Cam(2)]
    tiles = [(0, 0, 0), (0, 1, 2), (1, -1, -1), (1, 1, 1), (2, 0, 1), (2, 2, 2)]  # ascending keys
    sorted_items = []
    for run, (r, ty, tx) in zip(TIE_RUNS, tiles):
        for k in range(run):
            sorted_items.append((r, ty, tx, (k % 8) / 8.0, (k // 8) / 8.0))
    n = len(sorted_items)
    it = _Items(cams, 64)
    for i in range(n):  # given in an order that is not sorted by key: 65 is coprime to 168
        r, ty, tx, fv, fu = sorted_items[(i * 65 + 11) % n]
        it.tile_item(r, ty, tx, fv, fu, "tie")
    return Case("ties", cams, 64, it)


def _few():
    """fewer items than most worlds: cuts coincide and shares are empty"""
    cams = [Cam(0), Cam(1)]
    it = _Items(cams, 64)
    it.tile_item(1, 1, 1, 0.5, 0.5, "tie")
    it.tile_item(0, 0, 1, 0.5, 0.5)
    it.tile_item(1, 1, 1, 0.25, 0.75, "tie")
    it.tile_item(1, -1, 2, 0.5, 0.5)
    it.tile_item(1, 1, 1, 0.125, 0.5, "tie")
    return Case("few", cams, 64, it)


def _sized(n):
    """n items hashed over the 48 tiles (clamp tiles included) of 3 views"""
    cams = [Cam(0), Cam(1), Cam(2)]
    it = _Items(cams, 64)
    for i in range(n):
        h = ((i + 1) * 2654435761) & 0xFFFFFFFF
        it.tile_item((h >> 20) % 3, (h >> 8) % 4 - 1, (h >> 16) % 4 - 1, ((h >> 12) % 16) / 16.0, ((h >> 4) % 16) / 16.0)
    return Case("n%d" % n, cams, 64, it)


BUILDERS = {
    "boundaries": _boundaries,
    "clamps": _clamps,
    "non_numbers": _non_numbers,
    "pow2_keys": lambda: _key_width("pow2_keys", 128),
    "pow2_keys_plus_column": lambda: _key_width("pow2_keys_plus_column", 129),
    "nine_keys": _nine_keys,
    "tile1": _tile1,
    "tile_huge": _tile_huge,
    "unequal": _unequal,
    "ties": _ties,
    "few": _few,
}
BUILDERS.update({"n%d" % n: functools.partial(_sized, n) for n in SIZES})
NAMES = tuple(BUILDERS)

# the classes each case must hold at least one item of (test_partcases_cpu.py)
REQUIRED = {
    "boundaries": ("interior", "integer_u", "integer_v", "zero", "negative_integer", "ulp_below_u", "ulp_below_v"),
    "clamps": ("u_first_below", "u_far_below", "u_last_partial", "u_past_image", "u_at_TX", "u_above",
               "v_first_below", "v_far_below", "v_last_partial", "v_past_image", "v_at_TY", "v_above",
               "corner_low", "largest_key"),
    "non_numbers": ("centre", "principal_plane", "behind", "at_+2e9", "at_-2e9", "beyond_+2e9", "beyond_-2e9",
                    "inside_+2e9", "inside_-2e9", "largest_key"),
    "pow2_keys": ("largest_key",),
    "pow2_keys_plus_column": ("largest_key",),
    "nine_keys": ("largest_key",),
    "tile1": ("integer_u", "integer_v", "interior", "u_far_below", "u_above", "largest_key"),
    "tile_huge": ("u_far_below", "u_first_below", "integer_u", "interior", "u_past_image", "u_at_TX", "u_above",
                  "largest_key"),
    "unequal": ("smallest_view", "past_own_tiles", "u_above", "v_above", "largest_key"),
    "ties": ("tie",),
    "few": ("tie",),
}


@functools.lru_cache(maxsize=None)
def build(name) -> Case:
    return BUILDERS[name]()


_runs = {}


def oracle_run(orc, name):
    """(case, seed patches, {world: (owners, statistics, keys)}) of generation 0
    by the oracle's GenerationEngine: computed once, shared by every test,
    never modified"""
    if name not in _runs:
        case = build(name)
        G = orc.GenerationEngine(orc.Scene(case.P, case.imgs))
        g = G.densify_begin(case.seeds)
        out = {}
        for world in WORLDS:
            own, fb = G.densify_owners(g, world, case.tile_px)
            assert fb is False
            out[world] = (own, G.densify_partition_stats(), G.densify_partition_keys())
        _runs[name] = (case, G.sp.copy(), out)
    return _runs[name]


def cuts(n, world):
    """lo_r = floor(r n / world), r = 0 .. world"""
    return [(r * n) // world for r in range(world + 1)]
