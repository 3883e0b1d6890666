"""Scenes whose views differ in size, for the stages that take a patch set
through depth maps to a mesh (dp_render_maps, dp_refine_maps, dp_fuse_maps,
dp_tsdf_integrate / dp_tsdf_mesh).  Each of them is written per view -- its own
W, H, image pitch, gray pitch, and its own offset into the z-buffer, the mask
plane and the staging buffers -- under grids sized by the largest requested
view.  A scene of equal sizes cannot tell these apart.

View v of a scene is view v of the synth rig of its own size (the same
construction as filtercases._mixed): synth.cameras(synth.config(V, W_v, H_v,
kind))[v], rendered by synth.render_host of that config.  The rig's poses do not
depend on the size and the texture is a function of the world, so the images
show the same surface at different resolutions.

build(name) returns a Scene; chain(orc, name) its reference chain (render ->
refine -> fuse -> integrate), computed once by the numpy references alone.
tests/test_mapcases_cpu.py asserts on that chain that each scene exercises what
it is named for, so a scene that stops doing so fails instead of silently
passing; tests/test_gpu_mixed_sizes.py compares the kernels against it."""
import functools

import numpy as np

import densepoints_amd as dp
from densepoints_amd import synth

import fuse_ref as FR
import mapref_ref as MR
import render_ref as RR
import tsdf_ref as TR

# mixed:  96 x 72   whole tiles across, 4.5 tiles down
#         70 x 50   no side a multiple of 16
#         131 x 67  odd width; gray pitch 192 where the others are 128 or 64
#         33 x 17   one pixel past a tile on each axis; a plane row shorter than a wave
#         15 x 13   smaller than one refine tile; 195 pixels, fewer than a 256-thread fuse block
MIXED_SIZES = [(96, 72), (70, 50), (131, 67), (33, 17), (15, 13)]
# tiny:   70 x 50   an ordinary view, so that something matches and scores
#         16 x 16   exactly one refine tile
#         17 x 1, 1 x 19   a single row, a single column
#         5 x 3     no refine window fits in it
TINY_SIZES = [(70, 50), (16, 16), (17, 1), (1, 19), (5, 3)]
# the seeds are those of the rig at this size, on a dense grid (Scene.seed_stride)
SEED_SIZE = (70, 50)
# the 19x17x13 volume of tests/test_gpu_tsdf.py: it reaches outside every image and behind the cameras
VOLUME = dict(origin=(-1.8, -1.6, -0.55), voxel=0.19, dim=(19, 17, 13), trunc=0.4)
# the second option set of the refine tests: the widest window and reach, one score per candidate
WIDE = dict(window=11, reach=(16, 0), max_sources=4, top_k=1)


def gray_pitch(W):
    """the gray plane's pitch in pixels (densepoints_amd/csrc/dp_fast.hip)"""
    return (W + 2 + 63) & ~63


class Scene:
    """P (V x 3 x 4), imgs (BGR8, H_v x W_v x 3), sizes [(W_v, H_v)], views
    (dp.View), seeds (n x 3, in front of every camera), and the reference view
    tables of a pyramid level"""

    def __init__(self, name, sizes, kind=1, spread_deg=35.0, seed_stride=6.0, splat_scale=2.0, fuse_from="refine"):
        self.name, self.sizes, self.V, self.kind = name, list(sizes), len(sizes), kind
        self.splat_scale, self.fuse_from = splat_scale, fuse_from
        cfgs = [synth.config(self.V, W, H, kind, spread_deg=spread_deg) for W, H in sizes]
        self.P = np.stack([synth.cameras(c)[v] for v, c in enumerate(cfgs)])
        self.imgs = [synth.render_host(c, self.P, v) for v, c in enumerate(cfgs)]
        self.views = [dp.View(self.P[v], self.imgs[v]) for v in range(self.V)]
        scfg = synth.config(self.V, SEED_SIZE[0], SEED_SIZE[1], kind, spread_deg=spread_deg, seed_stride_px=seed_stride)
        seeds = synth.seeds(scfg, synth.cameras(scfg))
        front = np.all(np.einsum("vj,nj->nv", self.P[:, 2, :3], seeds) + self.P[:, 2, 3] > 0.0, axis=1)
        self.seeds = np.ascontiguousarray(seeds[front])
        self._levels = {0: (self.P, self.imgs)}

    def level(self, orc, level=0):
        """(P_L, images_L) of the level-L scene (orc.level_scene)"""
        if level not in self._levels:
            self._levels[level] = orc.level_scene(self.P, self.imgs, level)
        return self._levels[level]

    def level_sizes(self, orc, level=0):
        return [(im.shape[1], im.shape[0]) for im in self.level(orc, level)[1]]

    def patches(self, orc):
        """the unrefined seed patches, by the oracle's seed conversion"""
        return orc.Scene(self.P, self.imgs).seeds_to_patches(self.seeds)

    def cameras(self, orc, level=0):
        P, imgs = self.level(orc, level)
        return RR.Cameras(orc, P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs])

    def mapref_views(self, orc, level=0):
        P, imgs = self.level(orc, level)
        return MR.Views(orc, P, imgs)

    def fuse_views(self, orc, level=0):
        P, imgs = self.level(orc, level)
        return FR.Views(P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], imgs)

    def tsdf_views(self, orc, level=0):
        P, imgs = self.level(orc, level)
        return TR.Views(P, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], imgs)


# mixed: at the rig's default spread (35 degrees), stride 6 and splat scale 2 the
# discs of the patches whose reference view is one of the two small views (their
# rho is 8 of *their* pixels) cover the three large views completely and the
# refinement has no hole to fill there; a narrower rig, a coarser seed grid and
# half-radius discs leave holes in every view whose neighbours score.
# tiny: the refinement keeps nothing in the views that are too small to be
# scored, so its fusion and integration read the rendered planes.
SCENES = {
    "mixed": dict(sizes=MIXED_SIZES, spread_deg=15.0, seed_stride=8.0, splat_scale=0.5),
    "tiny": dict(sizes=TINY_SIZES, fuse_from="render"),
}


@functools.lru_cache(maxsize=None)
def build(name) -> Scene:
    return Scene(name, **SCENES[name])


def pick(planes, views):
    """the planes of `views` out of one plane per view"""
    return [planes[v] for v in views]


def run_chain(orc, sc, views=None, level=0, refine_kw=None, fuse_kw=None, patches=None):
    """the four stages by the references alone, each on the one before:
    dict(pat, cams, mvw, fvw, tvw, render, refine, maps, fuse, tsdf).  `views`: the
    requested view ids in order (None = all), handed to every stage."""
    pat = sc.patches(orc) if patches is None else patches
    out = dict(pat=pat, views=list(range(sc.V)) if views is None else list(views), cams=sc.cameras(orc, level),
               mvw=sc.mapref_views(orc, level), fvw=sc.fuse_views(orc, level), tvw=sc.tsdf_views(orc, level))
    out["render"] = RR.render(out["cams"], pat, views=views, splat_scale=sc.splat_scale)
    rd = out["render"]
    out["refine"] = MR.refine(out["mvw"], rd["depth"], rd["normal"], views=views, **(refine_kw or {}))
    out["maps"] = out[sc.fuse_from]  # what the fusion and the integration read
    rf = out["maps"]
    out["fuse"] = FR.fuse(out["fvw"], rf["depth"], rf["normal"], views=views, **(fuse_kw or {}))
    out["tsdf"] = TR.integrate(out["tvw"], rf["depth"], views, **VOLUME)
    return out


_chains = {}


def chain(orc, name):
    """run_chain of the whole scene at level 0 with the default options:
    computed once, shared by every test, never modified"""
    if name not in _chains:
        _chains[name] = run_chain(orc, build(name))
    return _chains[name]
