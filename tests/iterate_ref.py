"""CPU reference of dp_densify_resume / dp_densify_iterate: a composition of
the oracle's own pieces (oracle/pyoracle.py), nothing new in C.

  resume    or_org_create + or_org_insert(org, p, len(store), 0xFFFFFFFF, out)
            over the offered patches in index order (PatchOrganizer::SetSeeds
            on patches), then GenerationEngine's densify_refine/densify_commit
            loop from _Gen(items=len(store), head=0, per_item=4,
            cell=expand_cell_size, seq0=n, index=1)
  filter    Scene.filter_patches
"""
import numpy as np

NO_PARENT = 0xFFFFFFFF


def make_engine(orc, S, fast=None, threads=8):
    """GenerationEngine with the two calls the iterated drivers use."""

    class ResumeEngine(orc.GenerationEngine):
        def densify_resume(self, patches, keep=None):
            return resume(orc, self, patches, keep)

        def filter_patches(self, patches, passes=3, min_neighbor_frac=0.25):
            return self.S.filter_patches(patches, passes, min_neighbor_frac)

    return ResumeEngine(S, threads=threads, fast=fast)


def resume(orc, eng, patches, keep=None):
    """the organizer and the store rebuilt from patches[keep != 0]; the first
    expansion generation"""
    lib = orc.lib
    patches = np.ascontiguousarray(patches, dtype=orc.PATCH_DTYPE)
    if eng.org:
        lib.or_org_destroy(eng.org)
    eng.org = lib.or_org_create(eng.S._h)
    eng.store = []
    eng.nseeds = len(patches)
    out = np.zeros(1, dtype=orc.PATCH_DTYPE)
    for i in range(len(patches)):
        if keep is not None and not keep[i]:
            continue
        one = np.ascontiguousarray(patches[i:i + 1])
        if lib.or_org_insert(eng.org, orc._p(one), len(eng.store), NO_PARENT, orc._p(out)):
            eng.store.append(out[0].copy())
    n = len(eng.store)
    items = n if (n > 0 and eng.S.opt.max_pops > 0) else 0
    return orc._Gen(items, 0, 4, eng.S.opt.expand_cell_size, len(patches), 1)


def run_all(eng, g):
    """every remaining generation; the store"""
    while g.items:
        cand, acc = eng.densify_refine(g, 0, g.items)
        g = eng.densify_commit(g, cand, acc)
    return eng.densify_result()[0]


def resume_and_run(orc, S, patches, keep=None, fast=None):
    eng = make_engine(orc, S, fast)
    g = resume(orc, eng, patches, keep)
    stored = len(eng.store)
    return run_all(eng, g), stored


def iterate(orc, S, seeds, iterations, passes=3, fast=None):
    """(survivors of the last round, per-round counts, per-round (store, keep))"""
    eng = make_engine(orc, S, fast)
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    rounds, states = [], []
    store = keep = None
    for k in range(iterations):
        if k == 0:
            offered = len(seeds)
            store = eng.densify_all(seeds)
        else:
            offered = int(np.count_nonzero(keep))
            store = run_all(eng, resume(orc, eng, store, keep))
        keep = S.filter_patches(store, passes)
        rounds.append({"offered": offered, "reinserted": int(np.count_nonzero(store["parent"] == NO_PARENT)),
                       "patches": len(store), "filtered_out": int(len(keep) - np.count_nonzero(keep))})
        states.append((store, keep))
    return store[keep != 0], rounds, states
