/*
 * densepoints.h -- C ABI of the MI355X-native PMVS patch-loop engine
 * (libdensepoints.so, built from densepoints_amd/csrc/).
 *
 * Drop-in boundary for the reference's hot path (manlito/densepoints):
 *   operator seam  methods/pmvs/optimization.h:11-45 (Optimization,
 *                  virtual Optimize / FilterByErrorMeasurement /
 *                  GetProjectedTextures), methods/pmvs/optimization_opencv.h:10-14
 *   scoring op     modules/core/error_measurements.h:11 (NCCScore)
 *   callers        methods/pmvs/seed.cpp:110-144, expand.cpp:103-143,
 *                  pmvs.cpp:11-43 (PMVS::AddCamera / Run)
 * The reference constructs one Optimization per patch on the stack and calls
 * it from OpenMP workers; this ABI takes BATCHES of patches (one wavefront
 * per patch on the GPU).  Plain C: POD structs, pointers and sizes only.
 *
 * All functions return DP_OK (0) or a negative DP_E_* status; the message of
 * the last failure on a context is available from dp_last_error().
 * A context is single-host-thread; use one context per GPU.
 */
#ifndef DENSEPOINTS_H
#define DENSEPOINTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DP_ABI_VERSION 2

/* ---- status codes (replace LOG(FATAL) / cv::Exception) ------- */
#define DP_OK 0
#define DP_E_ARG (-1)          /* bad argument / unsupported option value          */
#define DP_E_HIP (-2)          /* HIP runtime failure (message in dp_last_error)   */
#define DP_E_OOM (-3)          /* device or host allocation failed                 */
#define DP_E_DEGENERATE (-4)   /* dx == 0 (optimization.cpp:27 LOG(FATAL))         */
#define DP_E_STATE (-5)        /* call order violated (e.g. no views set)          */
#define DP_E_NODEVICE (-6)     /* no HIP device available                          */

#define DP_MAX_VIEWS 128       /* visible/candidate sets are 128-bit masks          */
#define DP_MAX_CELL 16         /* n x n window, n <= 16 (reference uses 16 and 11)  */
#define DP_MAX_LEVELS 8        /* image pyramid levels (dp_build_pyramid)           */

/* ---- options: every hot-path knob, reference defaults --- */
typedef struct dp_options {
    int32_t seed_cell_size;       /* 16  matcher.h:25, used at seed.cpp:117,135       */
    int32_t expand_cell_size;     /* 11  expand.h:12, used at expand.cpp:129          */
    int32_t grid_scale;           /* 8   patch_organizer.h:43                          */
    int32_t max_patches_per_cell; /* 1   patch_organizer.h:42 (1..64; a cell keeps its first k claims) */
    int32_t min_visible;          /* 3   optimization.h:17                             */
    int32_t min_expand_visible;   /* 2   expand.cpp:67                                 */
    int32_t nm_max_evals;         /* 500 optimization_opencv.cpp:60                    */
    int32_t reserved0;
    double ncc_threshold;         /* 0.6  optimization.h:16                            */
    double visible_angle;         /* 0.78 patch.h:56                                   */
    double candidate_angle;       /* 1.04 patch.h:57                                   */
    double nm_step[3];            /* 0.02, 0.2, 0.2 optimization_opencv.cpp:56         */
    double nm_eps;                /* 1e-4 optimization_opencv.cpp:60                   */
    double ncc_denom_min;         /* 0.1  error_measurements.cpp:57                    */
    int64_t max_pops;             /* 1e7  expand.cpp:95                                */
} dp_options;

/* ---- patch record: pcl::PointXYZRGBNormal + Patch bookkeeping (patch.h:86-100)
 * Ascending view lists (visible_images_, candidate_images_) are stored as
 * 128-bit masks, which is lossless because the reference only ever builds
 * them in ascending order (patch.cpp:37-47) and erases elements in place. */
typedef struct dp_patch {
    float pos[3];        /* centre, f32 as stored by Patch::SetPosition          */
    float normal[3];     /* f32 as stored by Patch::SetNormal                     */
    uint32_t ref;        /* reference view (Patch::reference_image_)             */
    uint32_t seq;        /* organizer / queue index (dp_densify output)           */
    uint64_t vis[2];     /* visible_images_ bitmask                               */
    uint64_t cand[2];    /* candidate_images_ bitmask                             */
    float score;         /* mean NCC of the last filter evaluation (extension)    */
    uint32_t evals;      /* objective evaluations spent on this patch (E)         */
    uint8_t rgb[3];      /* Patch::ComputeColor (patch.cpp:51-73)                 */
    uint8_t flags;       /* DP_PATCH_*                                            */
    uint32_t parent;     /* parent queue index; 0xFFFFFFFF for seed patches       */
} dp_patch;

#define DP_PATCH_ACCEPTED 1u
#define DP_PATCH_DEGENERATE 2u

/* ---- refine modes: which reference call sequence runs per patch ---------- */
#define DP_MODE_EVAL 0    /* one evaluation: scores only, no mutation            */
#define DP_MODE_FILTER 1  /* Optimization::FilterByErrorMeasurement (opt.cpp:98)*/
#define DP_MODE_NM 2      /* OptimizationOpenCV::Optimize (opencv.cpp:44-78)     */
#define DP_MODE_SEED 3    /* Seed::FilterPatches then OptimizePatches            */
#define DP_MODE_EXPAND 4  /* Optimize -> InitRelatedImages -> Filter (expand.cpp:127-135) */
/* performance mode (no reference counterpart; spec below, dp_fast_options) */
#define DP_MODE_FAST_EVAL 5    /* one fast evaluation at the stored pose: score only */
#define DP_MODE_FAST_REFINE 6  /* fast CG refine -> InitRelatedImages -> fast filter */

/* ---- images: BGR8 as cv::imread returns it (types.cpp:9) ----------------- */
typedef struct dp_image {
    int32_t width;
    int32_t height;
    int32_t stride;      /* bytes per row; 0 = 3*width                            */
    int32_t reserved;
    const uint8_t *bgr;  /* host pointer, copied by dp_set_views                 */
} dp_image;

typedef struct dp_densify_stats {
    int64_t seeds_in;          /* seed points given                               */
    int64_t seed_patches;      /* seed patches accepted by the organizer           */
    int64_t patches;           /* total patches (seed + expanded)                  */
    int64_t pops;              /* queue pops (expand.cpp:87)                       */
    int64_t candidates;        /* expansion candidates refined (4 per expanded pop)*/
    int64_t evals;             /* objective evaluations in all refine kernels      */
    int32_t generations;       /* BFS generations                                  */
    int32_t stalls;            /* device-resident generations that outgrew the
                                  candidate buffers and were resumed (dp_densify_run) */
    double refine_ms;          /* device time in the fused refine kernels          */
    double total_ms;           /* wall time of dp_densify                          */
} dp_densify_stats;

typedef struct dp_ctx dp_ctx;

/* defaults identical to the reference constructors (list in dp_options) */
void dp_default_options(dp_options *opt);
int dp_abi_version(void);
/* number of HIP devices visible to the process (0 if none) */
int dp_device_count(void);

/* Create a context bound to HIP device `device`. */
int dp_ctx_create(const dp_options *opt, int device, dp_ctx **out);
int dp_ctx_destroy(dp_ctx *ctx);
const char *dp_last_error(const dp_ctx *ctx);
int dp_set_options(dp_ctx *ctx, const dp_options *opt);

/* PMVS::AddCamera (pmvs.cpp:11-20) for all views at once.  P: V x 3x4
 * row-major fp64; images BGR8 host buffers, uploaded as BGRA8 SoA planes. */
int dp_set_views(dp_ctx *ctx, int V, const double *P, const dp_image *images);

/* Same, but the views' BGRA8 pixels are already resident on this device
 * (dev_bgra[v] points to height*pitch_px uint32 pixels, B in the low byte).
 * No copy: the caller keeps the buffers alive while the context uses them. */
int dp_set_views_device(dp_ctx *ctx, int V, const double *P, const int32_t *width,
                        const int32_t *height, const int32_t *pitch_px,
                        const void *const *dev_bgra);

/* ---- image pyramids (BASELINE configs "N pyramid levels") --
 * The reference samples full-resolution images only: methods/pmvs Options::scale
 * (options.h:10) is stored but never read, and PMVS::AddCamera (pmvs.cpp:11-20)
 * keeps the cv::imread image.  Level l+1 = cv::pyrDown of level l (5x5 binomial
 * [1 4 6 4 1]^2/256, BORDER_REFLECT_101, size ((W+1)/2, (H+1)/2), per-channel
 * (s + 128) >> 8), built on the device from the level-0 planes.
 * dp_set_level(L) runs every later call on level L: images = level L, projection
 * rows 0-1 scaled by 2^-L (pyrDown's pixel grid), camera geometry and organizer
 * grids recomputed from that P -- i.e. the reference algorithm applied to the
 * level-L scene.  dp_set_views resets to level 0 and drops the pyramid. */
int dp_build_pyramid(dp_ctx *ctx, int levels);          /* 1 <= levels <= DP_MAX_LEVELS */
int dp_set_level(dp_ctx *ctx, int level);
int dp_level_info(const dp_ctx *ctx, int level, int view, int32_t *width, int32_t *height,
                  const void **d_bgra);
/* host BGR8 copy (width*height*3 bytes) of one pyramid level of one view */
int dp_read_level(dp_ctx *ctx, int level, int view, uint8_t *bgr_out);

/* View::SetProjectionMatrix (types.cpp:28-68): camera centre, K (normalised
 * K(2,2)=1, positive diagonal), [R|t] and the camera x-axis (row 0 of R). */
int dp_view_geometry(const double P[12], double C[3], double K[9], double E[12],
                     double xaxis[3]);

/* Seed::CreatePatchesFromPoints (seed.cpp:26-54): ref = nearest camera,
 * normal = unit ray, InitRelatedImages.  Host arrays; computed on the device. */
int dp_seeds_to_patches(dp_ctx *ctx, const double *xyz, int n, dp_patch *out);

/* One objective evaluation per patch at its stored pose: score_out[i] = mean
 * NCC against texture 0 over the visible views (-1 if none). Host arrays. */
int dp_eval_batch(dp_ctx *ctx, const dp_patch *in, int n, int cell, float *score_out);

/* Fused evaluate + refine + filter over a batch (host arrays).  `mode` is a
 * DP_MODE_*; accept_out[i] = 1 if patch i survives (may be NULL).
 * This is the reference's Optimization operator applied to n patches. */
int dp_refine_batch(dp_ctx *ctx, dp_patch *inout, int n, int cell, int mode,
                    uint8_t *accept_out);

/* Same with device-resident arrays, asynchronous on `stream` (hipStream_t,
 * NULL = the context's stream).  Used by bench.py with torch-owned buffers. */
int dp_refine_batch_device(dp_ctx *ctx, dp_patch *d_inout, int n, int cell, int mode,
                           uint8_t *d_accept, void *stream);

/* Expand::ExpandPatch (expand.cpp:103-143) over a batch of parents: child
 * 4*i+d is parent i moved by grid_scale/dx pixels along +x,-x,+y,-y (d=0..3)
 * of the reference view, then Optimize (expand_cell_size, parent's visible
 * set) -> InitRelatedImages -> FilterByErrorMeasurement.  children and
 * accept_out hold 4*n entries.  Parents with fewer than min_expand_visible
 * visible views produce rejected, untouched children (expand.cpp:67). */
int dp_expand_batch(dp_ctx *ctx, const dp_patch *parents, int n, dp_patch *children,
                    uint8_t *accept_out);
int dp_expand_batch_device(dp_ctx *ctx, const dp_patch *d_parents, int n, dp_patch *d_children,
                           uint8_t *d_accept, void *stream);

/* Seeds -> filter+refine (cell 16) -> organizer -> BFS expansion (cell 11):
 * PMVS::Run minus feature matching (pmvs.cpp:22-43).  The returned patch
 * array is owned by the context and valid until the next call/destroy. */
int dp_densify(dp_ctx *ctx, const double *seeds_xyz, int n, const dp_patch **out,
               int64_t *n_out, dp_densify_stats *stats);

/* ---- the same BFS one generation at a time, for sharding it across GPUs ----
 * (SURVEY 8e).  Every rank (one context per GPU) keeps a replicated organizer
 * grid and patch store.  Per generation each rank refines its own items; the
 * candidates of the whole generation reach every rank (an all-gather); every
 * rank then commits the full generation.  Claims are deterministic (owner =
 * lowest sequence number), so every rank's store equals dp_densify's bit for
 * bit.  Host-array form (any binding, no device memory):
 *   dp_densify_begin(ctx, seeds, n, &g)
 *   while (g.items > 0) {
 *     dp_densify_owners(ctx, &g, world, 64, owner, NULL);   the rank of each item
 *     dp_densify_refine_items(ctx, &g, mine, n_mine, my_cands, my_accept);
 *     <all-gather; put every candidate at its generation position
 *      item * per_item + direction>
 *     dp_densify_commit(ctx, &g, all_cands, all_accept, g.items * g.per_item);
 *   }
 *   dp_densify_result(ctx, &out, &n_out, &stats);   evals/refine_ms: this rank's share
 * On one GPU dp_densify_run(ctx, &g, K) runs up to K expansion generations
 * device-resident with one host wait (what dp_densify does after the seed
 * generation). */
typedef struct dp_generation {
    int64_t items;    /* work items: seed points (generation 0) or parents; 0 = finished */
    int64_t head;     /* queue index of the first parent (expansion generations)          */
    int32_t per_item; /* candidates per item: 1 (seed generation) or 4 (ExpandPatch)      */
    int32_t cell;     /* refine window size of this generation                            */
    uint32_t seq0;    /* sequence number of candidate 0                                   */
    int32_t index;    /* 0 = seed generation, then 1, 2, ...                              */
} dp_generation;

int dp_densify_begin(dp_ctx *ctx, const double *seeds_xyz, int n, dp_generation *gen);
/* Organizer step over ALL candidates of the generation (host arrays in item
 * order, n_cand = items * per_item); advances *gen to the next generation. */
int dp_densify_commit(dp_ctx *ctx, dp_generation *gen, const dp_patch *cand, const uint8_t *accept,
                      int64_t n_cand);
int dp_densify_result(dp_ctx *ctx, const dp_patch **out, int64_t *n_out, dp_densify_stats *stats);
/* Up to max_generations expansion generations (gen->index >= 1) on this
 * context alone, device-resident: each generation's refine and organizer read
 * its size from device memory, so they are queued 8 at a time behind ONE host
 * wait; advances *gen (items == 0: finished).  Not with the analytic-gradient
 * performance refine (dp_fast_options.gradient), which is host-driven. */
int dp_densify_run(dp_ctx *ctx, dp_generation *gen, int32_t max_generations);
/* dp_densify_run that also stops BEFORE a generation of yield_items or more
 * items (returned unrun in *gen; 0 = no such stop), and reports in *evals_out
 * (optional) the objective evaluations its refines spent.  The multi-rank
 * densify runs its small generations this way on every rank -- their refine is
 * latency-bound, so partitioning them gains nothing while the exchange costs a
 * host turnaround -- and counts their evaluations on one rank only. */
int dp_densify_run_until(dp_ctx *ctx, dp_generation *gen, int32_t max_generations, int64_t yield_items,
                         int64_t *evals_out);
/* Partitioned generations (north star: "reference-view grid cells shard across
 * the 8 GPUs").  owner_out[i] (host, gen->items) = the rank that
 * refines item i.  Partition spec (round 4; round 3 hashed the tiles and fell
 * back to round robin above 1.1x the mean share):
 *  - key(i) = (ref (TY + 2) + ty + 1) (TX + 2) + tx + 1 (round 6; dense, so
 *    the device sort covers ceil(log2(V (TY + 2) (TX + 2))) bits), from the
 *    item's centre (seed patch or parent) projected into its reference view
 *    (fp64, ((p0 x + p1 y) + p2 z) + p3, one division per coordinate):
 *    ty = floor(v / tile_px), tx = floor(u / tile_px) (NaN or |q| >= 2e9 -> 0),
 *    clamped to [-1, TY] and [-1, TX], TX = ceil(Wmax / tile_px), TY =
 *    ceil(Hmax / tile_px) over the largest view sizes;
 *  - the items stable-sorted by key (ties: ascending item index) -- reference
 *    view, then super-tile row, then column -- and that order cut into `world`
 *    contiguous shares: rank r refines sorted positions [lo_r, lo_{r+1}),
 *    lo_r = floor(r * items / world).  Every share is spatially contiguous and
 *    at most one item above the mean; only the <= world - 1 tiles a cut falls
 *    in are shared by two ranks.
 * Every rank computes the same owners from its replicated store.
 * *fallback_out is always 0 (kept for ABI compatibility).
 * dp_densify_partition_stats: the last partition's {items, world, distinct
 * super-tiles, items in tiles split between two ranks}. */
int dp_densify_owners(dp_ctx *ctx, const dp_generation *gen, int world, int tile_px, int32_t *owner_out,
                      int32_t *fallback_out);
int dp_densify_partition_stats(dp_ctx *ctx, int64_t *stats_out);
int dp_densify_refine_items(dp_ctx *ctx, const dp_generation *gen, const int64_t *items, int64_t n,
                            dp_patch *cand_out, uint8_t *accept_out);
/* The device-resident form with ONE host wait per generation.  Everything is
 * queued on `stream` (NULL = the legacy default stream itself; the context's
 * own stream is joined in), in this order:
 *  - dp_densify_partition_async: the partition of dp_densify_owners as a
 *    rank-major item order on the device (*d_order_out, context-owned, valid
 *    until the next generation) and the shares counts_out[r] = floor((r+1) n /
 *    world) - floor(r n / world) (host, no device read); its statistics
 *    arrive with the commit (dp_densify_partition_stats after it);
 *  - dp_densify_refine_share_async: refines the rank's n items d_items[0..n)
 *    (its slice of *d_order_out) and compacts the candidates whose filter
 *    passed into the rank's exchange SLOT d_slot: record 0 is a header whose
 *    first 8 bytes hold the count (int64), records 1..count the candidates (any
 *    order), each with its generation position (item * per_item + direction)
 *    in `seq`; the slot holds stride + 1 records, stride >= n * per_item;
 *  - the exchange: ONE all-gather of every rank's slot (stride + 1 records
 *    each, stride the same on every rank -- e.g. max_r counts_out[r] *
 *    per_item, host-known);
 *  - dp_densify_commit_gathered_device: scatters the `world` gathered slots at
 *    d_recs (rank r's at d_recs + r * (stride + 1)) to their generation
 *    positions (every other candidate counts as rejected: it claims nothing),
 *    commits the organizer step and reads the generation's status with one
 *    small copy -- the only host wait; *exchanged_out = the records exchanged.
 *    With one rank, pass the rank's own slot (world 1).
 * Every rank's store equals dp_densify's bit for bit. */
int dp_densify_partition_async(dp_ctx *ctx, const dp_generation *gen, int world, int tile_px, void *stream,
                               const int64_t **d_order_out, int64_t *counts_out);
int dp_densify_refine_share_async(dp_ctx *ctx, const dp_generation *gen, const int64_t *d_items, int64_t n,
                                  dp_patch *d_slot, int64_t stride, void *stream);
int dp_densify_commit_gathered_device(dp_ctx *ctx, dp_generation *gen, const dp_patch *d_recs, int64_t stride,
                                      int world, void *stream, int64_t *exchanged_out);

/* ---- patch filter ----------------------------------------
 * PMVS::FilterPatches is declared (methods/pmvs/pmvs.h:27) but never defined
 * and modules/filtering is empty, so this spec follows PMVS (Furukawa & Ponce,
 * PAMI 2010, 3.4).  Every decision of a pass reads a snapshot of the previous
 * pass's survivors (order-independent).  For view v and organizer cell c
 * (grid_scale px, the TryInsert indexing), front(v, c) is the surviving patch
 * with v in its visible set whose (f32 depth, index) is smallest there; depth =
 * third row of P [X;1].  rho(p) = grid_scale / dx(p) (dx as in ExpandPatch);
 * p, q are neighbours iff |(Xq-Xp).np| + |(Xq-Xp).nq| < 2 rho(p) (fp64).
 * V(p) is the set of bits of vis below the context's V: a bit at or beyond V
 * names no view and is ignored, so it counts in neither |V(p)|, the front map
 * nor the 3x3 scan.  ref >= V gives rho(p) = 0 (no neighbours).  A patch is a
 * front candidate of v only where its f32 depth is > 0 and its cell lies in
 * v's grid (W / grid_scale by H / grid_scale whole cells; the coordinate is
 * truncated toward zero, so (-grid_scale, 0) is cell 0); a depth that is <= 0
 * or NaN never fronts a cell but the patch still reads the cell it projects
 * to.  Scores are read as f32 and widened; the two tests are strict fp64
 * comparisons, so a NaN on either side keeps the patch.
 *   DP_FILTER_VISIBILITY: U(p) = { front(v, c_v(p)) : v in V(p) } minus p and
 *     its neighbours (a multiset over views); p is removed iff
 *     |V(p)| * score(p) < sum_{q in U(p)} score(q).
 *   DP_FILTER_NEIGHBORS: over v in V(p) and the 3x3 cells around c_v(p), T =
 *     front patches other than p, M = those that are neighbours of p; p is
 *     removed iff T > 0 and M < min_neighbor_frac * T.
 * keep_out[i] = 1 for survivors.  Multi-GPU: the patch store is replicated on
 * every rank after the generation all-gathers, so each rank filters locally. */
#define DP_FILTER_VISIBILITY 1
#define DP_FILTER_NEIGHBORS 2
typedef struct dp_filter_options {
    int32_t passes;            /* DP_FILTER_* bits (default both)                   */
    int32_t reserved;
    double min_neighbor_frac;  /* 0.25 (PMVS neighbourhood filter)                  */
} dp_filter_options;

void dp_default_filter_options(dp_filter_options *fo);
int dp_filter_patches(dp_ctx *ctx, const dp_patch *patches, int64_t n, const dp_filter_options *fo,
                      uint8_t *keep_out);
int dp_filter_patches_device(dp_ctx *ctx, const dp_patch *d_patches, int64_t n, const dp_filter_options *fo,
                             uint8_t *d_keep, void *stream);

/* ---- iterated expand-filter (PMVS alternates expansion and filtering, three
 * times by default: Furukawa & Ponce, PAMI 2010, 3.3-3.4) ---------------------
 * dp_densify_resume restarts the BFS from an existing patch set
 * (PatchOrganizer::SetSeeds, patch_organizer.cpp:70-75, applied to patches
 * instead of refined seeds):
 *  - offered: patches[i] with keep[i] != 0 (keep NULL = all), in ascending i;
 *  - reset: the organizer grids, the store (emptied), the statistics and
 *    evaluation counters and the pop count;
 *  - insertion: each offered patch goes through TryInsert in that order,
 *    exactly as an accepted candidate of a generation with per_item = 1.  It is
 *    NOT refined again.  A patch that claims at most one cell is dropped and
 *    its claims stay.  A stored record is the input record with seq = its new
 *    store index, parent = 0xFFFFFFFF, flags |= DP_PATCH_ACCEPTED and rgb
 *    recomputed (Patch::ComputeColor); score and evals are kept.  The claims of
 *    patches that are not offered are not carried over: their cells are free;
 *  - *gen = the first expansion generation: index 1, head 0, items = the
 *    stored count (0 if nothing was stored or max_pops <= 0), per_item 4, cell
 *    = expand_cell_size, seq0 = n; stats.seeds_in = n, stats.seed_patches = the
 *    stored count;
 *  - afterwards every generation call works on this state as after a seed
 *    generation (dp_densify_run[_until], dp_densify_owners / _refine_items /
 *    _commit, the _async device protocol, dp_densify_result); performance mode
 *    (dp_fast_options.densify = 1) expands with the fast refine.
 * The device form copies nothing to the host and waits once (the status read;
 * a patch store that has to grow costs one more).  stream NULL = the context's
 * stream.  d_patches may be any device memory INCLUDING the context's own
 * store (the pointer dp_filter_patches_device was given): the patches are
 * staged before the store is reset.  The order and the stored indices do not
 * depend on the launch geometry (the sequence number is the input index). */
int dp_densify_resume(dp_ctx *ctx, const dp_patch *patches, int64_t n, const uint8_t *keep /* NULL = all */,
                      dp_generation *gen);
int dp_densify_resume_device(dp_ctx *ctx, const dp_patch *d_patches, int64_t n, const uint8_t *d_keep,
                             dp_generation *gen, void *stream);

/* The context's patch store on the device: *n records at *d_store (NULL when
 * empty), as the last dp_densify / generation call / dp_densify_resume left
 * it; valid until the next call that changes the store.  For
 * dp_filter_patches_device and dp_densify_resume_device without a host copy. */
int dp_densify_store_device(dp_ctx *ctx, const dp_patch **d_store, int64_t *n);

/* `iterations` (1..16, else DP_E_ARG) rounds of expansion then filter: round 1
 * is dp_densify then dp_filter_patches on its store; round k > 1 is
 * dp_densify_resume_device on the previous store with the previous keep flags,
 * every generation, then the filter (fo NULL = the defaults).  The result is
 * the last store's survivors in store order, records unchanged (patches[keep ==
 * 1]); with iterations == 1 that is dp_densify followed by dp_filter_patches.
 * The store never visits the host between rounds: a round costs the BFS's own
 * waits plus the resume's status read.  *stats sums pops, candidates, evals,
 * generations, stalls and refine_ms over the rounds; stats->patches = *n_out,
 * stats->seed_patches = round 1's.  per_iter[k] (may be NULL): offered = the
 * seed points (k = 0) or the previous round's survivors, reinserted = the
 * patches the organizer stored of them, patches = the store after the BFS,
 * filtered_out = those the filter then removed; total_ms is host time (the
 * filter's device time shows in the next round's, the last includes the copy
 * of the result). */
typedef struct dp_iterate_stats {
    int64_t offered, reinserted, patches, filtered_out, candidates, evals;
    int32_t generations, reserved;
    double refine_ms, filter_ms, total_ms;
} dp_iterate_stats;
int dp_densify_iterate(dp_ctx *ctx, const double *seeds_xyz, int n, int iterations, const dp_filter_options *fo,
                       const dp_patch **out, int64_t *n_out, dp_densify_stats *stats,
                       dp_iterate_stats *per_iter /* iterations entries, may be NULL */);

/* ---- per-view depth / index / normal / score maps of a patch set ------------
 * No reference counterpart (the reference's only product is the point list).
 * Every patch is splatted as an oriented disc in its own plane into the
 * requested views of the CURRENT level (dp_set_level: level-L P, W, H); each
 * pixel keeps the nearest disc.  Every decision is a function of one (patch,
 * view, pixel) alone and the per-pixel resolve is a minimum, so the result
 * does not depend on the patch order or the launch geometry.  All arithmetic is
 * fp64, one IEEE rounding per operation, in exactly the order written (the
 * build has -ffp-contract=off); dot(a, b) = (a0*b0 + a1*b1) + a2*b2 and
 * row_r(P, X) = ((P[4r]*X0 + P[4r+1]*X1) + P[4r+2]*X2) + P[4r+3] throughout;
 * project(P, X) = (row_0 / row_2, row_1 / row_2).
 *
 * Patch p (index i, keep NULL or keep[i] != 0) takes part iff the six floats of
 * pos and normal are finite, ref < V and rho(p) > 0, where rho(p) is the
 * filter's: with rv = view ref, (cu, cv) = project(P_rv, X0), (qu, qv) =
 * project(P_rv, X0 + xr_rv) (componentwise sum), du = qu - cu, dv = qv - cv,
 * dx = sqrt(du*du + dv*dv), rho = dx > 0 ? grid_scale / dx : 0.
 * X0, n = the stored f32 pos, normal widened to fp64 (n is NOT renormalised);
 * R = (double)splat_scale * rho(p).
 *
 * (p, v) is a pair iff, tested in this order,
 *   1. v is requested, and v is in vis(p) -- or, with DP_RENDER_ALL_FACING,
 *      dot(n, d) > 0 for d_k = X0[k] - C_v[k] instead of the vis test (a stored
 *      normal points AWAY from the cameras that see the patch: InitRelatedImages
 *      takes the angle between n and X - C, patch.cpp:36-47);
 *   2. d0 = row_2(P_v, X0) > 0;
 *   3. frame: t = dot(xr_v, n) (xr_v = the view's own camera x-axis,
 *      GetXAxis().normalized()), e1_k = xr_v[k] - t*n[k], s = dot(e1, e1);
 *      skipped unless s >= 1e-12;  e2 = n x e1 (e2_0 = n1*e1_2 - n2*e1_1,
 *      e2_1 = n2*e1_0 - n0*e1_2, e2_2 = n0*e1_1 - n1*e1_0);
 *   4. box: (cu, cv) = project(P_v, X0); skipped unless |cu| < 2e9 and
 *      |cv| < 2e9 (NaN skips); (qu, qv) = project(P_v, X0 + xr_v), dxv =
 *      sqrt(du*du + dv*dv) as above; Bq = (2.0*R)*dxv + 2.0, B = Bq <
 *      (double)max_radius_px ? Bq : (double)max_radius_px; columns x0 =
 *      max(0, floor(cu - B)) .. x1 = min(W - 1, ceil(cu + B)), rows y0, y1 the
 *      same from cv and H; skipped if x0 > x1 or y0 > y1.
 * The box is normative: no pixel outside it is ever covered by the pair.
 *
 * Plane-to-pixel homography H (3x3, rows r = 0..2) and its adjugate:
 *   h[3r] = (P[4r]*e1_0 + P[4r+1]*e1_1) + P[4r+2]*e1_2,  h[3r+1] = the same
 *   with e2,  h[3r+2] = row_r(P_v, X0);
 *   A0 = h4*h8 - h5*h7, A1 = h2*h7 - h1*h8, A2 = h1*h5 - h2*h4,
 *   A3 = h5*h6 - h3*h8, A4 = h0*h8 - h2*h6, A5 = h2*h3 - h0*h5,
 *   A6 = h3*h7 - h4*h6, A7 = h1*h6 - h0*h7, A8 = h0*h4 - h1*h3,
 *   D = (h0*A0 + h1*A3) + h2*A6.
 * Integer pixel (x, y) of the box: a = (A0*x + A1*y) + A2, b = (A3*x + A4*y) +
 * A5, w = (A6*x + A7*y) + A8.  It is covered by the pair iff (w > 0 and D > 0,
 * or w < 0 and D < 0) and (a*a + b*b)*s <= (R*R)*(w*w); its depth is z =
 * (float)(D / w) (the exact ray-plane depth: row 3 of H times A is D e3),
 * accepted iff z > 0.  Per pixel the minimum of key = (f32 bits of z) << 32 | i
 * wins: nearest depth, ties to the lowest patch index (the rule of front()).
 *
 * Outputs, one pointer per requested view in the order of `views`, each
 * row-major W x H of that view at the current level; an array or an entry may
 * be NULL: depth f32 (0 where empty), index int32 (-1), normal 3 x f32 (the
 * winner's stored normal, 0), score f32 (the winner's score, 0).
 * Errors (DP_E_ARG): n < 0 or n > 2^31 - 1, n_views outside 1..V, a view id
 * repeated or >= V, splat_scale not > 0, max_radius_px outside 1..255; no views
 * set: DP_E_STATE.  ro NULL = the defaults.
 * stats (may be NULL), counted on the device: patches taking part, pairs,
 * pixel_tests = the sum of the pairs' box areas, covered_pixels = non-empty
 * pixels after the resolve; render_ms = device time of the call's kernels.
 * The device form takes device patches (the context's own store,
 * dp_densify_store_device, included), device keep flags (the filter's) and
 * device output planes, queues everything on `stream` (NULL = the context's)
 * and waits only when stats != NULL, for the statistics read. */
#define DP_RENDER_ALL_FACING 1
typedef struct dp_render_options {
    float splat_scale;      /* 1.0  disc radius in units of rho(p)                  */
    int32_t max_radius_px;  /* 32   bound of the candidate box half-size (1..255)   */
    int32_t flags;          /* DP_RENDER_* bits (default 0)                         */
} dp_render_options;
typedef struct dp_render_stats {
    int64_t patches, pairs, pixel_tests, covered_pixels;
    double render_ms;
} dp_render_stats;

void dp_default_render_options(dp_render_options *ro);
int dp_render_maps(dp_ctx *ctx, const dp_patch *patches, int64_t n, const uint8_t *keep /* NULL = all */,
                   const int32_t *views, int n_views, const dp_render_options *ro, float *const *depth,
                   int32_t *const *index, float *const *normal, float *const *score, dp_render_stats *stats);
int dp_render_maps_device(dp_ctx *ctx, const dp_patch *d_patches, int64_t n, const uint8_t *d_keep,
                          const int32_t *views, int n_views, const dp_render_options *ro, float *const *d_depth,
                          int32_t *const *d_index, float *const *d_normal, float *const *d_score,
                          dp_render_stats *stats, void *stream);

/* ---- depth-map fusion: per-view depth maps into one cross-view-consistent,
 * oriented, coloured point cloud ------------------------------------------------
 * No reference counterpart (the reference's only product is the point list).
 * Every depth pixel of the requested views is back-projected, observed in every
 * other requested view's depth map, kept when enough of them agree, and written
 * once as the mean of the agreeing back-projections.  All arithmetic is fp64,
 * one IEEE rounding per operation, in exactly the order written (the build has
 * -ffp-contract=off); dot, row_r and project are dp_render_maps's.
 *
 * Inputs: the requested views views[0..K-1] (unique ids < V, 1 <= K <= 64) at
 * the CURRENT level (dp_set_level: level-L P, W, H and BGRA8 planes); per
 * requested view, in the order of `views`, an f32 depth plane W x H, row-major
 * (0 = empty; the value is the projective depth row_2(P_v, X), which is what
 * dp_render_maps writes) and, optionally, a 3 x f32 normal plane (all of them or
 * none: the array pointer NULL = none); the options below.  A plane value z is a
 * depth iff z > 0 and z is finite (0, negatives, NaN and +inf are not).
 *
 * Per requested view v, once on the host in fp64 (the view table): m = the left
 * 3x3 of P_v, m[0..8] = P[0,1,2,4,5,6,8,9,10]; its adjugate A0..A8 by the
 * cofactor formulas dp_render_maps gives for h (with h = m) and det = (m0*A0 +
 * m1*A3) + m2*A6.  A requested view whose det is 0 or not finite: DP_E_ARG.
 *
 * backproject(v, x, y, z): zd = (double)z, b0 = zd*x - P[3], b1 = zd*y - P[7],
 *   b2 = zd - P[11], X_j = ((A[3j]*b0 + A[3j+1]*b1) + A[3j+2]*b2) / det.
 *
 * observe(s, X), of a pixel of view r with normal nr:
 *   1. d = row_2(P_s, X); require d > 0;
 *   2. u = row_0 / d, v = row_1 / d; require |u| < 2e9 and |v| < 2e9 (NaN fails);
 *   3. xi = rint(u), yi = rint(v), round-half-even; require 0 <= xi < W_s and
 *      0 <= yi < H_s;
 *   4. zs = depth_s[yi][xi]; require zs > 0;              -- a MATCHED pair
 *   5. require fabs((double)zs - d) <= (double)depth_tol * d;
 *   6. with normal planes only: ns = normal_s[yi][xi], nr, ns widened to fp64,
 *      c = dot(nr, ns); require c >= 0 and c*c >= (cs*cs) * (dot(nr, nr) *
 *      dot(ns, ns)), cs = (double)min_normal_cos.        -- a CONSISTENT pair
 *
 * Pixel (k, x, y), r = views[k], z = depth_r[y][x], takes part iff z is a depth.
 * X = backproject(r, x, y, z); bit k' of its 64-bit mask is set iff k' != k and
 * observe(views[k'], X) passes; it is FUSABLE iff popcount(mask) >= min_views.
 * A fusable pixel is EMITTED iff DP_FUSE_NO_SUPPRESS is set, or no set bit
 * k' < k of its mask has a matched pixel (k', xi, yi) that is itself fusable
 * (one surface point comes out once, from the first requested view that holds
 * it, instead of once per view).  This is a function of the masks alone, so it
 * does not depend on the launch geometry.
 *
 * Emitted point (dp_fused_point): acc = X; for each set bit k' in ascending
 * order acc_j += backproject(views[k'], xi, yi, zs)_j; m = 1 + popcount(mask);
 * pos_j = (float)(acc_j / (double)m).  With normal planes: sum = nr, then sum_j
 * += ns_j in the same order; q = dot(sum, sum); normal_j = q > 0 ? (float)(sum_j
 * / sqrt(q)) : 0; without them the normal is zeros.  rgb = the R, G, B of view
 * r's BGRA8 texel at (x, y) of the current level; n_views = m; view = r.
 * Order of the output: ascending (k, y, x).
 *
 * Statistics, all counted on the device: depth_pixels (pixels taking part),
 * matched_pairs (observations that pass steps 1-4), consistent_pairs (the sum of
 * popcount(mask)), fusable, emitted; fuse_ms = device time of the call's kernels.
 *
 * Host form: host planes; *out is context-owned, valid until the next
 * dp_fuse_maps or destroy.  Device form: device planes; writes the first
 * min(cap, emitted) points to d_points (may be NULL with cap 0) and nothing
 * beyond them; *n_out = the full emitted count, so a caller sees an overflow;
 * everything is queued on `stream` (NULL = the context's) and the call waits
 * once, for n_out and the statistics.  fo NULL = the defaults; stats may be NULL.
 * Errors (DP_E_ARG): n_views outside 1..min(V, 64), a view id repeated or >= V,
 * depth_tol negative or not finite, min_views outside 0..63, min_normal_cos
 * outside 0..1, depth NULL or a NULL depth entry, a NULL normal entry, cap < 0,
 * cap > 0 without d_points, out or n_out NULL; no views set: DP_E_STATE. */
#define DP_FUSE_NO_SUPPRESS 1
typedef struct dp_fuse_options {
    float depth_tol;       /* 0.01 relative depth agreement                        */
    int32_t min_views;     /* 2    consistent views other than the pixel's own     */
    float min_normal_cos;  /* 0.5  least cosine between agreeing normals           */
    int32_t flags;         /* DP_FUSE_* bits (default 0)                           */
} dp_fuse_options;
typedef struct dp_fused_point {
    float pos[3];
    float normal[3];
    uint8_t rgb[3];
    uint8_t n_views;       /* 1 + the consistent views                             */
    int32_t view, x, y;    /* the emitting pixel                                   */
} dp_fused_point;
typedef struct dp_fuse_stats {
    int64_t depth_pixels, matched_pairs, consistent_pairs, fusable, emitted;
    double fuse_ms;
} dp_fuse_stats;

void dp_default_fuse_options(dp_fuse_options *fo);
int dp_fuse_maps(dp_ctx *ctx, const int32_t *views, int n_views, const dp_fuse_options *fo,
                 const float *const *depth, const float *const *normal /* NULL = none */,
                 const dp_fused_point **out, int64_t *n_out, dp_fuse_stats *stats);
int dp_fuse_maps_device(dp_ctx *ctx, const int32_t *views, int n_views, const dp_fuse_options *fo,
                        const float *const *d_depth, const float *const *d_normal, dp_fused_point *d_points,
                        int64_t cap, int64_t *n_out, dp_fuse_stats *stats, void *stream);

/* ---- depth-map refinement: per-pixel photometric choice among a few candidate
 * planes, with hole filling and a confidence -------------------------------------
 * No reference counterpart.  Every pixel of the requested views builds a short
 * list of candidate planes (its own, a depth sweep of its own, its neighbours'),
 * scores each against a few source views through the performance mode's sampler
 * and keeps the best.  The call reads the input planes only and writes the
 * output planes only (Jacobi), so the result depends on neither pixel order nor
 * launch geometry; feeding the output back in propagates further.  All fp64
 * arithmetic is one IEEE rounding per operation in exactly the order written
 * (-ffp-contract=off); dot, row_r, project are dp_render_maps's, the view table
 * (A, det), backproject and "is a depth" are dp_fuse_maps's.  backproject_d is
 * backproject with an fp64 depth zd in place of (double)z.
 *
 * Inputs: views[0..K-1] (unique ids < V, 1 <= K <= 64) at the CURRENT level;
 * per requested view, in the order of `views`, an f32 depth plane W x H and a
 * 3 x f32 normal plane (both required); the level's P, W, H, the views' C and
 * xr (dp_render_maps's xr_v) and the context's fp16 gray planes (dp_build_gray;
 * built on demand as by the first performance-mode call); gray_v(x, y) is the
 * 8-bit gray of view v.  `sources`: K rows of max_sources view ids, row k the
 * source views of views[k] in order, -1 padded at the end; each id a requested
 * view other than views[k], no repeats.  sources == NULL: row k = the other
 * requested views s by ascending d2 = dot(e, e), e_j = C_s[j] - C_r[j] (ties to
 * the lower view id), the first max_sources of them.
 *
 * Candidates of pixel (k, x, y), r = views[k], z = depth_r[y][x], n =
 * normal_r[y][x] widened to fp64 (never renormalised); a pixel HAS A PLANE iff z
 * is a depth and dot(n, n) > 0.  Candidate indices are fixed:
 *   0            the pixel's own plane: X0 = backproject(r, x, y, z), normal n;
 *                void unless the pixel has a plane;
 *   1..2*sweep   hypotheses h = -sweep..-1, +1..+sweep in this order: (cu, cv) =
 *                project(P_r, X0), (qu, qv) = project(P_r, X0 + xr_r), du = qu -
 *                cu, dv = qv - cv, dx = sqrt(du*du + dv*dv); e_j = X0[j] - C_r[j],
 *                len = sqrt(dot(e, e)); t = ((double)h * (double)step_px) / dx;
 *                the plane through X_h[j] = X0[j] + (t * e_j) / len with normal n;
 *                void unless the pixel has a plane, dx > 0 and len > 0;
 *   then, for each non-zero reach[i] = d in the order i = 0, 1, four indices for
 *                the offsets (-d, 0), (+d, 0), (0, -d), (0, +d): the plane of the
 *                input pixel (x', y') = (x, y) + offset (X0 = backproject(r, x',
 *                y', z'), normal n'); void unless (x', y') is inside the image
 *                and has a plane.  A zero reach takes no indices.
 * The plane (X0, n) as seen from r: m_j = (A[j]*n_0 + A[3+j]*n_1) + A[6+j]*n_2,
 * c = det * dot(n, X0) + dot(m, (P[3], P[7], P[11])); its depth at pixel (u, v):
 * zeta(u, v) = c / ((m_0*u + m_1*v) + m_2), its point there: backproject_d(r, u,
 * v, zeta(u, v)).  zc = zeta(x, y), zf = (float)zc; the candidate is void unless
 * zf is a depth (this rejects NaN, a zero or wrong-signed denominator, overflow).
 *
 * Score of a non-void candidate against source s (W_s, H_s its plane size), with
 * Xc, Xi, Xj the plane's points at (x, y), (x+1, y), (x, y+1):
 *   1. dc = row_2(P_s, Xc), di, dj the same; require dc > 0, di > 0, dj > 0;
 *   2. (uc, vc) = (row_0/dc, row_1/dc) of Xc, (ui, vi), (uj, vj) of Xi, Xj with
 *      their own divisors; U0 = (float)(32.0*uc), V0 = (float)(32.0*vc), Ui =
 *      (float)(32.0*(ui - uc)), Vi = (float)(32.0*(vi - vc)), Uj, Vj the same
 *      from (uj, vj): the first-order window map in 1/32 px;
 *   3. h = (window - 1)/2; for the four corners (i, j) = (+-h, +-h): a = ((double)
 *      U0 + (double)i*(double)Ui) + (double)j*(double)Uj, b the same from V;
 *      require 0 <= a <= 32*(W_s - 1) and 0 <= b <= 32*(H_s - 1) (NaN fails);
 *      otherwise the source is INVALID for this candidate;
 *   4. sample (i, j), i, j = -h..h, exactly as the performance mode's: in fp32,
 *      U = fmaf((float)j, Uj, fmaf((float)i, Ui, U0)) + 8388608.0f, clamped to
 *      [8388608, 8388608 + 32*(W_s - 1)], iu = (int)(U - 8388608.0f), xs = iu >>
 *      5, fx = iu & 31; yv, fy the same from V and H_s; the taps p00 = gray_s(xs,
 *      yv), p01 = gray_s(min(xs+1, W_s-1), yv), p10 = gray_s(xs, min(yv+1,
 *      H_s-1)), p11; b = ((32-fx)*(32-fy)*p00 + fx*(32-fy)*p01 + (32-fx)*fy*p10
 *      + fx*fy*p11 + 32) >> 6, in 1/16 gray levels;
 *   5. the reference sample a = 16 * gray_r(clamp(x+i, 0, W_r-1), clamp(y+j, 0,
 *      H_r-1));
 *   6. exact integer moments over the N = window^2 samples: Sa, Saa, Sb, Sbb,
 *      Sab; num = N*Sab - Sa*Sb, va = N*Saa - Sa*Sa, vb = N*Sbb - Sb*Sb (exact
 *      integers, each below 2^53); den = sqrt((double)va * (double)vb), dmin =
 *      ((ncc_denom_min * 256.0) * N) * N (dp_options.ncc_denom_min, the floor of
 *      DP_MODE_FAST_EVAL in these units); ncc = (double)num / (den > dmin ? den
 *      : dmin).
 * Candidate score: the ncc of its valid sources, sorted descending (equal values
 * in source-list order), S = the first, S = S + the next, ... over the first
 * top_k of them, score = S / (double)top_k.  With fewer than top_k valid sources
 * the candidate is void.
 *
 * Selection: the non-void candidate of the greatest score wins, ties to the
 * lowest index.  If score >= (double)min_ncc the pixel is KEPT: depth = zf of
 * the winner, normal = the winner's stored f32 normal, score = (float)score,
 * choice = its index.  Otherwise the pixel is empty: depth 0, normal 0, score 0,
 * choice -1.  With DP_MAPREF_KEEP_UNSCORED a pixel whose z is a depth and that
 * has no non-void candidate keeps its input depth and normal (bit for bit) with
 * score 0 and choice -2.
 *
 * Outputs: per requested view depth f32, normal 3 x f32, score f32, choice int32
 * planes; an array or an entry may be NULL.  Statistics, counted on the device:
 * depth_pixels_in (pixels whose z is a depth), candidates (non-void), source_scores
 * ((candidate, valid source) pairs scored, of candidates not void by their
 * plane), kept, filled (kept, z not a depth), moved (kept, choice != 0);
 * refine_ms = device time of the call's kernel.
 * Host form: host planes.  Device form: device planes, everything queued on
 * `stream` (NULL = the context's); it waits only for the statistics read, and
 * not at all with stats == NULL.  mo NULL = the defaults, which are design
 * choices that nobody has tuned.
 * Errors (DP_E_ARG): window even or outside 3..11, sweep outside 0..8, step_px
 * not > 0 or not finite, a reach outside 0..16, max_sources outside 1..8, top_k
 * outside 1..max_sources, min_ncc outside -1..1, unknown flag bits; n_views
 * outside 1..min(V, 64), a view id repeated or >= V, a singular left 3x3; a
 * sources row with an id that is not requested, the row's own, repeated, below
 * -1, or after a -1; depth or normal NULL or a NULL entry; an output plane
 * pointer equal to an input plane pointer; no views set: DP_E_STATE. */
#define DP_MAPREF_KEEP_UNSCORED 1
typedef struct dp_mapref_options {
    int32_t window;       /* 7    side of the scored window, reference pixels (odd, 3..11) */
    int32_t sweep;        /* 2    depth hypotheses on each side of the own plane (0..8)    */
    float step_px;        /* 1.0  sweep step in reference-pixel footprints (> 0)           */
    int32_t reach[2];     /* 1, 4 distances of the propagation offsets (0..16, 0 = off)   */
    int32_t max_sources;  /* 4    source views per reference view (1..8)                   */
    int32_t top_k;        /* 2    best sources averaged into a score (1..max_sources)      */
    float min_ncc;        /* 0.5  least score for a pixel to be kept (-1..1)               */
    int32_t flags;        /* DP_MAPREF_* bits (default 0)                                  */
} dp_mapref_options;
typedef struct dp_mapref_stats {
    int64_t depth_pixels_in, candidates, source_scores, kept, filled, moved;
    double refine_ms;
} dp_mapref_stats;

void dp_default_mapref_options(dp_mapref_options *mo);
int dp_refine_maps(dp_ctx *ctx, const int32_t *views, int n_views, const dp_mapref_options *mo,
                   const int32_t *sources /* NULL = nearest */, const float *const *depth,
                   const float *const *normal, float *const *depth_out, float *const *normal_out,
                   float *const *score_out, int32_t *const *choice_out, dp_mapref_stats *stats);
int dp_refine_maps_device(dp_ctx *ctx, const int32_t *views, int n_views, const dp_mapref_options *mo,
                          const int32_t *sources, const float *const *d_depth, const float *const *d_normal,
                          float *const *d_depth_out, float *const *d_normal_out, float *const *d_score_out,
                          int32_t *const *d_choice_out, dp_mapref_stats *stats, void *stream);

/* ---- TSDF volume and triangle mesh: per-view depth maps integrated into one
 * dense truncated-signed-distance volume, and its zero surface extracted by
 * marching tetrahedra -----------------------------------------------------------
 * No reference counterpart (modules/surface/ is an empty stub).  One dense
 * volume per call: nothing is accumulated between calls.  All fp64 arithmetic is
 * one IEEE rounding per operation in exactly the order written
 * (-ffp-contract=off); dot, row_r and project are dp_render_maps's; "is a depth"
 * and the rules of the requested views (unique ids < V, 1 <= K <= 64, the CURRENT
 * level's P, W, H and BGRA8 planes) are dp_fuse_maps's.
 *
 * The volume (dp_tsdf_options): nx x ny x nz voxels of side `voxel`, the low
 * corner of voxel (0, 0, 0) at `origin`; every plane of it is [nz][ny][nx], x
 * fastest.  The centre of voxel idx = (i, j, k) is X_a = (double)origin[a] +
 * ((double)idx_a + 0.5) * (double)voxel, a = 0, 1, 2.
 *
 * dp_tsdf_integrate.  Per requested view v, once on the host in fp64: m2 =
 * (P[8], P[9], P[10]), g_v = sqrt(dot(m2, m2)); g_v not finite or not > 0:
 * DP_E_ARG.  Dividing a projective depth difference by g_v makes it a distance
 * along the optical axis, so `trunc` is in world units whatever the scale of P.
 * Voxel (i, j, k), X its centre: tsum = 0.0, w = 0, integers sr = sg = sb = 0;
 * then for the requested views in the order of `views`:
 *   1. d = row_2(P_v, X); require d > 0;
 *   2. u = row_0 / d, v = row_1 / d; require |u| < 2e9 and |v| < 2e9 (NaN fails);
 *      xi = rint(u), yi = rint(v), round-half-even; require 0 <= xi < W_v and
 *      0 <= yi < H_v                      -- steps 2-3 of dp_fuse_maps's observe;
 *   3. z = depth_v[yi][xi]; require that z is a depth;
 *   4. sdf = ((double)z - d) / g_v;
 *   5. if sdf < -(double)trunc the view does not count (the voxel is occluded);
 *   6. otherwise t = sdf >= (double)trunc ? 1.0 : sdf / (double)trunc, tsum =
 *      tsum + t, w += 1, and sr, sg, sb add the R, G, B of the BGRA8 texel (xi,
 *      yi) of view v at the current level.
 * Outputs: weight = w; tsdf = w > 0 ? (float)(tsum / (double)w) : 1.0f; rgb = w >
 * 0 ? R | G << 8 | B << 16, each channel (s + w/2) / w in integers : 0.  One
 * voxel's result is a function of the voxel alone, the views walked in order: it
 * depends on neither the launch geometry nor on atomics.  An output pointer may
 * be NULL.  Statistics, counted on the device: voxels, observations (the sum of
 * w), observed_voxels (w > 0), near_voxels (w > 0 and fabsf(tsdf) < 1);
 * integrate_ms = device time of the call's kernel.
 * Host form: host planes and host outputs.  Device form: device planes and
 * outputs, everything queued on `stream` (NULL = the context's); it waits only
 * for the statistics read, and not at all with stats == NULL.
 *
 * dp_tsdf_mesh.  Inputs: the tsdf, weight and (optionally, NULL = vertex colour
 * 0) rgb planes of a volume described by `opts`; tsdf values are expected to be
 * finite (the integration writes [-1, 1] only): a vertex of an edge with a NaN
 * or infinite end has an unspecified position and colour, nothing else changes.
 * Lattice point p = (i, j, k) sits at the centre of voxel p.  A point is INSIDE
 * iff tsdf < 0 (0, -0, 1 and NaN are outside).  Cell (i, j, k), 0 <= i < nx - 1,
 * 0 <= j < ny - 1, 0 <= k < nz - 1, has the corners p + {0,1}^3 and is ACTIVE iff
 * all eight have weight >= min_weight.
 * Kuhn split: every cell is cut into six tetrahedra, one per permutation (a, b,
 * c) of the axes (0, 1, 2) in lexicographic order (012, 021, 102, 120, 201,
 * 210); tetrahedron (a, b, c) has the corners q0 = p, q1 = p + e_a, q2 = p + e_a
 * + e_b, q3 = p + (1, 1, 1).  The split is the same in every cell, so
 * neighbouring cells agree on their common faces and the mesh is watertight
 * wherever active cells meet.  An edge (q_m, q_n), m < n, of a tetrahedron runs
 * from the lattice point q_m in the direction q_n - q_m, one of (1,0,0) (0,1,0)
 * (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), numbered dir = 0..6 in this order.
 * Edge (p, dir) CARRIES A VERTEX iff its ends differ in INSIDE and at least one
 * ACTIVE cell has both ends among its corners.  Vertices are numbered in
 * ascending (k, j, i, dir).  With A at p, B at p + dir, a, b their tsdf widened
 * to fp64 and ca, cb a colour channel of their rgb words: s = a / (a - b), pos_c
 * = (float)(XA_c + s * (XB_c - XA_c)), channel = (uint8)rint((double)ca + s *
 * ((double)cb - (double)ca)); pad = 0.
 * Triangles: each tetrahedron of an active cell emits the triangles of its 4-bit
 * inside mask (bit m set iff q_m is INSIDE), each corner the vertex of the named
 * edge "mn" = (q_m, q_n).  For an EVEN permutation (012, 120, 201):
 *    1: 01 02 03           2: 01 13 12           4: 02 12 23
 *    8: 03 23 13           7: 03 13 23          11: 02 23 12
 *   13: 01 12 13          14: 01 03 02
 *    3: 02 03 13, 02 13 12         5: 01 23 03, 01 12 23
 *    6: 01 13 23, 01 23 02         9: 01 02 23, 01 23 13
 *   10: 01 23 12, 01 03 23        12: 02 12 13, 02 13 03
 * and nothing for 0 and 15; for an ODD permutation (021, 102, 210) the second
 * and third corner of every triangle are exchanged.  The rule reads the
 * permutation and the mask only, never a coordinate; with it cross(v1 - v0, v2 -
 * v0) points from inside to outside, which is towards the cameras.  A triangle
 * is three vertex numbers (int32).  Order: ascending cell (k, j, i), then
 * tetrahedron, then triangle.  Zero-area triangles are kept (a tsdf of exactly 0
 * puts a vertex on a lattice point).
 * Statistics, counted on the device: active_cells, vertices, triangles; mesh_ms
 * = device time of the call's kernels.
 * Host form: host planes; *vertices and *triangles are context-owned, valid until
 * the next dp_tsdf_mesh or destroy (NULL when the count is 0).  Device form:
 * device planes; writes the first min(vertex_cap, vertices) vertices and the
 * first min(triangle_cap, triangles) triangles and nothing beyond them (a buffer
 * may be NULL with cap 0); *n_vertices and *n_triangles are the full counts, so a
 * caller sees an overflow; everything is queued on `stream` (NULL = the
 * context's) and the call waits once, for the counts.  stats may be NULL.
 *
 * Errors (DP_E_ARG): opts NULL, an origin, voxel or trunc that is not finite,
 * voxel or trunc not > 0, a dim outside 2..1024, nx*ny*nz > 2^30, min_weight
 * outside 1..64, flags != 0; a NULL input plane or array; for the integration
 * the view rules above and a g_v as above; for the mesh a NULL count or result
 * pointer, a negative cap, a cap > 0 without its buffer, and a volume whose mesh
 * has more than 2^31 - 1 vertices or triangles.  No views set, for the
 * integration: DP_E_STATE (the mesh reads no view). */
typedef struct dp_tsdf_options {
    float origin[3];     /* world position of the volume's low corner (no default)      */
    float voxel;         /* voxel side, world units (> 0, finite; no default)           */
    int32_t dim[3];      /* nx, ny, nz: each 2..1024, nx*ny*nz <= 2^30 (no default)     */
    float trunc;         /* truncation distance, world units (> 0, finite; no default)  */
    int32_t min_weight;  /* 1  least observations for a voxel to take part in the mesh (1..64) */
    int32_t flags;       /* none defined; non-zero is DP_E_ARG                          */
} dp_tsdf_options;
typedef struct dp_mesh_vertex {
    float pos[3];
    uint8_t rgb[3];
    uint8_t pad;         /* 0 */
} dp_mesh_vertex;
typedef struct dp_tsdf_stats {
    int64_t voxels, observations, observed_voxels, near_voxels;
    double integrate_ms;
} dp_tsdf_stats;
typedef struct dp_mesh_stats {
    int64_t active_cells, vertices, triangles;
    double mesh_ms;
} dp_mesh_stats;

/* min_weight = 1, flags = 0, everything else 0: an unfilled struct is rejected */
void dp_default_tsdf_options(dp_tsdf_options *to);
int dp_tsdf_integrate(dp_ctx *ctx, const int32_t *views, int n_views, const dp_tsdf_options *opts,
                      const float *const *depth, float *tsdf, int32_t *weight, uint32_t *rgb, dp_tsdf_stats *stats);
int dp_tsdf_integrate_device(dp_ctx *ctx, const int32_t *views, int n_views, const dp_tsdf_options *opts,
                             const float *const *d_depth, float *d_tsdf, int32_t *d_weight, uint32_t *d_rgb,
                             dp_tsdf_stats *stats, void *stream);
int dp_tsdf_mesh(dp_ctx *ctx, const dp_tsdf_options *opts, const float *tsdf, const int32_t *weight,
                 const uint32_t *rgb /* NULL: vertex colour 0 */, const dp_mesh_vertex **vertices,
                 int64_t *n_vertices, const int32_t **triangles, int64_t *n_triangles, dp_mesh_stats *stats);
int dp_tsdf_mesh_device(dp_ctx *ctx, const dp_tsdf_options *opts, const float *d_tsdf, const int32_t *d_weight,
                        const uint32_t *d_rgb, dp_mesh_vertex *d_vertices, int64_t vertex_cap, int64_t *n_vertices,
                        int32_t *d_triangles, int64_t triangle_cap, int64_t *n_triangles, dp_mesh_stats *stats,
                        void *stream);

/* ---- mesh clean-up: the connected components of a triangle mesh, and the mesh
 * without its small components --------------------------------------------------
 * No reference counterpart.  A mesh of real depth maps is the surface plus a
 * cloud of small closed "floaters" wherever a few wrong depth pixels agreed in
 * min_weight views; this labels the components and drops the small ones.  Every
 * quantity is an integer or a byte copy; the only floating-point operation is
 * the one comparison with min_fraction.  Neither call reads a view, so a
 * context without dp_set_views works.
 *
 * Inputs: n_triangles triangles of three int32 vertex indices each, over
 * n_vertices vertices (dp_mesh_clean also reads the 16-byte vertex records).
 * A triangle is VALID iff its three indices lie in [0, n_vertices).  An invalid
 * triangle joins nothing, has component -1, is never written, and counts in
 * invalid_triangles; its indices are never used as an address.  A triangle with
 * repeated indices is valid.
 * A vertex is USED iff a valid triangle names it.  Every valid triangle (a, b, c)
 * joins a, b and c; label(v) is the smallest vertex index in v's connected set.
 * So two triangles that share only one vertex are in one component (vertex
 * connectivity: it needs no edge table, and it never splits what marching
 * tetrahedra emitted as one surface).
 * Components: a component's root is its label; components are numbered 0..C-1
 * by ascending root.  vertex_component[v] = that number, or -1 for an unused
 * vertex; triangle_component[t] = the number of its first index's component, or
 * -1 for an invalid triangle.  Table row c (dp_mesh_component) holds root,
 * vertices (the used vertices of c), triangles T_c and rank; rank(c) = the number
 * of components c' with T_c' > T_c, or with T_c' = T_c and c' < c.
 * Selection (dp_mesh_clean_options): Tmax = max T_c (largest_triangles; 0 when
 * C = 0).  c is KEPT iff T_c >= min_triangles, and (double)T_c >=
 * (double)min_fraction * (double)Tmax, and max_components = 0 or rank(c) <
 * max_components.
 * Clean output: the kept vertices are the used vertices of kept components, in
 * ascending input order, each 16-byte record copied byte for byte (the pad byte
 * included); the kept triangles are the valid triangles of kept components, in
 * input order, their indices remapped to the new numbering.  vertex_map[v] and
 * triangle_map[t] hold the new index, or -1.  Hence the result of a clean,
 * cleaned again with the same options, is itself.
 * The labels are minima and the counts are integers, so nothing depends on the
 * order in which lanes or blocks run.
 * Statistics: vertices_in, triangles_in (the counts given), invalid_triangles,
 * unused_vertices, components = C, largest_triangles = Tmax, components_kept,
 * vertices_out, triangles_out; clean_ms = device time of the call's kernels.
 * dp_mesh_components selects nothing: it reports components_kept = C,
 * vertices_out = the used vertices and triangles_out = the valid triangles.
 *
 * Host form: host arrays; vertex_component / triangle_component and vertex_map /
 * triangle_map are the caller's (n_vertices / n_triangles int32, may be NULL);
 * *components, *vertices_out and *triangles_out are context-owned, valid until
 * the next call of the same function or destroy, and NULL when their count is 0.
 * Device form: device arrays (the output of dp_tsdf_mesh_device is the intended
 * input); one cap per output buffer: the first min(cap, count) records are
 * written and nothing beyond them (a buffer may be NULL with cap 0); the counts
 * returned are the full counts, so a caller sees an overflow; everything is
 * queued on `stream` (NULL = the context's) and the call waits once, for the
 * counts and statistics.  mco NULL = the defaults; stats may be NULL.
 * Errors (DP_E_ARG): a negative count or a count above 2^31 - 1; a NULL input
 * with a non-zero count; min_triangles < 0; min_fraction outside 0..1 or NaN;
 * max_components < 0; flags != 0; a NULL count (or, host form, result) pointer;
 * a negative cap, or a cap > 0 without its buffer; an output pointer equal to an
 * input pointer.  n_triangles = 0 or n_vertices = 0 is legal and yields empty
 * results. */
typedef struct dp_mesh_clean_options {
    int64_t min_triangles;   /* 1    least triangles of a kept component (>= 0)             */
    float   min_fraction;    /* 0    least share of the largest component's triangles (0..1) */
    int32_t max_components;  /* 0    0 = no limit, else keep only the first so many by rank  */
    int32_t flags;           /* none defined; non-zero is DP_E_ARG                           */
    int32_t reserved;
} dp_mesh_clean_options;
typedef struct dp_mesh_component {
    int32_t root, vertices, triangles, rank;
} dp_mesh_component;
typedef struct dp_mesh_clean_stats {
    int64_t vertices_in, triangles_in, invalid_triangles, unused_vertices, components, largest_triangles,
        components_kept, vertices_out, triangles_out;
    double clean_ms;
} dp_mesh_clean_stats;

void dp_default_mesh_clean_options(dp_mesh_clean_options *mco);
int dp_mesh_components(dp_ctx *ctx, const int32_t *triangles, int64_t n_triangles, int64_t n_vertices,
                       int32_t *vertex_component, int32_t *triangle_component, const dp_mesh_component **components,
                       int64_t *n_components, dp_mesh_clean_stats *stats);
int dp_mesh_components_device(dp_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices,
                              int32_t *d_vertex_component, int32_t *d_triangle_component,
                              dp_mesh_component *d_components, int64_t component_cap, int64_t *n_components,
                              dp_mesh_clean_stats *stats, void *stream);
int dp_mesh_clean(dp_ctx *ctx, const dp_mesh_clean_options *mco, const dp_mesh_vertex *vertices, int64_t n_vertices,
                  const int32_t *triangles, int64_t n_triangles, const dp_mesh_vertex **vertices_out,
                  int64_t *n_vertices_out, const int32_t **triangles_out, int64_t *n_triangles_out,
                  int32_t *vertex_map, int32_t *triangle_map, dp_mesh_clean_stats *stats);
int dp_mesh_clean_device(dp_ctx *ctx, const dp_mesh_clean_options *mco, const dp_mesh_vertex *d_vertices,
                         int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                         dp_mesh_vertex *d_vertices_out, int64_t vertex_cap, int64_t *n_vertices_out,
                         int32_t *d_triangles_out, int64_t triangle_cap, int64_t *n_triangles_out,
                         int32_t *d_vertex_map, int32_t *d_triangle_map, dp_mesh_clean_stats *stats, void *stream);

/* ---- mesh adjacency, Taubin smoothing and vertex normals -----------------------
 * No reference counterpart.  The mesh of dp_tsdf_mesh is terraced (every vertex
 * sits on a lattice edge), carries the depth maps' noise and has no normals;
 * these three calls build the adjacency of a triangle mesh, relax its vertex
 * positions and give every vertex an area-weighted normal.  None reads a view.
 * Every result is independent of the order in which lanes or blocks run: the
 * integer part is counts and sorted sets, every float sum runs over a sorted
 * row in a fixed order, and there is no floating-point atomic.  Every fp64
 * expression below is one IEEE rounding per operation (no contraction), dvdiv
 * and dvsqrt are the IEEE-correct fp64 quotient and square root, (float) and
 * (double) are the IEEE conversions (round to nearest even).
 *
 * Definitions.  A triangle is VALID as in the clean-up section (three indices in
 * [0, n_vertices)), DEGENERATE iff it is valid and two of its indices are equal,
 * PROPER iff it is valid and not degenerate.  Only proper triangles take part in
 * anything below; invalid and degenerate triangles are counted
 * (invalid_triangles, degenerate_triangles) and their indices are never used as
 * an address before the range check.  A proper triangle (a, b, c) puts b and c
 * into N(a), a and c into N(b), a and b into N(c); N(v) is a set.  count(u, v) is
 * the number of proper triangles that name both u and v.  Edge {u, v} is a
 * BOUNDARY edge iff count = 1 and NONMANIFOLD iff count > 2.  Vertex flag byte:
 * bit 0 (DP_VERTEX_BOUNDARY) set iff some incident edge is a boundary edge, bit 1
 * (DP_VERTEX_NONMANIFOLD) set iff some incident edge is nonmanifold.
 *
 * dp_mesh_adjacency.  offsets: int32, n_vertices + 1 entries, offsets[0] = 0;
 * row v is [offsets[v], offsets[v + 1]).  neighbours: int32, row v holds N(v) in
 * ascending order.  edge_triangles: int32, parallel to neighbours, entry e of row
 * v holds count(v, neighbours[e]).  vertex_flags: uint8, n_vertices entries.  The
 * entry count E = offsets[n_vertices] is returned in *n_entries.  Statistics:
 * vertices_in, triangles_in, invalid_triangles, degenerate_triangles,
 * isolated_vertices (empty rows), edges = E / 2, boundary_edges,
 * nonmanifold_edges, boundary_vertices (bit 0 set), max_valence (the longest
 * row), adjacency_ms = device time of the call's kernels.
 * Host form: any of the four result pointers may be NULL (not wanted); the
 * arrays are context-owned, valid until the next dp_mesh_adjacency or destroy.
 * Device form: any of the four buffers may be NULL; d_offsets and
 * d_vertex_flags are written whole, d_neighbours / d_edge_triangles get the
 * first min(entry_cap, E) entries and nothing beyond them; *n_entries is the
 * full E, so a caller sees an overflow; everything is queued on `stream` (NULL =
 * the context's) and the call waits once, for the counts.
 *
 * dp_mesh_smooth (dp_mesh_smooth_options; defaults are Taubin's lambda | mu
 * pair, a design choice that nobody has tuned for this pipeline).  One STEP with
 * factor f (the option widened to fp64) reads the previous step's positions only
 * (Jacobi).  Vertex v is MOVABLE iff its row is non-empty and it is not pinned;
 * pinned means bit 0 is set and DP_SMOOTH_FREE_BOUNDARY is not given.  For a
 * movable v with n = |N(v)| and each coordinate c:
 *   S = 0.0;  for j in row v, ascending:  S = S + (double)pos_j[c]
 *   m = dvdiv(S, (double)n);  x = (double)pos_v[c];  new = (float)(x + f * (m - x))
 * Other vertices keep their bits.  One iteration is a lambda step, then a mu
 * step if mu != 0; positions are fp32 between steps.  The output is the input's
 * 16-byte records with pos replaced, rgb and pad copied byte for byte; triangles
 * are untouched, so the adjacency is built once per call.  iterations = 0
 * copies.  Positions are expected to be finite.  Statistics: the adjacency's
 * integer counts, movable_vertices, pinned_vertices, steps (launched),
 * adjacency_ms, smooth_ms.
 * Host form: *vertices_out is context-owned (valid until the next dp_mesh_smooth
 * or destroy, NULL when n_vertices = 0).  Device form: d_vertices_out holds
 * n_vertices records and must differ from d_vertices; all steps are queued
 * behind one another on `stream` with no host wait between them; one wait at
 * the end for the statistics, none when stats is NULL.
 *
 * dp_mesh_normals.  normal[v] (3 floats): walk the proper triangles that name v
 * in ascending triangle index; for each such triangle (i0, i1, i2) with
 * positions p0, p1, p2 (whichever of them v is):
 *   e1 = (double)p1 - (double)p0,  e2 = (double)p2 - (double)p0   (componentwise)
 *   g = (e1y*e2z - e1z*e2y,  e1z*e2x - e1x*e2z,  e1x*e2y - e1y*e2x)
 *   s = s + g   (componentwise, s starts at 0.0)
 * then l2 = (s.x*s.x + s.y*s.y) + s.z*s.z; if !(l2 > 0) or l2 is not finite the
 * normal is (0, 0, 0) and counts in zero_normals, else normal_c =
 * (float)dvdiv(s_c, dvsqrt(l2)).  With dp_tsdf_mesh's winding the normals point
 * from inside (tsdf < 0) to outside.  The sum follows the triangle order, so the
 * same mesh with its triangles reordered may give normals that differ in the
 * last bits.  Statistics: vertices_in, triangles_in, invalid_triangles,
 * degenerate_triangles, zero_normals, normals_ms.  Host form: *normals is
 * context-owned (until the next dp_mesh_normals or destroy, NULL when n_vertices
 * = 0).  Device form: d_normals holds 3 * n_vertices floats; one wait for the
 * statistics, none when stats is NULL.
 *
 * Errors (DP_E_ARG), counts before pointers: the clean-up section's list (counts,
 * NULL inputs, an output pointer equal to an input pointer, a negative cap), and
 * for dp_mesh_adjacency and dp_mesh_smooth 6 * n_triangles > 2^31 - 1 (offsets
 * are int32) and for dp_mesh_normals 3 * n_triangles > 2^31 - 1 (its pairs are
 * counted in int32); iterations outside 0..1000; lambda outside (0, 1] or NaN; mu > 0 or
 * NaN or infinite; unknown flag bits; a NULL n_entries or (host form) result
 * pointer of dp_mesh_smooth / dp_mesh_normals; (device form) a NULL output of
 * dp_mesh_smooth / dp_mesh_normals with n_vertices > 0. */
#define DP_VERTEX_BOUNDARY 1
#define DP_VERTEX_NONMANIFOLD 2
#define DP_SMOOTH_FREE_BOUNDARY 1
typedef struct dp_mesh_smooth_options {
    int32_t iterations;  /* 10     lambda (| mu) iterations, 0..1000                     */
    float   lambda;      /* 0.5    the shrinking step's factor, in (0, 1]                */
    float   mu;          /* -0.53  the inflating step's factor, <= 0; 0 = plain Laplacian */
    int32_t flags;       /* DP_SMOOTH_FREE_BOUNDARY: boundary vertices move too          */
    int32_t reserved;
} dp_mesh_smooth_options;
typedef struct dp_mesh_adjacency_stats {
    int64_t vertices_in, triangles_in, invalid_triangles, degenerate_triangles, isolated_vertices, edges,
        boundary_edges, nonmanifold_edges, boundary_vertices, max_valence;
    double adjacency_ms;
} dp_mesh_adjacency_stats;
typedef struct dp_mesh_smooth_stats {
    int64_t vertices_in, triangles_in, invalid_triangles, degenerate_triangles, isolated_vertices, edges,
        boundary_edges, nonmanifold_edges, boundary_vertices, max_valence, movable_vertices, pinned_vertices, steps;
    double adjacency_ms, smooth_ms;
} dp_mesh_smooth_stats;
typedef struct dp_mesh_normals_stats {
    int64_t vertices_in, triangles_in, invalid_triangles, degenerate_triangles, zero_normals;
    double normals_ms;
} dp_mesh_normals_stats;

void dp_default_mesh_smooth_options(dp_mesh_smooth_options *mso);
int dp_mesh_adjacency(dp_ctx *ctx, const int32_t *triangles, int64_t n_triangles, int64_t n_vertices,
                      const int32_t **offsets, const int32_t **neighbours, const int32_t **edge_triangles,
                      const uint8_t **vertex_flags, int64_t *n_entries, dp_mesh_adjacency_stats *stats);
int dp_mesh_adjacency_device(dp_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices,
                             int32_t *d_offsets, int32_t *d_neighbours, int32_t *d_edge_triangles, int64_t entry_cap,
                             uint8_t *d_vertex_flags, int64_t *n_entries, dp_mesh_adjacency_stats *stats, void *stream);
int dp_mesh_smooth(dp_ctx *ctx, const dp_mesh_smooth_options *mso, const dp_mesh_vertex *vertices, int64_t n_vertices,
                   const int32_t *triangles, int64_t n_triangles, const dp_mesh_vertex **vertices_out,
                   dp_mesh_smooth_stats *stats);
int dp_mesh_smooth_device(dp_ctx *ctx, const dp_mesh_smooth_options *mso, const dp_mesh_vertex *d_vertices,
                          int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                          dp_mesh_vertex *d_vertices_out, dp_mesh_smooth_stats *stats, void *stream);
int dp_mesh_normals(dp_ctx *ctx, const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                    int64_t n_triangles, const float **normals, dp_mesh_normals_stats *stats);
int dp_mesh_normals_device(dp_ctx *ctx, const dp_mesh_vertex *d_vertices, int64_t n_vertices, const int32_t *d_triangles,
                           int64_t n_triangles, float *d_normals, dp_mesh_normals_stats *stats, void *stream);

/* ---- mesh simplification: vertex clustering on a uniform grid -------------------
 * No reference counterpart.  The mesh of dp_tsdf_mesh is never coarser than the
 * TSDF lattice, whatever the surface's detail; this merges the vertices of every
 * cell of a coarser lattice into one (Rossignac-Borrel), placed at their mean or
 * (DP_DECIMATE_QUADRIC) where the planes of the cell's triangles meet (Lindstrom
 * 2000), and drops the triangles that collapse or repeat.  No view is read.  The
 * result does not depend on the order in which lanes or blocks run: clusters and
 * triangles are sorted sets, every float sum runs over a sorted run in a fixed
 * order, and there is no floating-point atomic.  Every fp64 expression below is
 * one IEEE rounding per operation (no contraction), dvdiv is the IEEE-correct
 * fp64 quotient, (float) and (double) are the IEEE conversions.
 *
 * Definitions.  VALID, DEGENERATE and PROPER triangles are as in the smoothing
 * section; only proper triangles take part, invalid and degenerate ones are
 * counted (invalid_triangles, degenerate_triangles), and no index is used as an
 * address before its range check.  A vertex is USED iff a proper triangle names
 * it (unused_vertices counts the others).
 * Cell of a position p (also the quadric's acceptance test below), per axis c:
 *   q = floor(dvdiv((double)p[c] - (double)origin[c], (double)cell))
 *   k_c = -2^20 if !(q >= -2^20) (a NaN too), 2^20 - 1 if q > 2^20 - 1, else (int64)q
 * A used vertex with any axis changed by these bounds counts in clamped_vertices.
 * Cells are ordered by (k_z, k_y, k_x) ascending.
 * Clusters.  A cluster is the set of used vertices of one cell, its members taken
 * in ascending vertex index; clusters are numbered 0..K-1 by ascending cell;
 * clusters = K, max_cluster = the largest member count.
 * Triangles.  A proper triangle (a, b, c) maps to the clusters (A, B, C) of its
 * indices.  It is COLLAPSED iff two of them are equal: dropped, counted in
 * collapsed_triangles.  Otherwise its canonical triple is the rotation of
 * (A, B, C) that puts the smallest first (the cyclic order, and so the
 * orientation, is kept), and it is a DUPLICATE iff a non-collapsed triangle of
 * lower index has the same canonical triple: dropped, counted in
 * duplicate_triangles.  Oppositely wound triples are different triples: both
 * stay.  The kept triangles come out in input order, their indices in their
 * positions (not rotated), each replaced by its cluster's output number; so
 * dp_tsdf_mesh's winding, and the outward normals, survive.
 * Output vertices.  A cluster SURVIVES iff a kept triangle names it; the others
 * count in orphan_clusters, and the output never has an unused vertex.
 * Survivors are numbered by ascending cluster number.  vertex_map[v] = the output
 * number of v's cluster, -1 if v is unused or its cluster an orphan;
 * triangle_map[t] = the output index, -1 for invalid, degenerate, collapsed and
 * duplicate triangles.
 * Output record of a surviving cluster with members v_1 < ... < v_n:
 *   mean, per axis c:    S = 0.0;  for j ascending: S = S + (double)pos_{v_j}[c];  m_c = dvdiv(S, (double)n)
 *   colour, per channel: R = the integer sum of the members' bytes; rgb = (2R + n) / (2n) in
 *                        integers (exact, so order-free); pad = 0
 *   DP_DECIMATE_MEAN:    pos_c = (float)m_c; the vertex counts in mean_vertices
 *   DP_DECIMATE_QUADRIC: walk the proper triangles that name at least one member
 *   (collapsed and duplicate ones included, each once per cluster) in ascending
 *   triangle index, with widened positions p0, p1, p2; the nine sums start at 0.0:
 *     e1 = p1 - p0;  e2 = p2 - p0;  g = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x)
 *     r = p0 - m;    d = (g.x*r.x + g.y*r.y) + g.z*r.z
 *     Axx += g.x*g.x; Axy += g.x*g.y; Axz += g.x*g.z; Ayy += g.y*g.y; Ayz += g.y*g.z; Azz += g.z*g.z
 *     bx += d*g.x;  by += d*g.y;  bz += d*g.z
 *   then
 *     c00 = Ayy*Azz - Ayz*Ayz;  c01 = Axz*Ayz - Axy*Azz;  c02 = Axy*Ayz - Axz*Ayy
 *     c11 = Axx*Azz - Axz*Axz;  c12 = Axy*Axz - Axx*Ayz;  c22 = Axx*Ayy - Axy*Axy
 *     det = (Axx*c00 + Axy*c01) + Axz*c02;  t = dvdiv((Axx + Ayy) + Azz, 3.0)
 *     solvable iff det is finite and det > DP_DECIMATE_DET_EPS * ((t*t)*t)
 *     x = (dvdiv((c00*bx + c01*by) + c02*bz, det), dvdiv((c01*bx + c11*by) + c12*bz, det),
 *          dvdiv((c02*bx + c12*by) + c22*bz, det));  cand_c = (float)(m_c + x_c)
 *   pos = cand iff the cluster is solvable, all three cand_c are finite and the
 *   cell of cand (the formula above, bounds included) is the cluster's cell; the
 *   vertex then counts in quadric_vertices.  Otherwise pos_c = (float)m_c and the
 *   vertex counts in mean_vertices: flat and crease clusters are unsolvable by
 *   construction and take the mean, which is intended.
 * quadric_vertices + mean_vertices = vertices_out.  Positions are expected to be
 * finite.  Statistics: the counts named above, vertices_in, triangles_in,
 * vertices_out, triangles_out; decimate_ms = device time of the call's kernels.
 *
 * Host and device forms follow dp_mesh_clean's: host arrays, vertex_map /
 * triangle_map the caller's (may be NULL), *vertices_out and *triangles_out
 * context-owned, valid until the next dp_mesh_decimate or destroy and NULL when
 * their count is 0; device arrays, one cap per output buffer, the first
 * min(cap, count) records written and nothing beyond them, the full counts
 * returned, everything queued on `stream` (NULL = the context's) and one wait,
 * for the counts (with stats NULL too).
 * Errors (DP_E_ARG), counts before pointers: the clean-up section's list (counts,
 * NULL inputs, caps, an output pointer equal to an input pointer, a NULL count
 * or, host form, result pointer); 3 * n_triangles > 2^31 - 1 (the (cluster,
 * triangle) pairs are counted in int32); opts NULL; cell not finite or not > 0; a
 * non-finite origin; mode outside {0, 1}; flags != 0.  n_triangles = 0 or
 * n_vertices = 0 is legal and yields empty results. */
#define DP_DECIMATE_MEAN 0
#define DP_DECIMATE_QUADRIC 1
#define DP_DECIMATE_DET_EPS 1e-6   /* design choice, nobody has tuned it */
typedef struct dp_mesh_decimate_options {
    float origin[3];   /* 0,0,0  anchor of the cluster lattice (finite)                       */
    float cell;        /* 0      cluster cell side, world units: must be set, > 0, finite     */
    int32_t mode;      /* DP_DECIMATE_MEAN                                                    */
    int32_t flags;     /* none defined; non-zero is DP_E_ARG                                  */
    int32_t reserved;
} dp_mesh_decimate_options;
typedef struct dp_mesh_decimate_stats {
    int64_t vertices_in, triangles_in, invalid_triangles, degenerate_triangles, unused_vertices,
        clamped_vertices, clusters, orphan_clusters, max_cluster, collapsed_triangles, duplicate_triangles,
        quadric_vertices, mean_vertices, vertices_out, triangles_out;
    double decimate_ms;
} dp_mesh_decimate_stats;

void dp_default_mesh_decimate_options(dp_mesh_decimate_options *mdo);
int dp_mesh_decimate(dp_ctx *ctx, const dp_mesh_decimate_options *opts, const dp_mesh_vertex *vertices,
                     int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                     const dp_mesh_vertex **vertices_out, int64_t *n_vertices_out, const int32_t **triangles_out,
                     int64_t *n_triangles_out, int32_t *vertex_map, int32_t *triangle_map,
                     dp_mesh_decimate_stats *stats);
int dp_mesh_decimate_device(dp_ctx *ctx, const dp_mesh_decimate_options *opts, const dp_mesh_vertex *d_vertices,
                            int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                            dp_mesh_vertex *d_vertices_out, int64_t vertex_cap, int64_t *n_vertices_out,
                            int32_t *d_triangles_out, int64_t triangle_cap, int64_t *n_triangles_out,
                            int32_t *d_vertex_map, int32_t *d_triangle_map, dp_mesh_decimate_stats *stats,
                            void *stream);

/* ---- per-view depth / triangle-index / normal maps of a triangle mesh -----------
 * No reference counterpart.  The way back from the mesh to the views: every
 * triangle is rasterised into the requested views of the CURRENT level
 * (dp_set_level: level-L P, W, H) and each pixel keeps the nearest one.  This is
 * dp_render_maps' disc rule restated for triangles -- an adjugate per (triangle,
 * view), a depth D / w, a per-pixel minimum of depth bits << 32 | index -- so the
 * result does not depend on the triangle order or the launch geometry.  All
 * arithmetic is fp64, one IEEE rounding per operation, in exactly the order
 * written (the build has -ffp-contract=off); row_r, dot and the rules of the
 * requested views (unique ids < V, 1 <= n_views <= V) are dp_render_maps'.
 *
 * Inputs: n_vertices 16-byte dp_mesh_vertex records, of which only pos is read,
 * and n_triangles triangles of three int32 indices; the output of any mesh stage
 * is a legal input.
 * Per view v, once on the host:
 *   m_v = (P0*(P5*P10 - P6*P9) - P1*(P4*P10 - P6*P8)) + P2*(P4*P9 - P5*P8),
 * the determinant of the left 3x3 of the level's P; an m_v that is not finite or
 * is 0 is DP_E_ARG.
 *
 * Triangle t = (i0, i1, i2) takes part iff its three indices lie in
 * [0, n_vertices) -- otherwise it counts in invalid_triangles, and its indices
 * are never used as an address -- and the nine floats of its positions are
 * finite.  X_k = pos of vertex i_k, widened to fp64.
 *
 * (t, v) is a pair iff, tested in this order,
 *   1. h_k = (row_0(P_v, X_k), row_1(P_v, X_k), row_2(P_v, X_k)) for k = 0, 1, 2:
 *      all three h_k[2] > 0.  A triangle that touches or crosses the camera plane
 *      is skipped whole (there is no clipping); such a pair counts in
 *      clipped_pairs when at least one h_k[2] > 0;
 *   2. edge rows, for k = 0, 1, 2 with a = h_{(k+1)%3}, b = h_{(k+2)%3}:
 *        r_k = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
 *        D = (h_0[0]*r_0[0] + h_0[1]*r_0[1]) + h_0[2]*r_0[2]
 *      skipped unless D is finite and D != 0.  The triangle is FRONT-facing in v
 *      iff D and m_v have opposite signs: cross(X1 - X0, X2 - X0) points towards
 *      the camera, dp_tsdf_mesh's outward winding.  With DP_MESH_RENDER_CULL_BACK
 *      a pair that is not FRONT is skipped and counts in culled_pairs;
 *   3. box: u_k = h_k[0] / h_k[2], v_k = h_k[1] / h_k[2]; skipped unless every
 *      |u_k| < 2e9 and every |v_k| < 2e9 (NaN skips); columns x0 = max(0,
 *      floor(min u_k)) .. x1 = min(W - 1, ceil(max u_k)), rows y0, y1 the same
 *      from v_k and H; skipped if x0 > x1 or y0 > y1.
 * The box is normative: no pixel outside it is ever covered by the pair.  It is
 * rounded outwards, so a rounding of u_k can never cut a pixel that the edge test
 * accepts.
 *
 * Integer pixel (x, y) of the box: l_k = (r_k[0]*x + r_k[1]*y) + r_k[2] for each
 * k.  It is covered iff (D > 0 and all three l_k >= 0) or (D < 0 and all three
 * l_k <= 0).  w = (l_0 + l_1) + l_2; skipped if w == 0; z = (float)(D / w),
 * accepted iff z is finite and z > 0.  (l / D is the inverse of [h_0 h_1 h_2]
 * applied to (x, y, 1), the pixel's barycentric weights; D / w is therefore
 * row_2(P_v, X) at the point X of the triangle's plane on the pixel's ray, the
 * depth dp_render_maps, dp_fuse_maps and dp_tsdf_integrate use.)  Per pixel the
 * minimum of key = (f32 bits of z) << 32 | t wins: the nearest depth, ties to
 * the lowest triangle index.
 *
 * Shared edges -- why the rows are cross products of the cyclic pair.  Two
 * triangles that share an edge with opposite direction (a consistently oriented
 * mesh) compute that edge's row as exact negations of each other: a*b - c*d and
 * c*d - a*b round to negated values.  Hence their l at any pixel are exact
 * negations, and if both face the same way the inclusive tests leave no pixel
 * between them uncovered; a pixel exactly on the edge goes to the nearer
 * triangle, or the lower index.  This is zero rounding and zero luck: do not
 * "optimise" the rows into a shared adjugate routine that reorders operands.
 *
 * Outputs, one pointer per requested view in the order of `views`, each
 * row-major W x H of that view at the current level; an array or an entry may be
 * NULL: depth f32 (0 where empty), index int32 (the triangle, -1), normal 3 x f32
 * (0): the winner's unit face normal, e = X1 - X0, f = X2 - X0, N = e x f
 * (N_0 = e1*f2 - e2*f1, N_1 = e2*f0 - e0*f2, N_2 = e0*f1 - e1*f0), s =
 * sqrt(dot(N, N)), (float)(N_c / s) when s is finite and s > 0, otherwise 0.  It
 * is oriented by the winding, not flipped towards the camera.
 * stats (may be NULL), counted on the device: triangles taking part,
 * invalid_triangles, pairs, clipped_pairs, culled_pairs, pixel_tests = the sum
 * of the pairs' box areas, covered_pixels = non-empty pixels after the resolve;
 * render_ms = device time of the call's kernels.
 * Options: only flags, the sole flag DP_MESH_RENDER_CULL_BACK; mro NULL = the
 * defaults.
 * Errors (DP_E_ARG): a count negative or above 2^31 - 1, a NULL input with a
 * non-zero count, n_views outside 1..V, a view id repeated or >= V, an m_v as
 * above, any other flag bit; no views set: DP_E_STATE.  n_triangles = 0 is
 * legal and yields empty planes.
 * The host form takes host arrays and host planes.  The device form takes device
 * vertices and triangles (the outputs of dp_tsdf_mesh_device,
 * dp_mesh_clean_device and dp_mesh_decimate_device are the intended inputs) and
 * device planes, queues everything on `stream` (NULL = the context's) and waits
 * only when stats != NULL, for the statistics read: dp_render_maps_device's
 * rule. */
#define DP_MESH_RENDER_CULL_BACK 1
typedef struct dp_mesh_render_options {
    int32_t flags;          /* DP_MESH_RENDER_* bits (default 0) */
} dp_mesh_render_options;
typedef struct dp_mesh_render_stats {
    int64_t triangles, invalid_triangles, pairs, clipped_pairs, culled_pairs, pixel_tests, covered_pixels;
    double render_ms;
} dp_mesh_render_stats;

void dp_default_mesh_render_options(dp_mesh_render_options *mro);
int dp_mesh_render(dp_ctx *ctx, const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                   int64_t n_triangles, const int32_t *views, int n_views, const dp_mesh_render_options *mro,
                   float *const *depth, int32_t *const *index, float *const *normal, dp_mesh_render_stats *stats);
int dp_mesh_render_device(dp_ctx *ctx, const dp_mesh_vertex *d_vertices, int64_t n_vertices,
                          const int32_t *d_triangles, int64_t n_triangles, const int32_t *views, int n_views,
                          const dp_mesh_render_options *mro, float *const *d_depth, int32_t *const *d_index,
                          float *const *d_normal, dp_mesh_render_stats *stats, void *stream);

/* ---- vertex colours of a mesh from the views that see it -----------------------
 * No reference counterpart.  dp_tsdf_mesh's vertex colours are the voxels': a
 * per-voxel mean blurred to the voxel size, which dp_mesh_smooth and
 * dp_mesh_decimate then carry to places the surface no longer is.  This stage
 * colours the FINAL vertices: a vertex is projected into every requested view of
 * the CURRENT level (dp_set_level: level-L P, W, H and BGRA8 planes), a depth
 * plane of the mesh in that view (dp_mesh_render's depth output is the intended
 * input) decides whether the view sees it, and the colour is the mean of the
 * seeing views' texels, weighted by the cosine between the vertex normal and the
 * ray when normals are given.  All arithmetic is fp64, one IEEE rounding per
 * operation, in exactly the order written (the build has -ffp-contract=off);
 * row_r, dot, "is a depth", backproject, A, det and the rules of the requested
 * views (unique ids < V, 1 <= K <= min(V, 64)) are dp_fuse_maps's.
 *
 * Inputs: n_vertices 16-byte dp_mesh_vertex records; optionally `normals`, 3 x
 * f32 per vertex (dp_mesh_normals' output is the intended input; NULL = none);
 * the requested views views[0..K-1]; per requested view, in the order of
 * `views`, an f32 depth plane W x H, row-major, of the mesh at the current level
 * (the array and every entry are required); the options below.  No triangle is
 * read.
 *
 * Per requested view v, once on the host: A and det as in dp_fuse_maps (a det
 * that is 0 or not finite: DP_E_ARG) and the camera centre C_v = backproject(v,
 * 0, 0, 0), that is
 *   C_j = ((A[3j]*(0 - P[3]) + A[3j+1]*(0 - P[7])) + A[3j+2]*(0 - P[11])) / det;
 * a C that is not finite: DP_E_ARG.
 *
 * Vertex i takes part iff its three pos floats are finite; otherwise its record
 * is copied byte for byte, its seen is 0 and its best is -1, and it counts in no
 * statistic.  X = pos widened to fp64.  With normals, n = its normal widened,
 * l2 = dot(n, n), and the vertex HAS A NORMAL iff l2 is finite and l2 > 0.
 * Start with wsum = 0.0, s_R = s_G = s_B = 0.0, mask = 0, best = -1, bw = 0.0;
 * then for k = 0..K-1 in order, v = views[k]:
 *   1. d, u, v, xi, yi by steps 1-3 of dp_fuse_maps's observe (d > 0; |u|, |v| <
 *      2e9; rint, round-half-even; 0 <= xi < W_v and 0 <= yi < H_v);
 *   2. z = depth_v[yi][xi]; require that z is a depth.  A pair that gets this far
 *      counts in projected_pairs;
 *   3. occlusion, one-sided: require d - (double)z <= (double)depth_tol * d (a
 *      surface in front of the vertex hides it; one behind it does not).  A pair
 *      that fails counts in occluded_pairs;
 *   4. weight.  Without a normal wgt = 1.0.  With one: ray_j = X_j - C_j; q =
 *      dot(ray, ray) * l2, require q finite and q > 0; c = (0.0 - dot(n, ray)) /
 *      sqrt(q), require c > 0 and c >= (double)min_cos; wgt = c.  A pair that
 *      fails a requirement of this step counts in grazing_pairs;
 *   5. sample each channel ch of view v's BGRA8 plane (R = bits 16..23, G = bits
 *      8..15, B = bits 0..7 of the texel word, the bytes dp_tsdf_integrate reads;
 *      t(x, y) = that byte of texel (x, y)).  Default: val = (double)t(xi, yi).
 *      With DP_MESH_COLOUR_BILINEAR: x0 = floor(u), y0 = floor(v), fx = u -
 *      (double)x0, fy = v - (double)y0; taps xa = clamp(x0, 0, W-1), xb =
 *      clamp(x0 + 1, 0, W-1), ya, yb likewise with H;
 *        top = (1.0 - fx)*t(xa, ya) + fx*t(xb, ya)
 *        bot = (1.0 - fx)*t(xa, yb) + fx*t(xb, yb)
 *        val = (1.0 - fy)*top + fy*bot;
 *   6. s_ch = s_ch + wgt * val; wsum = wsum + wgt; mask |= 1 << k (64-bit); if
 *      wgt > bw: bw = wgt, best = k (ties go to the lowest k); the pair counts
 *      in visible_pairs.
 * projected_pairs = occluded_pairs + grazing_pairs + visible_pairs.
 *
 * Outputs: vertices_out, pos and pad copied; for mask != 0 rgb[ch] =
 * (uint8)min(255.0, rint(s_ch / wsum)), ch = R, G, B, and the vertex counts in
 * coloured_vertices; for mask == 0 the input colour -- or 0, 0, 0 with
 * DP_MESH_COLOUR_CLEAR_UNSEEN -- and it counts in unseen_vertices.  Optional
 * seen: uint64 per vertex, bit k = position k in `views`.  Optional best: int32
 * per vertex, the position k of the heaviest view, -1 when unseen.  One vertex's
 * result is a function of that vertex and the views walked in order: no atomics
 * on the results, no dependence on the launch geometry.
 * stats (may be NULL), counted on the device: vertices (those taking part),
 * projected_pairs, occluded_pairs, grazing_pairs, visible_pairs,
 * coloured_vertices, unseen_vertices; colour_ms = device time of the call's
 * kernel.
 * Options: mco NULL = the defaults.
 * Errors (DP_E_ARG): n_vertices negative or above 2^31 - 1, vertices NULL with
 * n_vertices > 0, the view rules, depth NULL or a NULL entry, depth_tol negative
 * or not finite, min_cos outside 0..1, an unknown flag, an output that equals an
 * input, a det or C as above; no views set: DP_E_STATE.  n_vertices = 0 is legal.
 * Host form: host arrays and planes; *vertices_out (required) is context-owned,
 * valid until the next dp_mesh_colour or destroy, NULL when n_vertices is 0; seen
 * and best are the caller's arrays.  Device form: device vertices, normals,
 * planes and caller buffers (d_vertices_out required when n_vertices > 0);
 * everything is queued on `stream` (NULL = the context's) and the call waits
 * only when stats != NULL.
 * Limits: the occlusion test reads the nearest pixel's depth, so on a steep
 * slant it leans on depth_tol; all K depth planes are resident at once; the
 * colour is per vertex (seen and best are what a texture atlas would start
 * from). */
#define DP_MESH_COLOUR_BILINEAR 1
#define DP_MESH_COLOUR_CLEAR_UNSEEN 2
typedef struct dp_mesh_colour_options {
    float depth_tol;        /* 0.01 relative depth by which a vertex may lie behind the plane */
    float min_cos;          /* 0.2  least cosine between the normal and the ray to the camera  */
    int32_t flags;          /* DP_MESH_COLOUR_* bits (default 0)                               */
} dp_mesh_colour_options;
typedef struct dp_mesh_colour_stats {
    int64_t vertices, projected_pairs, occluded_pairs, grazing_pairs, visible_pairs, coloured_vertices,
        unseen_vertices;
    double colour_ms;
} dp_mesh_colour_stats;

void dp_default_mesh_colour_options(dp_mesh_colour_options *mco);
int dp_mesh_colour(dp_ctx *ctx, const dp_mesh_vertex *vertices, int64_t n_vertices, const float *normals,
                   const int32_t *views, int n_views, const dp_mesh_colour_options *mco, const float *const *depth,
                   const dp_mesh_vertex **vertices_out, uint64_t *seen, int32_t *best, dp_mesh_colour_stats *stats);
int dp_mesh_colour_device(dp_ctx *ctx, const dp_mesh_vertex *d_vertices, int64_t n_vertices, const float *d_normals,
                          const int32_t *views, int n_views, const dp_mesh_colour_options *mco,
                          const float *const *d_depth, dp_mesh_vertex *d_vertices_out, uint64_t *d_seen,
                          int32_t *d_best, dp_mesh_colour_stats *stats, void *stream);

/* ---- nearest-point distances between two point clouds ----------------------------
 * No reference counterpart.  For every point of cloud A (the queries) the nearest
 * point of cloud B (the targets) within a radius: the primitive under accuracy,
 * completeness and F-score of a reconstruction against a ground truth (see
 * cloud_compare in the Python package and densify --evaluate).  All arithmetic
 * is fp64, one IEEE rounding per operation, in exactly the order written (the
 * build has -ffp-contract=off).
 *
 * Inputs: n_queries and n_targets points.  Point i of an array is three
 * consecutive f32 at base + i * stride; the stride is in bytes, a multiple of 4
 * and at least 12, so dp_patch (64, pointing at pos), dp_fused_point (40),
 * dp_mesh_vertex (16) and packed xyz (12) records are passed as they are.
 * Nothing but the twelve bytes of each point is read (the host form copies an
 * array from its first point to the end of its last, the bytes between the
 * points with it, and nothing behind that).  No view is read: the call
 * works on a context on which dp_set_views was never called.
 *
 * A point TAKES PART iff its three floats are finite.  A query that does not gets
 * index -1 and dist +inf and counts in skipped_queries; a target that does not is
 * never a candidate and counts in skipped_targets.  For a query q and a target t
 * that both take part:
 *   dx = (double)q.x - (double)t.x, dy and dz likewise;
 *   d2 = (dx*dx + dy*dy) + dz*dz;
 *   R2 = (double)max_dist * (double)max_dist;
 *   t is a CANDIDATE iff d2 <= R2 (the bound is inclusive).
 * The answer of q is the candidate with the smallest d2; equal d2 goes to the
 * lowest target index.  index[q] = that target's index in the caller's array,
 * dist[q] = (float)sqrt(d2), and q counts in matched.  A query with no candidate
 * gets index -1 and dist +inf and counts in unmatched.
 * With hist_bins = B > 0 every matched query adds 1 to bin
 *   min(B - 1, (int64)floor((double)dist / (double)max_dist * (double)B)),
 * dist being the f32 output; the counts are uint64 and the bins sum to matched
 * (integer atomics; there is no floating-point atomic anywhere).
 * queries + skipped_queries = n_queries, targets + skipped_targets = n_targets,
 * matched + unmatched = queries.  n_queries = 0 and n_targets = 0 are legal;
 * with no targets every query is unmatched.
 *
 * The result is a function of the two point sets and max_dist alone: not of the
 * search grid, the launch geometry or the order of the queries; a permutation of
 * the targets permutes `index` and nothing else, except where d2 ties.
 * grid_cells and max_cell_targets describe the search grid of the implementation
 * (its cells, at most 2^24, and the most targets in one of them), not the spec.
 * build_ms = device time of the grid's construction, query_ms = of the queries'
 * sort and walk.
 * Errors (DP_E_ARG): a count negative or above 2^31 - 1, a NULL array with a
 * positive count, a stride that is no multiple of 4 or below 12, opts NULL,
 * max_dist not finite or not positive, hist_bins outside 0..65536, a non-zero
 * flag, an output that equals an input; device form: d_index or d_dist NULL with
 * n_queries > 0.
 * Host form: host arrays; *index, *dist (both required) and *hist are
 * context-owned, valid until the next dp_cloud_nearest or destroy (*index and
 * *dist NULL when n_queries is 0); *hist is written only when hist is non-NULL
 * and hist_bins > 0.  Device form: device arrays and caller buffers (d_hist
 * optional: with hist_bins > 0 and d_hist NULL no histogram is written);
 * everything is queued on `stream` (NULL = the context's) and the call waits
 * only when stats != NULL.
 * Limits: one nearest neighbour, point to point (not point to triangle); scratch
 * is 28 bytes per target, 16 per query and the cell table (4 bytes per cell). */
typedef struct dp_cloud_nearest_options {
    float max_dist;     /* search radius, world units (> 0, finite; no default) */
    int32_t hist_bins;  /* 0 = no histogram; else 1..65536                     */
    int32_t flags;      /* none defined; non-zero is DP_E_ARG                  */
} dp_cloud_nearest_options;
typedef struct dp_cloud_nearest_stats {
    int64_t queries, targets;          /* those taking part                      */
    int64_t skipped_queries, skipped_targets, matched, unmatched;
    int64_t grid_cells, max_cell_targets;  /* facts of the implementation, not of the spec */
    double build_ms, query_ms;
} dp_cloud_nearest_stats;

int dp_cloud_nearest(dp_ctx *ctx, const void *queries, int64_t n_queries, int64_t query_stride,
                     const void *targets, int64_t n_targets, int64_t target_stride,
                     const dp_cloud_nearest_options *opts, const int32_t **index, const float **dist,
                     const uint64_t **hist, dp_cloud_nearest_stats *stats);
int dp_cloud_nearest_device(dp_ctx *ctx, const void *d_queries, int64_t n_queries, int64_t query_stride,
                            const void *d_targets, int64_t n_targets, int64_t target_stride,
                            const dp_cloud_nearest_options *opts, int32_t *d_index, float *d_dist,
                            uint64_t *d_hist, dp_cloud_nearest_stats *stats, void *stream);

/* ---- the k nearest neighbours between two point clouds ---------------------------
 * No reference counterpart.  dp_cloud_nearest for k neighbours: the primitive
 * under outlier removal (dp_cloud_clean below), normal estimation, smoothing and
 * density weights of a cloud.  Everything dp_cloud_nearest says holds here unless
 * stated: points read in place at any stride >= 12 that is a multiple of 4; a
 * point TAKES PART iff its three floats are finite; d2 = (dx*dx + dy*dy) + dz*dz in
 * fp64; a target is a CANDIDATE iff d2 <= R2, R2 = (double)max_dist *
 * (double)max_dist, inclusive; counts up to 2^31 - 1; no views.
 *
 * Options.  max_dist finite and > 0; k in 1..32; flags = 0 or
 * DP_CLOUD_KNN_EXCLUDE_SELF.  With EXCLUDE_SELF target i is never a candidate of
 * query i: the rule is on the index, not on the pointer or the position, so it
 * means the same in the host form, and it requires n_queries == n_targets.  A
 * duplicate of the point under another index stays a candidate at distance 0.
 *
 * Answer.  The answer of query q is its candidates ordered by (d2 ascending,
 * target index ascending), cut to the first k.  index[q * k + j] = the index of
 * the j-th of them in the caller's target array, dist[q * k + j] = (float)
 * dvsqrt(d2) of it; the rest of the row is -1 and +inf.  count[q] (int32, 0..k)
 * is the number of real entries.  A query that does not take part gets count 0
 * and a padded row and counts in skipped_queries.
 * Statistics.  queries, targets, skipped_queries, skipped_targets as in
 * dp_cloud_nearest; full = queries with count == k, partial = with 0 < count <
 * k, empty = with count == 0 (full + partial + empty = queries); neighbours =
 * the sum of all counts.  grid_cells, max_cell_targets, build_ms and query_ms
 * are facts of the implementation, as in dp_cloud_nearest.
 *
 * The result is a function of the two point sets, max_dist, k and the flag
 * alone: not of the grid, the launch geometry or the order of the queries (the
 * order (d2, index) is total, so the list is the same in whatever order the
 * candidates are met).  With k = 1 and no flag, index and dist equal
 * dp_cloud_nearest's bit for bit.
 * Errors (DP_E_ARG): dp_cloud_nearest's on the counts, pointers, strides, opts and
 * max_dist; k outside 1..32; an unknown flag; EXCLUDE_SELF with n_queries !=
 * n_targets; an output that equals an input; host form: index, dist or count
 * NULL; device form: d_index, d_dist or d_count NULL with n_queries > 0.
 * Host form: *index, *dist and *count are context-owned, valid until the next
 * dp_cloud_knn, dp_cloud_clean, dp_cloud_normals or destroy (NULL when n_queries
 * is 0).  Device
 * form: caller buffers of n_queries * k int32, n_queries * k f32 and n_queries
 * int32; everything is queued on `stream` (NULL = the context's) and the call
 * waits only when stats != NULL.
 * Limits: k <= 32, nothing beyond max_dist; one lane per query, its list in
 * registers (lists of 8, 16 or 32 entries, the smallest that holds k).  Scratch
 * is dp_cloud_nearest's and shared with it. */
#define DP_CLOUD_KNN_EXCLUDE_SELF 1
typedef struct dp_cloud_knn_options {
    float max_dist;     /* search radius, world units (> 0, finite; no default) */
    int32_t k;          /* neighbours per query, 1..32                         */
    int32_t flags;      /* DP_CLOUD_KNN_*; another bit is DP_E_ARG             */
} dp_cloud_knn_options;
typedef struct dp_cloud_knn_stats {
    int64_t queries, targets;          /* those taking part                      */
    int64_t skipped_queries, skipped_targets, full, partial, empty, neighbours;
    int64_t grid_cells, max_cell_targets;  /* facts of the implementation, not of the spec */
    double build_ms, query_ms;
} dp_cloud_knn_stats;

int dp_cloud_knn(dp_ctx *ctx, const void *queries, int64_t n_queries, int64_t query_stride,
                 const void *targets, int64_t n_targets, int64_t target_stride,
                 const dp_cloud_knn_options *opts, const int32_t **index, const float **dist,
                 const int32_t **count, dp_cloud_knn_stats *stats);
int dp_cloud_knn_device(dp_ctx *ctx, const void *d_queries, int64_t n_queries, int64_t query_stride,
                        const void *d_targets, int64_t n_targets, int64_t target_stride,
                        const dp_cloud_knn_options *opts, int32_t *d_index, float *d_dist,
                        int32_t *d_count, dp_cloud_knn_stats *stats, void *stream);

/* ---- statistical and radius outlier removal of a point cloud ----------------------
 * No reference counterpart (the reference links PCL's filters for this).  One
 * cloud: n records of `stride` bytes (a multiple of 4, at least 12), the point in
 * the first 12 bytes of each.  A record is kept when it has enough neighbours
 * within max_dist and its mean distance to them is not far above the cloud's.
 *
 * Options.  max_dist finite and > 0; k in 1..32; min_neighbours in 1..k;
 * std_mul finite and >= 0; flags = 0 or DP_CLOUD_CLEAN_RADIUS_ONLY.
 *
 * Per point.  dp_cloud_knn of the cloud against itself with EXCLUDE_SELF, max_dist
 * and k.  c_i = the point's count.  m_i = its mean neighbour distance: the fp64
 * sum, in rank order and starting from the first term, of dvsqrt(d2) over the
 * c_i neighbours, then dvdiv(sum, (double)c_i).  A point is ELIGIBLE iff it takes
 * part and c_i >= min_neighbours.
 *
 * Global statistics (skipped with RADIUS_ONLY, which reports mu = sigma =
 * threshold = 0).  N = the number of eligible points.
 *   mu    = dvdiv(S(x), (double)N),  x_i = m_i for eligible points, +0.0 otherwise;
 *   var   = dvdiv(S(y), (double)(N - 1)),  y_i = (m_i - mu) * (m_i - mu) for eligible
 *           points, +0.0 otherwise; var = 0 when N < 2;
 *   sigma = dvsqrt(var);   T = mu + (double)std_mul * sigma;
 *   with N = 0, mu = sigma = T = 0.
 * S is the balanced pairwise sum: the n-vector padded with +0.0 to the next
 * power of two, then replaced by x[2j] + x[2j+1] until one value is left (numpy:
 * while len(x) > 1: x = x[0::2] + x[1::2]).  The order is fixed, there is no
 * floating-point atomic, and the tree is the one xor-shuffles compute.
 *
 * Decision.  keep[i] = eligible_i && (RADIUS_ONLY || m_i <= T).
 * Outputs.  keep: uint8 per point, 0 or 1.  mean_dist (optional): (float)m_i,
 * +inf where c_i = 0 or the point does not take part.  map (optional): int32 per
 * point, its index among the kept points in input order, -1 for a removed one.
 * out (optional): the kept records, `stride` bytes each, copied whole and packed
 * in input order.  The kept count: *n_out (host form), *d_n_out (device form, an
 * optional device int64).
 * Statistics.  points = those taking part, skipped = the others (points + skipped
 * = n); eligible; kept; removed_sparse = takes part and c_i < min_neighbours;
 * removed_far = eligible and m_i > T; kept + removed_sparse + removed_far =
 * points.  mu, sigma, threshold as above.  grid_cells and max_cell_targets are
 * the search's; knn_ms = device time of the search, clean_ms = of the rest.
 * n = 0 is legal.
 * Errors (DP_E_ARG): n negative or above 2^31 - 1; points NULL with n > 0; a
 * stride that is no multiple of 4 or below 12; opts NULL; an option outside the
 * ranges above; an output that equals the input or another output; host form:
 * keep NULL; device form: d_keep NULL with n > 0.
 * Host form: *keep, *mean_dist, *map and *out are context-owned, valid until the
 * next dp_cloud_knn, dp_cloud_clean, dp_cloud_normals or destroy; pass NULL for those of
 * mean_dist, map, out and n_out that are not wanted.  Device form: caller buffers
 * (d_out of n * stride bytes); everything is queued on `stream` (NULL = the
 * context's), mu, sigma and T never leave the device before the end, and the
 * call waits only when stats != NULL.
 * Limits: dp_cloud_knn's.  Scratch is the search's plus 4 * k + 20 bytes per
 * point. */
#define DP_CLOUD_CLEAN_RADIUS_ONLY 1
typedef struct dp_cloud_clean_options {
    float max_dist;          /* neighbourhood radius (> 0, finite; no default)   */
    int32_t k;               /* neighbours per point, 1..32                      */
    int32_t min_neighbours;  /* 1..k                                             */
    float std_mul;           /* T = mu + std_mul * sigma (>= 0, finite)          */
    int32_t flags;           /* DP_CLOUD_CLEAN_*; another bit is DP_E_ARG        */
} dp_cloud_clean_options;
typedef struct dp_cloud_clean_stats {
    int64_t points, skipped, eligible, kept, removed_sparse, removed_far;
    int64_t grid_cells, max_cell_targets;  /* facts of the implementation, not of the spec */
    double mu, sigma, threshold;
    double knn_ms, clean_ms;
} dp_cloud_clean_stats;

int dp_cloud_clean(dp_ctx *ctx, const void *points, int64_t n, int64_t stride,
                   const dp_cloud_clean_options *opts, const uint8_t **keep, const float **mean_dist,
                   const int32_t **map, const void **out, int64_t *n_out, dp_cloud_clean_stats *stats);
int dp_cloud_clean_device(dp_ctx *ctx, const void *d_points, int64_t n, int64_t stride,
                          const dp_cloud_clean_options *opts, uint8_t *d_keep, float *d_mean_dist,
                          int32_t *d_map, void *d_out, int64_t *d_n_out, dp_cloud_clean_stats *stats,
                          void *stream);

/* ---- PCA normals and surface variation of a point cloud ----------------------------
 * No reference counterpart.  One cloud: n records of `stride` bytes (a multiple of
 * 4, at least 12; counts up to 2^31 - 1), the position in the first 12 bytes of
 * each, as in dp_cloud_clean.  Every point gets the direction of least spread of
 * its neighbourhood (the eigenvector of the smallest eigenvalue of the
 * neighbourhood's scatter matrix) as a unit normal, and that eigenvalue's share of
 * the trace as its surface variation (Pauly et al. 2002): 0 on a plane, 1/3 where
 * the neighbourhood spreads alike in all directions.  A point TAKES PART iff its
 * three floats are finite.  All arithmetic is fp64, one IEEE rounding per operation,
 * in exactly the order written; dvdiv and dvsqrt are the IEEE-correct quotient and
 * square root.  There is no floating-point atomic.  No view is read.
 *
 * Options.  max_dist finite and > 0; k in 3..32; min_neighbours in 3..k; flags = 0,
 * DP_CLOUD_NORMALS_ORIENT_VIEWPOINT or DP_CLOUD_NORMALS_ORIENT_DIRECTION (both
 * together, or another bit, is DP_E_ARG).  toward and toward_stride are arguments of
 * the call: required with either flag, NULL and 0 without one.  toward_stride = 0
 * means one entry for every point; otherwise it is a multiple of 4 and at least 12
 * and entry i is the three f32 at toward + i * toward_stride.  toward may point into
 * the records themselves (a dp_fused_point's own normal: toward = points + 12,
 * toward_stride = stride); nothing is written there.
 *
 * Neighbourhood.  The row of point i in dp_cloud_knn of the cloud against itself
 * with k, max_dist and NO flag: the point itself is in its own row (at d2 = 0,
 * ranked among its duplicates by index), so that a point with two neighbours has
 * the three points a plane needs, and so that the estimate at i is the fit of a
 * set that contains i.  The row has c_i entries p_0 .. p_{c-1} in rank order.
 * Mean.  m_a = dvdiv(sum of (double)p_j.a over j in rank order, starting from the
 * first term, (double)c_i) for each axis a.
 * Scatter.  d_ja = (double)p_j.a - m_a.  Six sums C_ab, ab = xx, xy, xz, yy, yz, zz,
 * each of d_ja * d_jb over j in rank order, starting from the first product.  They
 * are not divided by c_i: only ratios and directions are used, and a division
 * would add a rounding to every entry for nothing.  T = (C_xx + C_yy) + C_zz.
 * Classes.  A point that takes part is exactly one of
 *   SPARSE      c_i < min_neighbours;
 *   DEGENERATE  not sparse and T == 0.0 (every neighbour coincides);
 *   ESTIMATED   everything else.
 * Eigenvector (ESTIMATED points).  N = the symmetric 3 x 3 matrix C, V = the
 * identity.  DP_CLOUD_NORMALS_SWEEPS times, for (p, q) = (0,1), (0,2), (1,2) in this
 * order, dp_cloud_align's rotation: skipped when N_pq == 0.0, otherwise the same
 * theta, t, c, s and h expressions, the row update for the one k other than p and
 * q, the V update for k = 0..2.  j = the index of the smallest N_jj, the lowest on
 * ties; v = column j of V;
 *   len = dvsqrt((v0 * v0 + v1 * v1) + v2 * v2);  u_a = dvdiv(v_a, len);
 *   variation = (float)dvdiv(fmax(N_jj, 0.0), T)
 * with the T from before the rotations (the rotations keep the trace only up to
 * rounding, and T is the value the DEGENERATE test used); fmax(N_jj, 0.0) is +0.0
 * unless N_jj > 0, for a -0.0 too.
 *   DP_CLOUD_NORMALS_SWEEPS is 10, dp_cloud_align's count.  On the test inputs of
 *   tests/test_cloud_normals_cpu.py (random, sparse, planar, collinear, duplicated,
 *   lattice and far-offset clouds) the reference's off-diagonal mass sqrt(sum of
 *   N_pq^2, p < q) is below 2^-50 of T after at most 3 sweeps and exactly zero
 *   after at most 5; a sweep over a diagonal matrix skips every rotation, so the
 *   extra sweeps change no bit.
 * Sign.  a = the index of the largest fabs(u_a), the lowest on ties; if u_a < 0
 * every component is negated (a zero component becomes -0.0).  An eigenvector has
 * no sign of its own and Jacobi's depends on the rotations it happened to make;
 * this one depends on the direction alone.  With ORIENT_VIEWPOINT, w = entry i of
 * toward and x = the point's own position:
 *   s = (((double)w.x - (double)x.x) * u_x + ((double)w.y - (double)x.y) * u_y)
 *       + ((double)w.z - (double)x.z) * u_z;
 * with ORIENT_DIRECTION:
 *   s = ((double)w.x * u_x + (double)w.y * u_y) + (double)w.z * u_z.
 * If s < 0, u is negated and the point counts in flipped; if s == 0, or w is not
 * finite in all three floats, u keeps the sign above and the point counts in
 * unoriented.
 *
 * Outputs.  normal: 3 f32 per point, packed: (float)u_a of an ESTIMATED point,
 * (0, 0, 0) of any other.  variation (optional): f32 per point, in [0, 1/3] when
 * estimated, +inf otherwise.  count (optional): int32 per point, c_i, 0 for a
 * point that does not take part.
 * Statistics.  points = those taking part, skipped = the others (points + skipped
 * = n); estimated + sparse + degenerate = points; flipped and unoriented as above
 * (both 0 without a flag).  grid_cells and max_cell_targets are the search's;
 * knn_ms = device time of the search, normals_ms = of everything after it.
 * n = 0 is legal.
 * Errors (DP_E_ARG): dp_cloud_clean's on n, points, stride and opts; an option
 * outside the ranges above; the toward rules above; an output that equals an input
 * or another output; host form: normal NULL; device form: d_normal NULL with n > 0.
 * Host form: *normal, *variation and *count are context-owned, valid until the
 * next dp_cloud_normals, dp_cloud_knn, dp_cloud_clean or destroy (NULL when n is
 * 0); pass NULL for those of variation and count that are not wanted.  The records
 * are copied from the first point to the end of the last; toward entries that
 * start inside that range are read from the copy, which then reaches to the end
 * of the last entry.  Device form: caller buffers; everything is queued on
 * `stream` (NULL = the context's) and the call waits only when stats != NULL.
 * Limits: dp_cloud_knn's; unweighted PCA, no consistent orientation across the
 * cloud without `toward`.  One lane per point.  Scratch is the search's plus 4 * k
 * + 4 bytes per point. */
#define DP_CLOUD_NORMALS_ORIENT_VIEWPOINT 1
#define DP_CLOUD_NORMALS_ORIENT_DIRECTION 2
#define DP_CLOUD_NORMALS_SWEEPS 10
typedef struct dp_cloud_normals_options {
    float max_dist;          /* neighbourhood radius (> 0, finite; no default)   */
    int32_t k;               /* neighbours per point, itself included, 3..32     */
    int32_t min_neighbours;  /* 3..k                                             */
    int32_t flags;           /* 0 or one DP_CLOUD_NORMALS_ORIENT_*                */
} dp_cloud_normals_options;
typedef struct dp_cloud_normals_stats {
    int64_t points, skipped, estimated, sparse, degenerate, flipped, unoriented;
    int64_t grid_cells, max_cell_targets;  /* facts of the implementation, not of the spec */
    double knn_ms, normals_ms;
} dp_cloud_normals_stats;

int dp_cloud_normals(dp_ctx *ctx, const void *points, int64_t n, int64_t stride,
                     const dp_cloud_normals_options *opts, const void *toward, int64_t toward_stride,
                     const float **normal, const float **variation, const int32_t **count,
                     dp_cloud_normals_stats *stats);
int dp_cloud_normals_device(dp_ctx *ctx, const void *d_points, int64_t n, int64_t stride,
                            const dp_cloud_normals_options *opts, const void *d_toward, int64_t toward_stride,
                            float *d_normal, float *d_variation, int32_t *d_count,
                            dp_cloud_normals_stats *stats, void *stream);

/* ---- a 3 x 4 transform applied to the records of a cloud ----------------------------
 * No reference counterpart.  n records of `stride` bytes (a multiple of 4, at least
 * 12; counts up to 2^31 - 1), the position in the first 12 bytes of each, as in
 * dp_cloud_clean.  matrix is a host array of 12 doubles, row-major M = [A | t]:
 * row r is (a0, a1, a2, t) = matrix[4r .. 4r + 3].  All arithmetic is fp64, one
 * IEEE rounding per operation, in the order written.
 *
 * Every record is copied whole into out (the device form's d_out may equal
 * d_points: the transform in place).  Then, for a record whose position (x, y, z)
 * is finite in all three floats, coordinate r of the position becomes
 *   (float)(((a0 * (double)x + a1 * (double)y) + a2 * (double)z) + t);
 * a record whose position is not finite is left as copied.  With normal_offset >=
 * 0 the three floats n at that byte offset of the record are the normal: with
 *   v_r = (a0 * (double)n.x + a1 * (double)n.y) + a2 * (double)n.z,
 *   len = dvsqrt((v_0 * v_0 + v_1 * v_1) + v_2 * v_2),
 * they become (float)dvdiv(v_r, len) when len is finite and > 0, and are left as
 * copied otherwise (A * n zero or not finite).  The normal of a record is treated
 * whatever its position is.  One lane per record.
 * Errors (DP_E_ARG): n negative or above 2^31 - 1; points NULL with n > 0; a stride
 * that is no multiple of 4 or below 12; matrix NULL or with an entry that is not
 * finite; normal_offset neither -1 nor a multiple of 4 in 12 .. stride - 12; out
 * NULL (host form), d_out NULL with n > 0 (device form).
 * Host form: *out is context-owned, n * stride bytes, valid until the next
 * dp_cloud_transform, dp_cloud_align or destroy (NULL when n is 0).  Device form:
 * queued on `stream` (NULL = the context's); the call does not wait. */
int dp_cloud_transform(dp_ctx *ctx, const void *points, int64_t n, int64_t stride, const double *matrix,
                       int64_t normal_offset, const void **out);
int dp_cloud_transform_device(dp_ctx *ctx, const void *d_points, int64_t n, int64_t stride, const double *matrix,
                              int64_t normal_offset, void *d_out, void *stream);

/* ---- registration of one cloud to another: point-to-point ICP -----------------------
 * No reference counterpart.  The rigid motion (or, with DP_CLOUD_ALIGN_SCALE, the
 * similarity with s > 0) that moves the `source` cloud onto the `target` cloud,
 * by iterated closest points trimmed at the radius max_dist: what puts a
 * reconstruction into the frame of its ground truth before dp_cloud_nearest
 * measures it.  The clouds are dp_cloud_nearest's: three f32 at base + i * stride,
 * any stride that is a multiple of 4 and at least 12, counts up to 2^31 - 1, a
 * point TAKES PART iff its three floats are finite.  All arithmetic is fp64, one
 * IEEE rounding per operation, in exactly the order written; dvdiv and dvsqrt are
 * the IEEE-correct quotient and square root.  There is no floating-point atomic.
 *
 * Options.  max_dist finite and > 0; iterations in 1..1000; min_pairs >= 3;
 * rms_tol finite and >= 0 (0 = never stop early); flags = 0 or
 * DP_CLOUD_ALIGN_SCALE.  init: 12 finite doubles, the first M (row-major [A | t]
 * as in dp_cloud_transform), or NULL for the identity.
 *
 * A PASS with the current M (steps 1 to 4):
 * 1. y_i = dp_cloud_transform's position expression of source point x_i under M,
 *    into a packed scratch array (a point that is not finite is copied as it is).
 *    The source is never modified, and every pass starts from the original x_i:
 *    transforms are never composed and rounded points never chained.
 * 2. c(i), dist_i = dp_cloud_nearest(y, target, max_dist), bit for bit: the same
 *    d2, the inclusive radius, ties to the lowest index, c(i) = -1 for a y_i that
 *    does not take part or has no candidate.  i is MATCHED iff c(i) >= 0; q_i is
 *    target point c(i).  The target grid is built once per call.
 * 3. m = the number of matched i (an integer).  Six sums over i in source order,
 *    of x_i.x, x_i.y, x_i.z, q_i.x, q_i.y, q_i.z: the term of a matched i is
 *    (double)v + 0.0 (the + 0.0 turns a -0.0 into +0.0), of an unmatched i +0.0.
 *    Each sum is S of dp_cloud_clean: the balanced pairwise tree over the n_source
 *    terms padded with +0.0 to the next power of two.  mux_a = dvdiv(sum, (double)m)
 *    and muq_a likewise; all six are 0 when m = 0.
 * 4. With dx_a = (double)x_i.a - mux_a and dq_b = (double)q_i.b - muq_b, eleven
 *    sums S of the same kind (each term t entering as t + 0.0, +0.0 when unmatched):
 *      S_ab = sum of dx_a * dq_b   (a, b in x, y, z; nine sums),
 *      Sx   = sum of (dx_x * dx_x + dx_y * dx_y) + dx_z * dx_z,
 *      E    = sum of d2_i,  d2_i = (ex * ex + ey * ey) + ez * ez,  ex = (double)y_i.x -
 *             (double)q_i.x and so on: the search's own expression, the same bits.
 *    The pass's RECORD is {matched = m, rms = m > 0 ? dvsqrt(dvdiv(E, (double)m)) : 0}.
 *
 * The SOLVE (step 5), by one lane, from the S_ab of a pass:
 *   N00 = (Sxx + Syy) + Szz,  N11 = (Sxx - Syy) - Szz,  N22 = (Syy - Sxx) - Szz,
 *   N33 = (Szz - Sxx) - Syy,  N01 = Syz - Szy,  N02 = Szx - Sxz,  N03 = Sxy - Syx,
 *   N12 = Sxy + Syx,  N13 = Szx + Sxz,  N23 = Syz + Szy,  N symmetric (Horn 1987).
 *   V = the 4 x 4 identity.  DP_CLOUD_ALIGN_SWEEPS times, for (p, q) = (0,1), (0,2),
 *   (0,3), (1,2), (1,3), (2,3) in this order: if N_pq == 0.0 the rotation is
 *   skipped; otherwise
 *     theta = dvdiv(N_qq - N_pp, 2.0 * N_pq);
 *     t = dvdiv(theta >= 0 ? 1.0 : -1.0, fabs(theta) + dvsqrt(theta * theta + 1.0));
 *     c = dvdiv(1.0, dvsqrt(t * t + 1.0));  s = t * c;
 *     for the two k other than p and q, ascending:  u = N_kp, w = N_kq;
 *       N_kp = N_pk = c * u - s * w;  N_kq = N_qk = s * u + c * w;
 *     h = t * N_pq;  N_pp = N_pp - h;  N_qq = N_qq + h;  N_pq = N_qp = 0.0;
 *     for k = 0..3:  u = V_kp, w = V_kq;  V_kp = c * u - s * w;  V_kq = s * u + c * w.
 *   j = the index of the largest N_jj, the lowest on ties; v = column j of V;
 *   len = dvsqrt(((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3);  q_k = dvdiv(v_k, len);
 *   R00 = ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3,  R01 = 2.0 * (q1 * q2 - q0 * q3),
 *   R02 = 2.0 * (q1 * q3 + q0 * q2),  R10 = 2.0 * (q1 * q2 + q0 * q3),
 *   R11 = ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3,  R12 = 2.0 * (q2 * q3 - q0 * q1),
 *   R20 = 2.0 * (q1 * q3 - q0 * q2),  R21 = 2.0 * (q2 * q3 + q0 * q1),
 *   R22 = ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3:  the rotation of a quaternion,
 *   proper whatever the clouds are; a mirrored cloud never yields a reflection.
 *   scale = 1.0, or with DP_CLOUD_ALIGN_SCALE dvdiv(g, Sx), g = the sum in the order
 *   (a, b) = (x,x), (x,y), (x,z), (y,x), .. (z,z) of R_ba * S_ab, starting from the
 *   first product.  A_rk = scale * R_rk;  t_r = muq_r - ((A_r0 * mux_x + A_r1 * mux_y)
 *   + A_r2 * mux_z);  the new M = [A | t].
 *   DP_CLOUD_ALIGN_SWEEPS is 10.  On the test inputs of tests/cloudalign_ref.py
 *   (random, coplanar, collinear, mirrored, duplicated clouds) the reference's
 *   off-diagonal mass sqrt(sum of N_pq^2, p < q) is below 2^-50 of the largest
 *   |N_jj| after at most 4 sweeps and exactly zero after 6 (cyclic Jacobi
 *   converges quadratically once the off-diagonal part is small); 10 leaves a
 *   margin for clustered eigenvalues, and a sweep over a diagonal matrix skips
 *   every rotation, so the extra sweeps change no bit.
 *
 * The iteration.  M = init.  Step k = 0, 1, .. iterations - 1: a pass with M
 * writes trace[k]; then the call STOPS, keeping M, with stop_reason
 *   DP_CLOUD_ALIGN_STOP_PAIRS       when m < min_pairs;  otherwise
 *   DP_CLOUD_ALIGN_STOP_RMS         when k > 0, rms_tol > 0 and fabs(rms - rms of
 *                                   step k - 1) <= rms_tol;  otherwise
 *   DP_CLOUD_ALIGN_STOP_DEGENERATE  when Sx == 0, or the solve's scale is not
 *                                   finite and > 0, or an entry of the new M is
 *                                   not finite;
 * otherwise M becomes the solve's.  After the update of step iterations - 1 one
 * more pass writes trace[iterations], and stop_reason is
 * DP_CLOUD_ALIGN_STOP_ITERATIONS.  iterations_run = the number of updates made.
 * A pass's record is the residual BEFORE that step's update.  With n_source = 0
 * or n_target = 0 (not an error) stop_reason is DP_CLOUD_ALIGN_STOP_EMPTY, the
 * result is init and trace[0] = {0, 0}.
 * Outputs (host memory in both forms).  matrix: the final M, 12 doubles.  *scale:
 * the scale of the last update, 1.0 when none was made (init is not decomposed).
 * trace: iterations + 1 records, those after the last pass zero.  index and dist
 * (optional): c(i) and dist_i of the last pass, per source point.  Statistics:
 * dp_cloud_nearest's counters of the last pass (queries are the y_i), grid_cells
 * and max_cell_targets, iterations_run, stop_reason, grid_ms = device time of
 * the target grid, iterate_ms = of everything after it, the waits included.
 * The call waits once per pass, to read the pass's record and the solve's verdict
 * (24 bytes): that wait is what makes the early stop real.  Nothing else
 * crosses the bus before the end.
 * Errors (DP_E_ARG): dp_cloud_nearest's on the counts, pointers, strides, opts
 * and max_dist; iterations, min_pairs or rms_tol outside the ranges above; an
 * unknown flag; an init entry that is not finite; matrix, scale or trace NULL;
 * an output that equals an input; device form: one of d_index and d_dist given
 * without the other.
 * Host form: *index and *dist (pass NULL for both when not wanted) are
 * context-owned, valid until the next dp_cloud_align, dp_cloud_nearest or
 * destroy (NULL when n_source is 0).  Device form: device clouds, d_index and
 * d_dist caller buffers of n_source entries or both NULL; queued on `stream`
 * (NULL = the context's), and the call always waits.
 * Limits: point to point, no subsampling, no global search: a bad start is the
 * caller's init.  Scratch is dp_cloud_nearest's (shared with it) plus 20 bytes
 * per source point and the sum levels (88 bytes per 256 source points). */
#define DP_CLOUD_ALIGN_SCALE 1
#define DP_CLOUD_ALIGN_SWEEPS 10
#define DP_CLOUD_ALIGN_STOP_ITERATIONS 0
#define DP_CLOUD_ALIGN_STOP_RMS 1
#define DP_CLOUD_ALIGN_STOP_PAIRS 2
#define DP_CLOUD_ALIGN_STOP_DEGENERATE 3
#define DP_CLOUD_ALIGN_STOP_EMPTY 4
typedef struct dp_cloud_align_options {
    float max_dist;      /* trimming radius, world units (> 0, finite; no default) */
    int32_t iterations;  /* 1..1000                                               */
    int32_t min_pairs;   /* >= 3                                                  */
    int32_t flags;       /* DP_CLOUD_ALIGN_SCALE; another bit is DP_E_ARG         */
    double rms_tol;      /* >= 0, finite; 0 = never stop early                    */
} dp_cloud_align_options;
typedef struct dp_cloud_align_step {
    int64_t matched;
    double rms;
} dp_cloud_align_step;
typedef struct dp_cloud_align_stats {
    int64_t queries, targets;          /* those taking part, in the last pass   */
    int64_t skipped_queries, skipped_targets, matched, unmatched;
    int64_t grid_cells, max_cell_targets;  /* facts of the implementation, not of the spec */
    int64_t iterations_run, stop_reason;
    double grid_ms, iterate_ms;
} dp_cloud_align_stats;

int dp_cloud_align(dp_ctx *ctx, const void *source, int64_t n_source, int64_t source_stride,
                   const void *target, int64_t n_target, int64_t target_stride,
                   const dp_cloud_align_options *opts, const double *init, double *matrix, double *scale,
                   dp_cloud_align_step *trace, const int32_t **index, const float **dist,
                   dp_cloud_align_stats *stats);
int dp_cloud_align_device(dp_ctx *ctx, const void *d_source, int64_t n_source, int64_t source_stride,
                          const void *d_target, int64_t n_target, int64_t target_stride,
                          const dp_cloud_align_options *opts, const double *init, double *matrix, double *scale,
                          dp_cloud_align_step *trace, int32_t *d_index, float *d_dist,
                          dp_cloud_align_stats *stats, void *stream);

/* ---- nearest-triangle distances from points to a mesh surface ---------------------
 * No reference counterpart.  For every query point the nearest triangle of a
 * mesh within a radius, its distance and the closest point on it: the primitive
 * under the completeness of a mesh against a ground truth and under the
 * deviation between two meshes (mesh_compare and mesh_deviation in the Python
 * package, densify --eval-mesh-surface).  The conventions are dp_cloud_nearest's
 * except where stated.  All arithmetic is fp64, one IEEE rounding per operation,
 * in exactly the order written (the build has -ffp-contract=off); dvdiv and
 * dvsqrt are the IEEE-correct fp64 quotient and square root, (float) and
 * (double) the IEEE conversions.
 *
 * Inputs: n_queries points, three consecutive f32 at base + i * stride (bytes, a
 * multiple of 4, at least 12); n_vertices 16-byte dp_mesh_vertex records, of
 * which only pos is read; n_triangles index triples.  No view is read.
 *
 * Who takes part.  A query TAKES PART iff its three floats are finite; one that
 * does not gets index -1, dist +inf and closest (+inf, +inf, +inf) and counts in
 * skipped_queries.  A triangle is VALID, DEGENERATE or PROPER as in the smoothing
 * section (by its indices alone; no index is used as an address before its range
 * check); invalid and degenerate ones count in invalid_triangles and
 * degenerate_triangles.  A proper triangle TAKES PART iff its nine coordinates
 * are finite; the others count in nonfinite_triangles, those taking part in
 * `triangles`:  triangles + invalid_triangles + degenerate_triangles +
 * nonfinite_triangles = n_triangles.  A proper triangle whose positions coincide
 * or are collinear takes part: its edges answer for it.
 *
 * Distance of q to the triangle (a, b, c), everything widened to double first:
 *   ab = b - a, ac = c - a, bc = c - b, ca = a - c, ap = q - a, bp = q - b,
 *   cp = q - c (componentwise);  dot(u, v) = (ux*vx + uy*vy) + uz*vz;
 *   cross(u, v) = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx)   (dp_mesh_normals' order).
 *   Segment (s, e) with sp = q - s:  se = e - s;  den = dot(se, se);
 *     t = den > 0 ? dvdiv(dot(sp, se), den) : 0, then t < 0 becomes 0 and t > 1
 *     becomes 1;  r_k = sp_k - t * se_k;  d2 = dot(r, r);  point_k = (float)(s_k +
 *     t * se_k).  The segments are (a, b) with sp = ap and se = ab, (b, c) with bp
 *     and bc, (c, a) with cp and ca.
 *   Plane:  n = cross(ab, ac);  nn = dot(n, n).  The plane is USED iff
 *     nn > (dot(ab, ab) * dot(ac, ac)) * 2^-40  (the conditioning of the cross
 *     product: below it the edges describe the sliver to better than 10^-6 of its
 *     length) and dot(cross(ab, ap), n) >= 0 and dot(cross(bc, bp), n) >= 0 and
 *     dot(cross(ca, cp), n) >= 0.  Then s = dvdiv(dot(ap, n), nn);  r_k = s * n_k;
 *     d2 = dot(r, r);  point_k = (float)(q_k - r_k).
 *   The triangle's d2 and point are those of the smallest d2 among the plane (if
 *   used), (a, b), (b, c), (c, a), in that order; a later one replaces an earlier
 *   one only when strictly smaller.
 *
 * Candidates.  R = (double)max_dist, R2 = R * R, G = R + R * 2^-20.  With lo_k and
 * hi_k the smallest and the largest of the triangle's three f32 coordinates on
 * axis k, triangle T is a CANDIDATE of q iff
 *   (double)lo_k - G <= (double)q_k  and  (double)q_k <= (double)hi_k + G  on every axis k,
 *   and d2 <= R2 (inclusive).
 * The box test is part of the spec on purpose.  Mathematically it excludes no
 * triangle within max_dist, since the closest point lies in the box; it makes the
 * answer a function of the mesh, the queries and max_dist alone even for slivers
 * whose computed d2 is noise, so that a grid implementation can be proved equal
 * to brute force.
 * The answer of q is the candidate with the smallest d2; equal d2 goes to the
 * lowest triangle index.  index[q] = that triangle's index in the caller's array,
 * dist[q] = (float)dvsqrt(d2), closest[3q .. 3q + 2] = its point, and q counts in
 * matched.  A query with no candidate gets -1, +inf and (+inf, +inf, +inf) and
 * counts in unmatched.  The histogram is exactly dp_cloud_nearest's.
 * queries + skipped_queries = n_queries, matched + unmatched = queries.
 * n_queries = 0 and n_triangles = 0 are legal.
 *
 * Tie to dp_cloud_nearest: every vertex of a triangle starts one of its three
 * segments, and t = 0 gives the point-to-point d2 bit for bit, so with the same
 * max_dist dist[q] here is never above dp_cloud_nearest's against the vertices
 * that triangles taking part name.
 *
 * grid_cells (at most 2^24), grid_entries (triangle registrations, at most 8 *
 * n_triangles) and max_cell_entries describe the search grid of the
 * implementation, not the spec.  build_ms = device time of the grid's
 * construction, query_ms = of the queries' sort and walk.
 * Errors (DP_E_ARG): dp_cloud_nearest's (counts, strides, opts, max_dist,
 * hist_bins, flags, an output that equals an input), and vertices or triangles
 * NULL with a positive count; device form: d_index or d_dist NULL with n_queries
 * > 0.
 * Host form: *index, *dist (both required), *closest (3 floats per query; pass
 * closest = NULL when not wanted) and *hist are context-owned, valid until the
 * next dp_mesh_nearest or destroy.  Device form: caller buffers, d_closest and
 * d_hist optional; everything is queued on `stream` (NULL = the context's) and
 * the call waits only when stats != NULL.
 * Limits: one nearest triangle, unsigned distance.  Scratch is at most 8
 * registrations of 5 bytes per triangle, 16 bytes per query and the cell table
 * (8 bytes per cell, at most 2^24 + 1 cells), whatever the extent, max_dist and
 * the triangles' sizes are. */
typedef struct dp_mesh_nearest_options {
    float max_dist;     /* search radius, world units (> 0, finite; no default) */
    int32_t hist_bins;  /* 0 = no histogram; else 1..65536                     */
    int32_t flags;      /* none defined; non-zero is DP_E_ARG                  */
} dp_mesh_nearest_options;
typedef struct dp_mesh_nearest_stats {
    int64_t queries, skipped_queries, matched, unmatched;
    int64_t triangles, invalid_triangles, degenerate_triangles, nonfinite_triangles;
    int64_t grid_cells, grid_entries, max_cell_entries;  /* facts of the implementation, not of the spec */
    double build_ms, query_ms;
} dp_mesh_nearest_stats;

int dp_mesh_nearest(dp_ctx *ctx, const void *queries, int64_t n_queries, int64_t query_stride,
                    const dp_mesh_vertex *vertices, int64_t n_vertices, const int32_t *triangles,
                    int64_t n_triangles, const dp_mesh_nearest_options *opts, const int32_t **index,
                    const float **dist, const float **closest, const uint64_t **hist,
                    dp_mesh_nearest_stats *stats);
int dp_mesh_nearest_device(dp_ctx *ctx, const void *d_queries, int64_t n_queries, int64_t query_stride,
                           const dp_mesh_vertex *d_vertices, int64_t n_vertices, const int32_t *d_triangles,
                           int64_t n_triangles, const dp_mesh_nearest_options *opts, int32_t *d_index,
                           float *d_dist, float *d_closest, uint64_t *d_hist, dp_mesh_nearest_stats *stats,
                           void *stream);

/* ---- seed generation: Features::Matcher::GenerateSeeds ---
 * modules/features/matcher.cpp:18-43 with the default MatcherOptions
 * (matcher.h:21-32: ORB detector, kNN matcher, no direct epipolar matching,
 * 1.5 px epipolar distance, 16 px cells, 4 keypoints per cell).  Stages:
 *   DetectKeypoints   matcher.cpp:45-87   ORB::create(40000)->detect
 *   FilterKeypoints   matcher.cpp:89-153  per-cell best responses
 *   ComputeDescriptors matcher.cpp:155-183 ORB::create()->compute (rBRIEF)
 *   DefaultPairsList  matcher.cpp:185-204 (0,1),(0,2),..,(1,2),.. lexicographic
 *   MatchKeypoints    matcher.cpp:206-265 BruteForce-Hamming knnMatch k=2,
 *                                         d0 < 0.7f * d1
 *   FilterMatches     matcher.cpp:319-372 epipolar distance <= 1.5f, F from
 *                                         geometry/fundamental_matrix.cpp:6-53
 *   TriangulateMatches matcher.cpp:374-450 DLT, geometry/triangulation.cpp:15-34
 * DetectorType::AKAZE (matcher.cpp:56-60, 166-170: cv::AKAZE::create()
 * defaults -- MLDB 486 bits, threshold 0.001, 4 octaves x 4 sublevels, PM_G2)
 * is selected by detector_type = DP_DETECTOR_AKAZE: descriptors are then 64
 * bytes (486 bits, zero padded; dp_seed_descriptor_bytes), FilterKeypoints and
 * the matching stages are unchanged.  Its restated arithmetic is
 * oracle/or_akaze.c's header (parity unpinned against OpenCV).
 * OpenCV's ORB is restated, not reproduced bit-for-bit (OpenCV is absent from
 * the image; DESIGN.md "Seed generation" lists the restated semantics and the
 * points that are parity-unpinned; the rBRIEF sampling pattern is OpenCV's own
 * bit_pattern_31_, see dp_orb_pattern).  The
 * reference's unspecified orders (nth_element, omp critical push_back) are
 * fixed here: keypoints in (level, y, x) order, per-cell picks by (response
 * desc, index), seed points in (view, keypoint) order. */
typedef struct dp_matcher_options {
    int32_t n_features;             /* 40000 ORB::create(40000) matcher.cpp:62        */
    int32_t n_levels;               /* 8     cv::ORB default                          */
    double scale_factor;            /* 1.2   cv::ORB default                          */
    int32_t edge_threshold;         /* 31    cv::ORB default (border excluded)        */
    int32_t fast_threshold;         /* 20    cv::ORB default                          */
    int32_t cell_size;              /* 16    MatcherOptions::cell_size matcher.h:25   */
    int32_t max_keypoints_per_cell; /* 4     matcher.h:26                             */
    int32_t epipolar_matching;      /* 0     matcher.h:23 (1: DirectEpipolarMatching) */
    float max_epipolar_distance;    /* 1.5f  matcher.h:24                             */
    float nn_match_ratio;           /* 0.7f  matcher.cpp:217                          */
    int32_t matcher_type;           /* DP_MATCHER_KNN  MatcherOptions::matcher_type    */
    int32_t detector_type;          /* DP_DETECTOR_ORB MatcherOptions::detector_type   */
    float akaze_threshold;          /* 0.001f  AKAZE::create() detector threshold      */
} dp_matcher_options;
/* DetectorType (matcher.h:11, the reference's enum order) */
#define DP_DETECTOR_AKAZE 0
#define DP_DETECTOR_ORB 1
/* MatcherType (matcher.h:12, MatchKeypoints matcher.cpp:206-265):
 *  DP_MATCHER_KNN    BruteForce-Hamming knnMatch k = 2, ratio test d0 < 0.7 d1
 *  DP_MATCHER_FLANN  FlannBasedMatcher(LshIndexParams(12, 20, 2)).match, kept iff
 *                    distance < 30 (matcher.cpp:229-240).  LSH is approximate and
 *                    its hash tables come from FLANN's random generator, so no two
 *                    builds agree on its misses; this build answers the same query
 *                    exactly -- the nearest train descriptor by Hamming distance
 *                    (ties: lowest index, as BFMatcher), kept iff distance < 30 --
 *                    which LSH approximates (parity unpinned).  Both then go
 *                    through the same epipolar filter (FilterMatches). */
#define DP_MATCHER_KNN 0
#define DP_MATCHER_FLANN 1

/* the cv::KeyPoint fields the matcher reads (pt, response, angle, octave) */
typedef struct dp_keypoint {
    float x, y;        /* level-0 pixels                                        */
    float response;    /* Harris response (ORB HARRIS_SCORE)                    */
    float angle;       /* degrees, intensity-centroid orientation              */
    int32_t octave;    /* pyramid level                                        */
    int32_t reserved;
} dp_keypoint;

typedef struct dp_seed_stats {
    int64_t keypoints_detected;  /* after detect, all views                         */
    int64_t keypoints;           /* after FilterKeypoints                           */
    int64_t pairs;               /* view pairs                                      */
    int64_t ratio_matches;       /* kNN ratio-test survivors, all pairs             */
    int64_t matches;             /* after the epipolar filter                       */
    int64_t points;              /* triangulated seed points                        */
    double detect_ms, describe_ms, match_ms, triangulate_ms, total_ms;
} dp_seed_stats;

void dp_default_matcher_options(dp_matcher_options *mo);
/* The rBRIEF sampling pattern ComputeDescriptors uses: OpenCV 3.4's learned
 * bit_pattern_31_ (ORB::create()->compute, matcher.cpp:171-173), 512 points as
 * (x, y) int8 pairs; test i compares points 2i and 2i+1.  xy_out: 1024 bytes.
 * Host-only (no device needed). */
int dp_orb_pattern(int8_t *xy_out);
/* GenerateSeeds over the context's level-0 views.  *xyz_out (n x 3 doubles)
 * is context-owned, valid until the next dp_generate_seeds or destroy. */
int dp_generate_seeds(dp_ctx *ctx, const dp_matcher_options *mo, const double **xyz_out, int64_t *n_out,
                      dp_seed_stats *stats);
/* Stage results of the last dp_generate_seeds (context-owned, host copies);
 * descriptor rows are dp_seed_descriptor_bytes wide (32 ORB, 64 AKAZE).  An
 * AKAZE keypoint's `reserved` holds its evolution level (class_id). */
int dp_seed_keypoints(dp_ctx *ctx, int view, const dp_keypoint **kp, const uint8_t **desc32, int64_t *n);
int dp_seed_descriptor_bytes(dp_ctx *ctx);
int dp_seed_matches(dp_ctx *ctx, int pair, int32_t *first, int32_t *second, const int32_t **query_to_train,
                    int64_t *nq);

/* Standalone operators of the path.
 * BFMatcher(NORM_HAMMING).knnMatch(query, train, k=2) on 32-byte descriptors:
 * idx2/dist2 (nq x 2) hold the two nearest train rows by (distance, index);
 * -1 / -1 where train has fewer rows.  nt < 2^22. */
int dp_knn_match(dp_ctx *ctx, const uint8_t *query, int64_t nq, const uint8_t *train, int64_t nt,
                 int32_t *idx2, int32_t *dist2);
/* the same for descriptor_bytes 32 or 64 (AKAZE rows; nt < 2^21 for 64) */
int dp_knn_match_wide(dp_ctx *ctx, const uint8_t *query, int64_t nq, const uint8_t *train, int64_t nt,
                      int descriptor_bytes, int32_t *idx2, int32_t *dist2);
/* Geometry::ComputeFundamentalMatrix (fundamental_matrix.cpp:6-34), F 3x3 row-major. */
int dp_fundamental_matrix(const double P1[12], const double P2[12], double F[9]);
/* Geometry::DirectLinearTriangulation (triangulation.cpp:15-34), batched: point
 * i uses observations offsets[i] .. offsets[i+1]-1 (P: 12 doubles, obs: x, y
 * cast to float as the reference does). */
int dp_triangulate(dp_ctx *ctx, int64_t n_points, const int32_t *offsets, const double *P, const double *obs,
                   double *X);

/* ---- performance mode (north star: "LDS-staged image-pyramid tiles", "fused
 * conjugate-gradient steps", "fp16 pyramids") ---------------------------------
 * A second refine of the patch loop for throughput; parity mode (DP_MODE_EVAL
 * .. DP_MODE_EXPAND) stays the reference restatement.  It replaces
 * OptimizationOpenCV::Optimize (optimization_opencv.cpp:44-78, DownhillSolver
 * over depth/roll/pitch) and keeps the objective of the functor calc
 * (optimization_opencv.cpp:14-39: mean of 1 - NCC against texture 0, the
 * lowest-index scored view) and NCCScore's formula (error_measurements.cpp:
 * 36-60, 0.1 denominator floor).  The full arithmetic is oracle/or_fast.c;
 * in short, per patch:
 *  - gray planes: BGR2GRAY of the current level (the 14-bit fixed point of the
 *    parity path) stored as fp16 (biased by 1024), one SoA plane per view
 *    (dp_build_gray);
 *  - frame: e1 = the reference camera's x-axis projected onto the patch plane,
 *    e2 = n x e1, sample spacing one reference pixel (1/dx); pose (d, a, b):
 *    X = X0 + d (X0 - C_ref), plane normal n + a e1 + b e2, in scaled units
 *    d = x0 / (dx |X0 - C_ref|), a = x1 * 2/(n-1), b = x2 * 2/(n-1);
 *  - staging: per visible view (ascending, at most max_views) whose initial
 *    window corners project inside the image, a tile = the window's pixel
 *    bounding box + `margin` px (left edge even; footprint 4 ceil((tw+1)/2)
 *    (th+1) bytes; the margin is reduced until all tiles fit tile_budget
 *    bytes, then the longest fitting prefix of views is kept), copied once
 *    into LDS and used for the whole refine; samples clamp to the tile
 *    (BORDER_REPLICATE);
 *  - sample: per (view, pose) the window homography's first-order (affine)
 *    map about the window centre in fp32 (U0 = Ax / Az, axes (B - U0 Bz) / Az,
 *    one IEEE reciprocal), U = U0 + ti Ui + tj Uj by fmaf, 1/32 px (rounded
 *    to integers by one add of 2^23, clamped to the tile), bilinear on 8-bit
 *    gray, result in 1/16 gray levels; exact integer moments;
 *  - refine objective: the sum over the scored views of 1 - NCC, each NCC
 *    finished in fp32 and rounded to a multiple of 2^-24, summed exactly (the
 *    functor calc's mean without its constant 1/(m-1)); reported scores
 *    (FAST_EVAL, filter) use an fp64 finish;
 *  - refine: `iters` Polak-Ribiere+ conjugate-gradient steps with a two-probe
 *    line search (initial step ls_step, doubled on success, halved on
 *    failure) and, by `gradient`:
 *      1 (spec v4): the ANALYTIC gradient of the objective -- per
 *        sample the bilinear tap slopes times the window map's derivatives
 *        (bf16 coefficients per view and pose), as 16-bit integers Q (one unit
 *        = one gray level per scaled pose unit); per view exact integer sums
 *        (sum Q, sum b Q, sum (Q_anchor b + a Q)) and NCC's quotient rule in
 *        fp64, quantised to 2^-24 and summed exactly.  One evaluation with the
 *        gradient at the start and after every line search that moved x:
 *        E = 1 + 2 iters + (iterations after a moving line search);
 *      0 (spec v3, default): a forward-difference gradient (step fd_step): E = 1 +
 *        5 iters, less 3 per iteration after a line search that left x
 *        unchanged (the last gradient is reused: the differences would repeat it);
 *  - then Patch::InitRelatedImages (patch.cpp:19-49) at the new pose (its
 *    angle tests as cosine tests, x > cos(angle) with the cosines from the
 *    host libm; frame unit vectors by one reciprocal and products) and the
 *    fast filter: re-staged at the new pose (margin 0), one evaluation, views
 *    with NCC < ncc_threshold or that cannot be staged are dropped (no
 *    off-by-one), accepted iff >= min_visible views remain; score = mean NCC.
 * dp_refine_batch[_device] run DP_MODE_FAST_* with `cell` in [2, 16]. */
typedef struct dp_fast_options {
    int32_t iters;        /* 4     CG iterations                                    */
    int32_t margin;       /* 2     tile margin around the initial window, px       */
    int32_t tile_budget;  /* 6656  bytes of LDS tiles per patch (<= 16384; the
                                   kernel's arena is 6, 8 or 16 KiB by this value) */
    int32_t max_views;    /* 8     staged views of the refine (<= 32; r04: 32)      */
    float fd_step;        /* 0.5   forward-difference step, scaled units (gradient 0) */
    float ls_step;        /* 1.0   initial line-search step, scaled units           */
    int32_t densify;      /* 0     1: dp_densify runs the seed stage (at
                                   seed_cell_size) and every expansion (at
                                   expand_cell_size) with the fast refine, and so
                                   does the generation-at-a-time (multi-GPU) API */
    int32_t gradient;     /* 0     0: forward differences (spec v3), 1: analytic
                                   gradient (spec v4: better children from
                                   refined parents, worse from raw ones)          */
    int32_t filter_max_views; /* 32 staged views of the scoring evaluations (the
                                   filter after the refine, DP_MODE_FAST_EVAL);
                                   0 = max_views.  Spec v5 (r05): the refine
                                   stages at most max_views (default 8) so that
                                   its tiles keep their margin; the filter
                                   scores every view that fits the budget      */
} dp_fast_options;

void dp_default_fast_options(dp_fast_options *fo);
int dp_set_fast_options(dp_ctx *ctx, const dp_fast_options *fo);
/* fp16 gray planes of the current level for every view (built on demand by
 * the first fast call; explicit here so callers can time it).  The cached
 * planes follow dp_set_views*, dp_build_pyramid and dp_set_level only: a
 * caller that rewrites its dp_set_views_device planes in place must call
 * dp_build_gray again (it always rebuilds, after draining the device). */
int dp_build_gray(dp_ctx *ctx);
/* host copy (width*height fp16 values) of view `view`'s gray plane; the
 * planes hold 1024 + gray (biased fp16: the bits are 0x6400 | gray, so the
 * sampler reads integer taps without a conversion) */
int dp_read_gray(dp_ctx *ctx, int view, uint16_t *fp16_out);
/* Expand::ExpandPatch children (as dp_expand_batch) refined in performance
 * mode: DP_MODE_FAST_REFINE on the parent's visible set, cell =
 * expand_cell_size. */
int dp_fast_expand_batch(dp_ctx *ctx, const dp_patch *parents, int n, dp_patch *children, uint8_t *accept_out);
/* Work counters of the most recent performance-mode launch (device-counted; a
 * batch of device-resident densify generations counts as one launch):
 * patches = the launch's patches (four per parent of an expansion, whether the
 * parent expands or not); evals = the sum of their evals fields after the
 * launch (children and seeds start at 0, so the launch's evaluations; a patch
 * refined again brings its earlier count along);
 * view_evals = sum over patches and evaluations of the staged views sampled,
 * i.e. algorithmic bytes = view_evals * (n+1)^2 * 2 (fp16 texels);
 * staged_bytes = bytes the tiles copy from the gray planes (the compulsory
 * HBM traffic of the windows). */
typedef struct dp_fast_stats {
    int64_t patches;
    int64_t evals;
    int64_t view_evals;
    int64_t staged_bytes;
    int64_t clipped_stagings; /* stagings whose tiles did not fit tile_budget at the
                                 full margin (margin reduced or views dropped) */
} dp_fast_stats;
int dp_fast_last_stats(dp_ctx *ctx, dp_fast_stats *out);
int dp_fast_expand_batch_device(dp_ctx *ctx, const dp_patch *d_parents, int n, dp_patch *d_children,
                                uint8_t *d_accept, void *stream);

/* Elapsed device milliseconds of the most recent refine kernel launch, timed
 * with HIP events on the stream the kernel ran on. */
int dp_last_kernel_ms(dp_ctx *ctx, double *ms);

/* ---- synthetic scenes (build extension: deterministic test/bench input) -- */
typedef struct dp_synth_config {
    int32_t n_views;       /* V                                                  */
    int32_t width, height; /* image size                                         */
    int32_t kind;          /* 0 = textured plane, 1 = 3x3 tilted-facet heightfield */
    uint64_t seed;         /* RNG seed (default 20261015)                       */
    double spread_deg;     /* camera spread around the surface normal (35)      */
    double seed_stride_px; /* seed grid stride in each nominal ref view (32)    */
    double depth_noise;    /* relative seed depth noise sigma (0.005)           */
} dp_synth_config;

void dp_synth_default(dp_synth_config *cfg);
/* Cameras (V x 12 projection matrices). */
int dp_synth_cameras(const dp_synth_config *cfg, double *P_out);
/* Render view v as BGR8 on the host (OpenMP), rows of 3*width bytes. */
int dp_synth_render_host(const dp_synth_config *cfg, const double *P, int v, uint8_t *bgr_out);
/* Render view v as BGRA8 into device memory (height*width uint32). */
int dp_synth_render_device(dp_ctx *ctx, const dp_synth_config *cfg, const double *P, int v,
                           void *d_bgra, void *stream);
/* Seed points on the true surface with depth noise; returns count written
 * (at most cap); xyz_out may be NULL to query the count. */
int64_t dp_synth_seeds(const dp_synth_config *cfg, const double *P, double *xyz_out, int64_t cap);
/* Ground truth of the synthetic surface: height z(x, y) and the unit normal
 * (facing +z) at n points xy (n x 2); normal_out may be NULL.  Used to score
 * refine quality (tests, bench), never by the patch loop. */
int dp_synth_surface(const dp_synth_config *cfg, int64_t n, const double *xy, double *z_out, double *normal_out);

#ifdef __cplusplus
}
#endif
#endif /* DENSEPOINTS_H */
