/*
 * densepoints_probe.h -- diagnostic entry points of libdensepoints.so.
 *
 * Host-compiled instances of the SAME arithmetic the gfx950 kernels run
 * (densepoints_amd/csrc/dp_geom.h, dp_detmath.h), so the CPU test suite can
 * check the product's spec against the oracle without a GPU, plus a device
 * probe that runs the math on the GPU for the host==device check.  Not part
 * of the reference surface.
 */
#ifndef DENSEPOINTS_PROBE_H
#define DENSEPOINTS_PROBE_H

#include "densepoints.h"

#ifdef __cplusplus
extern "C" {
#endif

void dp_probe_sincos(double x, double *s, double *c);
double dp_probe_acos(double x);
/* window texture of one view (BGR8 host image): returns 1 + gray[cell*cell], or 0 if empty */
int dp_probe_texture(const double P[12], int32_t W, int32_t H, const uint8_t *bgr,
                     const double corners[12], int cell, int32_t *gray);
double dp_probe_ncc(int32_t N, int32_t Sa, int32_t Saa, int32_t Sb, int32_t Sbb, int32_t Sab,
                    double denom_min);
/* device run of sincos/acos/sqrt over n inputs (out: 4*n doubles s,c,acos(x),sqrt|x|) */
int dp_probe_math_device(const double *x, int n, double *out);
/* device run of the texel loop's bilinear + BGR2GRAY on n explicit texels:
 * taps_a/taps_b = BGRA8 pixel pairs (x0, x0+1) of rows y0 / y1, fxy = fx | fy << 5 */
int dp_probe_texel_device(const uint64_t *taps_a, const uint64_t *taps_b, const uint32_t *fxy, int n,
                          int32_t *gray);
/* device run of the performance mode's fp32 reciprocal (v_rcp_f32 + one
 * Newton step) on n inputs >= 2^-20; the kernel's spec is IEEE 1.0f / x */
int dp_probe_recip_f32_device(const float *x, int n, float *out);
/* device run of the performance mode's spec-v4 gradient quantiser:
 * rint(dncc 2^24) clamped to int32 (maxNum / minNum, NaN -> INT32_MIN) */
int dp_probe_grad_q24_device(const double *dncc, int n, int32_t *out);
/* 32-bit LDS reads at 2-byte alignment on the device (out: 4 x 64 words) */
int dp_probe_lds_unaligned_device(uint32_t *out256);
/* Whole planes of seed generation's image stage on the views set on the
 * context, borders included (keypoints lie well inside and cannot show them).
 * Both run dp_generate_seeds' own launch sequence and stop after the planes.
 * out = NULL asks for the size only; wh receives (w, h); cap = elements of out.
 * AKAZE scale space: view v, evolution level l, which = 0 Lt, 1 Lx, 2 Ly,
 * 3 Ldet (fp32); DP_E_ARG where the view has no such level. */
int dp_probe_akaze_plane(dp_ctx *c, int view, int level, int which, float *out, int64_t cap, int32_t wh[2]);
/* ORB's gray pyramid (u8) of n_levels levels at scale_factor: cvtColor at
 * level 0, then the INTER_LINEAR resizes level to level */
int dp_probe_orb_level(dp_ctx *c, int view, int level, int n_levels, double scale_factor, uint8_t *out,
                       int64_t cap, int32_t wh[2]);
/* The stages of seed generation after the detector, on keypoints the caller
 * plants: per-view offsets, pair plan, matching (kNN / FLANN / direct
 * epipolar), the match tables, triangulation and the read-back.  It uploads
 * counts[v] keypoints per view (n_views = the context's views; kp and desc
 * view-major, descriptor_bytes = 32 or 64 per row) as a detector's result and
 * then runs the same code as dp_generate_seeds.  Only the projection matrices
 * of the views are used: the pixels are never read and the coordinates need
 * not lie inside them.  mo = NULL takes the defaults; its detector fields are
 * ignored.  Points and stats as dp_generate_seeds (keypoints_detected =
 * keypoints = the planted count, detect_ms = describe_ms = 0);
 * dp_seed_keypoints, dp_seed_matches and dp_probe_seed_t2q read the rest.
 * DP_E_ARG: a null pointer, a width other than 32 or 64, a negative count, a
 * view with 2^22 (32-byte) / 2^21 (64-byte) or more rows, n_views != views. */
int dp_probe_seed_stages(dp_ctx *c, int n_views, const int32_t *counts, const dp_keypoint *kp, const uint8_t *desc,
                         int descriptor_bytes, const dp_matcher_options *mo, const double **xyz_out, int64_t *n_out,
                         dp_seed_stats *stats);
/* The train -> query table of one pair after dp_generate_seeds or
 * dp_probe_seed_stages: per keypoint of the pair's second view the first
 * (lowest) query matched to it, or -1; *nt = its length.  Valid until the
 * next call on the context. */
int dp_probe_seed_t2q(dp_ctx *c, int pair, const int32_t **t2q, int64_t *nt);
/* diagnostic builds (-DDP_STAMPS) only: per-phase s_memtime cycle sums of the
 * refine kernel since the last call (0 maps, 1 texture 0, 2 other views,
 * 3 NCC finish, 6 patches, 7 whole patch); DP_E_STATE otherwise */
int dp_debug_stamps(uint64_t *out8);
/* The survivor compaction of dp_densify_iterate on host arrays: out receives
 * patches[i] with keep[i] != 0, unchanged and in index order (room for n
 * records); *n_out = their count. */
int dp_probe_keep_gather(dp_ctx *ctx, const dp_patch *patches, int64_t n, const uint8_t *keep, dp_patch *out,
                         int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
