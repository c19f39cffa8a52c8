/* Adaptive sampling: a frame rendered in rounds over a list of the pixels that are still active.
 *
 * A uniform frame gives every pixel sppTotal samples.  An adaptive frame gives every pixel minSpp samples, measures the relative standard
 * error of each pixel mean's luminance from those samples (the recurrence of ptr_stats.h), and goes on sampling only the pixels whose
 * error - or a neighbour's - is above a threshold, stepSpp samples at a time, up to maxSpp.  A round is an ordinary pass of the
 * wavefront kernels whose local-pixel table is the active list: sample s of pixel p is the sample a uniform frame draws for (p, s), so
 * the hot kernels are untouched and every pixel of the result is a pixel of some uniform frame (see Outputs).
 * Kernels: csrc/kernels/adaptive.hip (k_adaptive_update, k_adaptive_select, k_adaptive_scan, k_adaptive_scatter, k_adaptive_finish).
 * Host: csrc/host/adaptive.cpp.  Restatement in numpy (the tests' reference): tests/adaptive_ref.py.
 *
 * Scope: one device, the whole image, the non-counting build of the kernels.  The same frame on several devices, bit for bit, is
 * ptr_render_multi_adaptive of ptr_multi.h; count_traversal is not supported.
 *
 * ---- The specification (kernels and restatement are written from this text) ---------------------------------------------------------
 *
 * Parameters (PtrAdaptiveParams): minSpp >= 2, maxSpp >= minSpp, stepSpp >= 1, threshold >= 0 and finite.
 *
 * Rounds.  Round 0 gives every pixel minSpp samples, sample indices 0 .. minSpp-1.  Round r >= 1 gives every ACTIVE pixel
 * min(stepSpp, maxSpp - n) more, n being the count all active pixels share (a pixel that stops never resumes).  The samples of pixel p
 * in a round are those of a uniform frame with the same indices.  The frame ends when the active list is empty or n = maxSpp.
 *
 * State per pixel, image order: sum (rgb), mean (rgb), M (rr, gg, bb, rg, rb, gb), n (uint32), e (float); all zero before round 0.
 *
 * Update, for each pixel active in the round, for each new sample x (rgb) in sample order, k = the sample's 1-based index in the frame:
 *
 *       sum    = sum + x                           (per channel)
 *       d      = x - mean                          (per channel)
 *       mean   = mean + d / float(k)
 *       e'     = x - mean
 *       M_ab  += d_a * e'_b                        for ab in rr, gg, bb, rg, rb, gb
 *
 *   and after the last sample of the round, with n the pixel's new count and K = (0.2126, 0.7152, 0.0722):
 *
 *       cov_ab = M_ab / (float(n) * float(n - 1))
 *       C      = the symmetric 3x3 matrix of cov    (C_gr = C_rg, C_br = C_rb, C_bg = C_gb)
 *       v      = sum over c in (r, g, b), d in (r, g, b) of (K_c * K_d) * C_cd      (c outer, d inner; the sum starts from 0)
 *       v      = 0 unless v is finite and v > 0
 *       l      = (0.2126 * mean_r + 0.7152 * mean_g) + 0.0722 * mean_b
 *       l      = 0 unless l > 0                     (so a NaN mean counts as 0)
 *       e      = sqrt(v) / (l + 1e-2)
 *
 *   e is the relative standard error of the luminance of the pixel mean; 1e-2 is the denominator offset of the project's relRMSE.
 *
 * Select, after every active pixel of the round has been updated, for each pixel p active in the round:
 *
 *       E = 0
 *       for q over the 3x3 window around p, in-image pixels only, row-major (dy outer, dx inner, both ascending):
 *           if e_q > E then E = e_q                 (a NaN is never taken; a pixel that stopped earlier contributes its last e)
 *       p stays active iff n_p < maxSpp and E > threshold
 *
 *   The dilation keeps a pixel sampling whose own variance is 0 by chance at a few samples while its neighbour's is not (the reason
 *   ptr_stats.h prefilters).
 *
 * Compact.  The next active list is the kept entries of the current list in the current list's order.  The first list is the local
 * pixel order of a one-partition frame: 8-row bands top to bottom, each walked in 8x8 blocks left to right, each block row-major
 * (on several devices every partition starts from its own bands in that order: ptr_multi.h).
 *
 * Outputs, in image order (row 0 = top), NOT the band layout:
 *       rgb   (width*height*3):            sum / float(n_p)
 *       cov   (width*height*6, nullable):  M_ab / (float(n_p) * float(n_p - 1))
 *       count (width*height uint32, nullable): n_p
 *   Pixel p's rgb and cov are bit for bit those of a uniform single-pass frame of n_p samples per pixel (ptr_render_bands_cov): the sum
 *   is the same additions in the same order as the resolve step's and the division is the same; the covariance is the recurrence and
 *   normalisation of ptr_stats.h.
 *
 * All arithmetic is float32, unfused, in the order written; division and square root are correctly rounded.
 */
#ifndef PTR_ADAPTIVE_H
#define PTR_ADAPTIVE_H

#include <stddef.h>
#include <stdint.h>

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_ADAPTIVE_INFO_ROUNDS 32

typedef struct PtrAdaptiveParams {
    uint32_t minSpp;   /* samples of round 0, >= 2 */
    uint32_t maxSpp;   /* no pixel gets more, >= minSpp */
    uint32_t stepSpp;  /* samples of a later round, >= 1 */
    float threshold;   /* a pixel goes on while the dilated relative error is above it; >= 0, finite */
} PtrAdaptiveParams;

typedef struct PtrAdaptiveInfo {
    uint32_t rounds;          /* rounds run (>= 1) */
    uint32_t pixelsAtMax;     /* pixels that reached maxSpp */
    uint64_t totalSamples;    /* sum of n_p over the image */
    uint32_t activeAfter[PTR_ADAPTIVE_INFO_ROUNDS];   /* length of the active list after each of the first 32 rounds */
} PtrAdaptiveInfo;

/* minSpp 8, stepSpp 8, threshold 0.05, maxSpp = max_spp (at least 8). */
void ptr_adaptive_default_params(PtrAdaptiveParams* out, uint32_t max_spp);

/* An adaptive frame into device buffers (image order; d_out_cov and d_out_count may be null).  stats (nullable): samples = sum of n_p,
 * times and launches added over the passes.  info (nullable).  A null scene / settings / params / d_out_rgb, a zero size and parameters
 * outside the ranges above are refused with 1 and a message that names the function, before any device call; 2 without a HIP device. */
int ptr_render_adaptive_device(PtrDeviceScene* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, void* d_out_rgb,
                               void* d_out_cov, void* d_out_count, void* stream, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                               size_t err_cap);

/* The same with host buffers. */
int ptr_render_adaptive(PtrDeviceScene* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, float* out_rgb,
                        float* out_cov, uint32_t* out_count, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err, size_t err_cap);

/* Test only: update -> select -> compact of one round (or of one sub-pass of a round) on synthetic data, without a scene, through the
 * kernels the renderer launches.  n_before: the count the listed pixels share; samples[round_spp][active_count][4] (rgb, w ignored) in
 * list order; with last_sub_pass = 0 only the update runs, e is left alone, and *out_next_count = active_count with out_next = list.
 * The five state arrays (sum[wh][3], mean[wh][3], m[wh][6], n[wh], e[wh]) are read and written in place.  out_next: active_count words;
 * words at and past *out_next_count are left as they were.  The list must name in-image pixels, each at most once. */
int ptr_adaptive_debug_round(uint32_t width, uint32_t height, const PtrAdaptiveParams* params, uint32_t n_before, uint32_t round_spp,
                             int last_sub_pass, const uint32_t* list, uint32_t active_count, const float* samples, float* sum, float* mean,
                             float* m, uint32_t* n, float* e, uint32_t* out_next, uint32_t* out_next_count, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_ADAPTIVE_H */
