/* Temporal accumulation that carries the covariance of the pixel mean: the history of ptr_temporal.h holds, beside (rgb, length), the
 * covariance of its colour, propagated by the blend weights, reprojected through the same taps and returned in the layout of
 * ptr_stats.h, so that ptr_denoise_cov can be told how noisy the accumulated frame is, pixel by pixel; and with a variance on both
 * sides the filter can tell a history that no longer fits the frame (a light that moved) from one that is merely noisy.
 *
 * The handle is the PtrTemporal of ptr_temporal.h, made by ptr_temporal_create_cov instead of ptr_temporal_create: release, reset,
 * ptr_debug_temporal_records and the pose snapshot apply unchanged.  A handle is one kind for life: ptr_temporal_step* refuses a handle
 * that carries covariance, ptr_temporal_step_cov* one that does not.  One step is k_surface, k_temporal_accumulate_cov
 * (csrc/kernels/temporal.hip), the pose snapshot.  Host: csrc/host/temporal.cpp.  Restatement in numpy (the tests' reference):
 * tests/temporal_cov_ref.py.  Kernel and restatement are written from the text below.
 *
 * ---- The rule (k_temporal_accumulate_cov) ----------------------------------------------------------------------------------------------
 *
 * Steps 1-7 of ptr_temporal.h stand, with its inputs, its dot, its finite and its order.  Further inputs: the frame's covariance `cov`,
 * six floats per pixel (rr, gg, bb, rg, rb, gb: the covariance of the pixel MEAN, ptr_stats.h); the covariance history, six floats per
 * pixel; rejectSigma.  Further outputs: out_cov and the stored covariance history.
 *
 *   Cc         the six values of cov at the pixel, each replaced by 0 when it is not finite
 *   lum(x)     (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b
 *   lumvar(C)  with k = (0.2126, 0.7152, 0.0722) and C the symmetric 3x3 matrix of six values (C_gr = C_rg, C_br = C_rb, C_bg = C_gb):
 *              the sum over c in (r, g, b), d in (r, g, b) of (k_c * k_d) * C_cd, c the outer loop, d the inner, the sum starting from 0;
 *              replaced by 0 unless it is finite and > 0
 *
 * 1. MISS pixel: out_cov = 0, and the stored covariance history is 0.
 * 2. NO HISTORY, and every RESET (of step 3, 4 or 6, or by the consistency test below): out_cov = Cc.
 * 6. Beside B, Sc and Sn:  Sv_j = sum of b * (the tap's covariance history)_j for the six j, over the same counting taps in the same
 *    order, starting from 0.  When B > 0:
 *      H_j = Sv_j / B
 *      Consistency test, after hist and H are known and before the blend:
 *        d = lum(c) - lum(hist);  V = lumvar(Cc) + lumvar(H)
 *        when rejectSigma > 0 and d * d > (rejectSigma * rejectSigma) * V the pixel is RESET: out = c, length = 1, out_cov = Cc.
 *        (A comparison that is false because a term is NaN or infinite does not reject.)
 *      Blend, otherwise: with a = 1 / N' as in ptr_temporal.h and k = 1 - a
 *        out_cov_j = (k * k) * H_j + (a * a) * Cc_j;  a result that is not finite is replaced by Cc_j.
 * 7. The stored covariance history is out_cov.
 *
 * All arithmetic is float32, unfused, in the order written.  Which taps count is that of ptr_temporal.h, so with rejectSigma = 0 out_rgb,
 * the length and the colour history are bit for bit those of k_temporal_accumulate.
 *
 * Why it is this rule:
 *   - History and frame are independent samples, so the variance of the blend k * hist + a * c is the weighted sum of their variances
 *     with the SQUARED weights.  On a settled surface that is the covariance of the mean of the N' frames: 1 / N' of a frame's.
 *   - The four taps are combined linearly (b / B, not its square), as SVGF does: neighbouring histories share samples after they have
 *     been resampled a few times, so they are not independent, and squaring the tap weights would understate the variance.
 *   - A false rejection costs noise and never bias: the pixel is the frame's own estimate again.  That noise is reported honestly in
 *     out_cov (it is Cc), so ptr_denoise_cov filters that pixel harder than its settled neighbours.
 *
 * Memory: a handle that carries covariance holds, beside the 128 B per pixel of ptr_temporal.h, two ping-ponged covariance histories
 * of 24 B per pixel each (unpadded: a plane of 16 B (rr, gg, bb, rg) and a plane of 8 B (rb, gb) per pixel, read with one 16 B and one
 * 8 B load per tap): 176 B per pixel in all.
 */
#ifndef PTR_TEMPORAL_COV_H
#define PTR_TEMPORAL_COV_H

#include "ptr_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrTemporalCovParams {
    float rejectSigma; /* >= 0 and finite, default 3: the consistency test's threshold in standard deviations; 0 = never reject */
    uint32_t flags;    /* 0 */
} PtrTemporalCovParams;

void ptr_temporal_cov_default_params(PtrTemporalCovParams* params);
/* Host only.  0, or 1 with a message for a value outside the ranges above (NaN included) or a null argument. */
int ptr_temporal_cov_check_params(const PtrTemporalCovParams* params, char* err, size_t err_cap);

/* ptr_temporal_create for a handle that carries covariance.  params, cov_params NULL: the defaults.  Same return codes. */
int ptr_temporal_create_cov(PtrDeviceScene* scene, uint32_t width, uint32_t height, const PtrTemporalParams* params,
                            const PtrTemporalCovParams* cov_params, PtrTemporal** out, char* err, size_t err_cap);

/* ptr_temporal_step_device with the frame's covariance.  d_cov and d_out_cov hold W*H*6 floats in image order (the layout of
 * ptr_stats.h: d_out_cov goes straight into ptr_denoise_cov_device), are 8 B aligned and may be the same buffer, like d_rgb and
 * d_out_rgb; two that overlap otherwise are refused.  Everything else - the other buffers, the stream, info, what is refused (before
 * any device work, with the history as it was) - is as in ptr_temporal_step_device, every buffer held to the same rule. */
int ptr_temporal_step_cov_device(PtrTemporal* temporal, const PtrSettings* settings, const void* d_rgb, const void* d_cov, void* d_out_rgb,
                                 void* d_out_cov, void* d_out_length, void* d_out_albedo, void* d_out_normal, void* stream,
                                 PtrTemporalInfo* info, char* err, size_t err_cap);
/* The same step on host buffers (out_rgb may alias rgb, out_cov may alias cov; out_length, out_albedo, out_normal, info may be NULL).
 * Synchronous. */
int ptr_temporal_step_cov(PtrTemporal* temporal, const PtrSettings* settings, const float* rgb, const float* cov, float* out_rgb,
                          float* out_cov, float* out_length, float* out_albedo, float* out_normal, PtrTemporalInfo* info, char* err,
                          size_t err_cap);

/* ---- test-only probe ----
 * k_temporal_accumulate_cov alone on host-given buffers: the arguments of ptr_debug_temporal_accumulate, and cov_params; cov W*H*6;
 * cov_history W*H*6 (image order, six floats per pixel).  Out: also out_cov W*H*6 and out_cov_history W*H*6. */
int ptr_debug_temporal_accumulate_cov(uint32_t width, uint32_t height, const PtrTemporalParams* params, const PtrTemporalCovParams* cov_params,
                                      int has_history, const float* rgb, const float* cov, const float* cur_records, const float* prev_records,
                                      const float* history, const float* cov_history, const float* cam_cur, const float* cam_prev, int device,
                                      float* out_rgb, float* out_cov, float* out_length, float* out_history, float* out_cov_history, char* err,
                                      size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_TEMPORAL_COV_H */
