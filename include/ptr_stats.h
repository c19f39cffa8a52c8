/* Per-pixel sample statistics of a rendered frame: the covariance of the pixel mean, and the denoiser of ptr_post.h run on it.
 *
 * Every pixel sample of a frame has an accumulator of its own in device memory until the frame is resolved (PathPool::itemAccum).
 * The render entry points of this header read them once more, in sample order, and return beside the image the sample covariance of
 * each pixel's MEAN: how far the value ptr_render returns for the pixel is expected to be from its limit.  Its luminance projection is
 * the variance the denoiser's luminance edge-stop needs; ptr_denoise_cov uses it in place of the 7x7 spatial estimate of ptr_post.h.
 * Kernels: csrc/kernels/stats.hip (k_resolve_cov), csrc/kernels/denoise.hip (k_denoise_prepare_cov).  Host: csrc/host/stats.cpp,
 * csrc/host/denoise.cpp.  Restatements in numpy (the tests' references): tests/stats_ref.py, tests/denoise_cov_ref.py.
 *
 * ---- The covariance (kernel and restatement are written from this text) ------------------------------------------------------------
 *
 * Per pixel, with x_1 .. x_n its per-sample accumulators (rgb; what the resolve step sums) in sample order, n = spp >= 2:
 *
 *   mean_0 = 0, M_0 = 0
 *   for k = 1 .. n:
 *       d      = x_k - mean_{k-1}                  (per channel)
 *       mean_k = mean_{k-1} + d / float(k)
 *       e      = x_k - mean_k
 *       M_ab  += d_a * e_b                         for ab in rr, gg, bb, rg, rb, gb
 *   cov_ab = M_ab / (float(n) * float(n - 1))
 *
 * All arithmetic is float32, unfused, in the order written.  cov is the unbiased sample covariance divided by n: the covariance of the
 * mean of the n samples.  A frame rendered in several passes continues the recurrence from pass to pass (k counts the samples of the
 * whole frame), so cov does not depend on how the frame is split into passes, on the size of the path pool or on the partition.
 *
 * Layout: six floats per pixel in the order rr, gg, bb, rg, rb, gb.  Band buffers follow out_rgb with 6 in place of 3,
 * [localBand][PTR_BAND_ROWS][width][6]; the padding rows of the last band are zero.
 *
 * ---- The denoiser on the measured variance -----------------------------------------------------------------------------------------
 *
 * ptr_denoise_cov is the filter of ptr_post.h with another variance v_p in its prepare step.  Decode, hit / miss rule, guide record,
 * depth slope, the a-trous passes and finish are those of ptr_post.h.  `cov` is width*height*6 floats in image order.
 *
 *   Per hit pixel q, with a the albedo divisor of prepare (1 without demodulation) and k = (0.2126, 0.7152, 0.0722):
 *     g_c = k_c / a_c                                           for c in r, g, b
 *     C   = the symmetric 3x3 matrix of cov at q                (C_gr = C_rg, C_br = C_rb, C_bg = C_gb)
 *     v_q = sum over c in (r, g, b), d in (r, g, b) of (g_c * g_d) * C_cd      (c outer, d inner; the sum starts from 0)
 *     v_q = 0 unless v_q is finite and v_q > 0
 *   (v_q is the variance of the demodulated luminance of the pixel mean.)
 *   v_p = sum(w_q v_q) / sum(w_q) over the 3x3 window of in-image hit pixels q, row-major order (dy outer, dx inner, both ascending),
 *     w = 1/4 at the centre, 1/8 at the four edge neighbours, 1/16 at the four corners; both sums start from 0.
 *   (The prefilter of SVGF: at 2-4 spp many dark pixels have a sample variance of exactly 0 by chance and would never be filtered.)
 *
 * All arithmetic is float32, unfused, in the order written.
 */
#ifndef PTR_STATS_H
#define PTR_STATS_H

#include <stddef.h>
#include <stdint.h>

#include "ptr_abi.h"
#include "ptr_post.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ptr_render_bands_device with a second output.  d_out_cov: device buffer of band_count * PTR_BAND_ROWS * width * 6 floats.  spp < 2,
 * a null pointer and a bad partition are refused with 1 and a message that names the function, before any device call. */
int ptr_render_bands_cov_device(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index,
                                uint32_t part_count, void* d_out_rgb, void* d_out_cov, void* stream, int count_traversal,
                                PtrRenderStats* stats, char* err, size_t err_cap);

/* ptr_render_bands with a second output (host buffers).  out_rgb_bands is bit for bit what ptr_render_bands returns. */
int ptr_render_bands_cov(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index, uint32_t part_count,
                         float* out_rgb_bands, float* out_cov_bands, int count_traversal, PtrRenderStats* stats, char* err,
                         size_t err_cap);

/* ptr_denoise with the variance taken from `cov` (width*height*6 floats).  Same return codes. */
int ptr_denoise_cov(const float* rgb, const float* albedo_rgba, const float* normal_rgba, const float* cov, uint32_t width,
                    uint32_t height, const PtrDenoiseParams* params, int device, float* out_rgb, double* kernel_ms, char* err,
                    size_t err_cap);

/* ptr_denoise_device with the variance taken from d_cov. */
int ptr_denoise_cov_device(const void* d_rgb, const void* d_albedo, const void* d_normal, const void* d_cov, uint32_t width,
                           uint32_t height, const PtrDenoiseParams* params, void* d_out_rgb, void* stream, char* err, size_t err_cap);

/* Test only: the frame's per-sample accumulators, out_samples[spp][height][width][3] in image order (row 0 = top).  Fails (1) when the
 * frame needs more than one pass: the accumulators of earlier passes are gone by then. */
int ptr_stats_debug_samples(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, float* out_samples, char* err,
                            size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_STATS_H */
