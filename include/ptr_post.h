/* Post-processing of a rendered frame: the edge-avoiding a-trous wavelet denoiser on the first-hit feature buffers.
 *
 * The reference hands its beauty image plus first-hit albedo and normal to a learned denoiser (RenderSettings::denoiseEnabled,
 * DenoiserContext.mm).  The network cannot be carried over; the same inputs can.  This is the edge-avoiding a-trous wavelet filter of
 * Dammertz et al. 2010 with the spatial variance estimate of SVGF (Schied et al. 2017), guided by the buffers ptr_render_aovs writes.
 * Kernels: csrc/kernels/denoise.hip.  Host: csrc/host/denoise.cpp.  Restatement in numpy (the tests' reference): tests/denoise_ref.py.
 *
 * ---- The filter (kernel and restatement are written from this text) ----------------------------------------------------------------
 *
 * Inputs
 *   rgb     W*H*3 floats.
 *   albedo  W*H*4 floats.  w > 0.5 marks a hit.
 *   normal  W*H*4 floats.  xyz = n*0.5 + 0.5, w = hit distance z.
 *   These are exactly the buffers ptr_render and ptr_render_aovs return (ptr_abi.h, the rule at ptr_render_aovs: with PTR_METAL_PBR the
 *   albedo is the textured base colour, the normal the mapped one, and a cut-out shows what is seen through it).  Albedo and normal are
 *   taken to be finite.
 *   A pixel is a HIT pixel when albedo.w > 0.5, z > 0 and its three colour channels are finite; every other pixel is a MISS pixel.
 *   (So a pixel with a non-finite colour is a miss pixel: as a tap it has weight 0, as a centre it is copied through.)
 *
 * Parameters (PtrDenoiseParams)
 *   iterations      1..8   default 5    number of a-trous passes
 *   sigmaLuminance  > 0    default 4    luminance edge-stop scale
 *   sigmaNormal     > 0    default 128  normal edge-stop exponent
 *   sigmaDepth      > 0    default 1    depth edge-stop scale
 *   flags           bit 0  default 1    demodulate by albedo
 *
 * Prepare (per hit pixel p)
 *   With demodulation on: a = max(albedo.rgb, 1e-3) and c = rgb / a.  Otherwise a = 1 and c = rgb.
 *   Luminance: l = (0.2126 r + 0.7152 g) + 0.0722 b of c.
 *   Guide record: unit normal n = m / |m| with m = 2 * normal.xyz - 1 (n = 0 where |m| = 0), depth z.
 *   Depth slope g_p = max(g_x, g_y).  Along an axis, with z+ and z- the depths of the two neighbours one pixel away:
 *     both are in-image hit pixels:  |z+ - z-| / 2;   only one is:  |z(that one) - z_p|  (one-sided);   neither:  0.
 *   Variance v_p over the 7x7 window of in-image hit pixels q, row-major order (dy outer, dx inner, both ascending):
 *     weights k_q = wn * wz as defined below with step s = 1; the centre has k = 1;
 *     two-pass: m = sum(k l) / sum(k), then v = sum(k (l - m)^2) / sum(k).  (Not E[l^2] - E[l]^2: it cancels in float32.)
 *
 * A-trous pass i (s = 2^i, i = 0 .. iterations-1), per hit pixel p
 *   Taps (dx, dy) in {-2..2}^2 in row-major order (dy outer, dx inner, both ascending).  q = p + s * (dx, dy).
 *   Out-of-image taps and miss pixels are skipped.
 *   Kernel: h = [1/16, 1/4, 3/8, 1/4, 1/16] (x) itself, h(dx, dy) = h[dx] * h[dy].
 *   wn = max(0, n_p . n_q) ^ sigmaNormal,  n_p . n_q = (x x' + y y') + z z'
 *   wz = exp(-|z_p - z_q| / (sigmaDepth * (g_p * (s * |(dx, dy)|) + 1e-3 * z_p)))
 *   wl = exp(-|l_p - l_q| / (sigmaLuminance * sqrt(v_p) + 1e-6))
 *   w = ((h * wn) * wz) * wl.  The centre tap has w = h(0, 0).
 *   c' = sum(w c_q) / sum(w)
 *   v' = sum((w w) v_q) / (sum(w) sum(w))
 *   l is recomputed from c' (each pass computes l_p and l_q from the colours it reads).
 *
 * Finish
 *   out = c * a for hit pixels.
 *   Miss pixels are copied through unchanged.  They give nothing to any hit pixel.
 *
 * All arithmetic is float32, unfused, in the order written; sums run in tap order starting from 0.
 */
#ifndef PTR_POST_H
#define PTR_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_DENOISE_DEMODULATE 1u /* PtrDenoiseParams::flags bit 0 */
#define PTR_DENOISE_MAX_ITERATIONS 8u

typedef struct PtrDenoiseParams {
    uint32_t iterations;
    float sigmaLuminance;
    float sigmaNormal;
    float sigmaDepth;
    uint32_t flags;
} PtrDenoiseParams;

/* iterations 5, sigmaLuminance 4, sigmaNormal 128, sigmaDepth 1, flags PTR_DENOISE_DEMODULATE */
void ptr_denoise_default_params(PtrDenoiseParams* params);

/* Host buffers in, host buffer out (width*height*3 floats; out_rgb may alias rgb).  kernel_ms (nullable): the filter's kernels, timed
 * with device events.  Returns 0, or nonzero with a message in err: 1 for a bad argument (checked before any device call), 2 when
 * there is no such device (no CPU fallback). */
int ptr_denoise(const float* rgb, const float* albedo_rgba, const float* normal_rgba, uint32_t width, uint32_t height,
                const PtrDenoiseParams* params, int device, float* out_rgb, double* kernel_ms, char* err, size_t err_cap);

/* Device buffers in, device buffer out (d_out_rgb may equal d_rgb), on the device that owns d_rgb.  Asynchronous on `stream`
 * (a hipStream_t; NULL = the default stream): scratch memory is allocated and freed in stream order. */
int ptr_denoise_device(const void* d_rgb, const void* d_albedo, const void* d_normal, uint32_t width, uint32_t height,
                       const PtrDenoiseParams* params, void* d_out_rgb, void* stream, char* err, size_t err_cap);

/* Measurement (tools/denoise_bench.py): ptr_denoise_device run `warmup` + `runs` times on the default stream with every kernel between
 * two device events.  out_ms[0] = prepare, out_ms[1 + i] = a-trous pass i, out_ms[1 + iterations] = finish: mean milliseconds over the
 * timed runs.  out_tiled (nullable, same layout): 1 where the LDS-tiled kernel ran.  Synchronous. */
int ptr_denoise_timed(const void* d_rgb, const void* d_albedo, const void* d_normal, uint32_t width, uint32_t height,
                      const PtrDenoiseParams* params, void* d_out_rgb, uint32_t runs, uint32_t warmup, double* out_ms, uint32_t* out_tiled,
                      char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_POST_H */
