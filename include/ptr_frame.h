/* Resumable frames: the per-pixel sample state of an adaptive frame kept on the device between calls.
 *
 * Every other render entry point is one shot: it builds a frame, returns it and throws the per-pixel state away.  A PtrFrame keeps that
 * state - the running sum, mean, M, n and e of ptr_adaptive.h - so that a caller can look at a 16-spp preview and go on to 256, tighten
 * the adaptive threshold after seeing the result, write a convergence series from one render, or stop now and continue later, without
 * rendering the first samples again.  Sample s of pixel p is a pure function of (seed, p, s) and the update of ptr_adaptive.h folds
 * samples in sample order, so a frame continued in any number of calls is BIT FOR BIT the frame rendered in one call.
 * Kernels: csrc/kernels/frame.hip (k_frame_class_min, k_frame_split, k_frame_merge; bodies in frame.h) and those of adaptive.hip.
 * Host: csrc/host/frame.cpp, with the round loop of csrc/host/frame_rounds.cpp and the count classes of csrc/host/frame_classes.h, which
 * the frame on several devices (ptr_multi_frame.h) shares.  Restatement in numpy (the tests' reference): tests/frame_ref.py.
 *
 * Scope: one device, the whole image, the non-counting build of the kernels.
 *
 * ---- The specification (kernels and restatement are written from this text) ---------------------------------------------------------
 *
 * A PtrFrame belongs to one PtrDeviceScene and one PtrSettings, whose width and height are fixed for its life.  It owns the per-pixel
 * state of ptr_adaptive.h in image order - sum (rgb), mean (rgb), M (rr, gg, bb, rg, rb, gb), n (uint32), e (float): 104 B per pixel -
 * the list buffers and the compaction's scratch.  The state is the frame's own, not the scene's: several frames may exist per scene,
 * and any other render call on the scene between two calls on a frame leaves the frame as it was.  The state starts at zero.
 *
 * Update, Select, the first-list order and the Outputs are those of ptr_adaptive.h, word for word.
 *
 * Accumulate(spp), spp >= 1.  Requires a uniform frame (all n_p equal; n their common value).  Every pixel gets the samples with indices
 * n .. n + spp - 1: the Update of ptr_adaptive.h over the full list in first-list order.  When the accumulators do not fit one pass the
 * samples arrive in sub-passes in sample order; e is computed on the last sub-pass, from the count n + spp.
 *
 * Refine(minSpp, maxSpp, stepSpp, threshold), the resumable adaptive loop:
 *
 *       if the frame is empty (all n_p = 0): Accumulate(minSpp)
 *       otherwise minSpp is not read, and every pixel must have n_p >= 2 (its e is then the error of n_p samples)
 *       L = the pixels p, in first-list order, with n_p < maxSpp and E_p > threshold       (the start list; E is the 3x3 dilation of the
 *                                                                                          stored e over the whole image: Select)
 *       while L is not empty:
 *           n_min = the smallest n_p in L
 *           S     = the entries of L with n_p == n_min, in L's order
 *           k     = min(stepSpp, maxSpp - n_min)
 *           every pixel of S gets the samples with indices n_min .. n_min + k - 1: Update over S (sub-passes as above; e of S is written
 *               on the last sub-pass)
 *           Select on S only: an entry of S stays iff n_p < maxSpp and E_p > threshold; E reads the current e of all neighbours,
 *               whatever class they are in
 *           L = the old L in its old order without the dropped entries of S     (entries of L that are not in S stay, untouched and in
 *                                                                                place)
 *
 *   PtrAdaptiveInfo of a Refine: rounds = the iterations of the loop, plus one if the first Accumulate ran; activeAfter[r] = |L| after
 *   each round (the start list's length is round 0's figure when the first Accumulate ran); totalSamples = the samples added by this
 *   call; pixelsAtMax = the pixels with n_p == maxSpp at the end.
 *
 *   Two consequences.  (1) On an empty frame, or on a uniform frame with n = minSpp, S equals L in every round: the call is
 *   ptr_render_adaptive bit for bit - rgb, cov, count, rounds and activeAfter (on the frame that already holds minSpp samples the
 *   rounds and activeAfter are those of ptr_render_adaptive without its round 0, which this call did not run).  (2) A second call with a lower threshold or a higher
 *   maxSpp picks stopped pixels up again, each at its own count, the lowest class first; after any sequence of calls pixel p is the pixel
 *   of a uniform single-pass frame of n_p samples.
 *
 * Resolve: the Outputs of ptr_adaptive.h from the state - rgb = sum / float(n_p), cov = M_ab / (float(n_p) * float(n_p - 1)), count = n_p,
 * image order; for n_p < 2 cov is whatever that formula gives.  The state is left as it was: a frame can be resolved any number of times
 * and continued afterwards.
 *
 * Export / Import: the five state arrays in host memory, a checkpoint.  Import checks pointers only; the values are the caller's
 * responsibility.  The law: export -> release -> create -> import -> continue gives the bits of the frame that was never interrupted.
 *
 * Reset: the state back to zero; settings of the same size replace the stored ones (a host uses this when the camera moves).
 *
 * All arithmetic is float32, unfused, in the order written; division and square root are correctly rounded.
 */
#ifndef PTR_FRAME_H
#define PTR_FRAME_H

#include <stddef.h>
#include <stdint.h>

#include "ptr_abi.h"
#include "ptr_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrFrame PtrFrame;

typedef struct PtrFrameInfo {
    uint32_t width, height;
    uint32_t minCount, maxCount;   /* the smallest and the largest n_p */
    uint64_t totalSamples;         /* the sum of n_p over the image */
    uint32_t uniform;              /* 1 when all n_p are equal */
    uint32_t reserved;
} PtrFrameInfo;

/* Errors, for every function below: null pointers (the nullable ones are named), a zero size, spp == 0, parameters outside the ranges of
 * ptr_adaptive.h, a non-uniform frame given to accumulate and a pixel with n_p < 2 given to refine are refused with 1 and a message that
 * starts with the function's name, before any device call; 2 and "no CPU fallback" without a HIP device.  An image of more than
 * 0xFFFF0000 pixels is refused. */

/* An empty frame for `scene` (which must outlive it) and `settings`. */
int ptr_frame_create(PtrDeviceScene* scene, const PtrSettings* settings, PtrFrame** out_frame, char* err, size_t err_cap);
void ptr_frame_release(PtrFrame* frame);

/* Reset.  settings may be null (the stored ones stay); another width or height is refused with 1. */
int ptr_frame_reset(PtrFrame* frame, const PtrSettings* settings, char* err, size_t err_cap);

/* Accumulate.  stats (nullable): the samples, times and launches of this call. */
int ptr_frame_accumulate(PtrFrame* frame, uint32_t spp, void* stream, PtrRenderStats* stats, char* err, size_t err_cap);

/* Refine.  stats and info are nullable. */
int ptr_frame_refine(PtrFrame* frame, const PtrAdaptiveParams* params, void* stream, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                     size_t err_cap);

/* Resolve into device buffers (width*height*3 floats; width*height*6 floats or null; width*height uint32 or null) on `stream`, which is
 * joined before the call returns ... */
int ptr_frame_resolve_device(PtrFrame* frame, void* d_out_rgb, void* d_out_cov, void* d_out_count, void* stream, char* err, size_t err_cap);

/* ... and into host buffers. */
int ptr_frame_resolve(PtrFrame* frame, float* out_rgb, float* out_cov, uint32_t* out_count, char* err, size_t err_cap);

/* Size and counts; no device call (the frame keeps the number of pixels at every count on the host). */
int ptr_frame_info(const PtrFrame* frame, PtrFrameInfo* out);

/* Export / Import: sum[wh][3], mean[wh][3], m[wh][6], n[wh], e[wh]; none nullable. */
int ptr_frame_export(PtrFrame* frame, float* sum, float* mean, float* m, uint32_t* n, float* e, char* err, size_t err_cap);
int ptr_frame_import(PtrFrame* frame, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e, char* err,
                     size_t err_cap);

/* Test only: a frame without a scene on `device`.  samples[sample_count][height][width][4] holds rgb (w ignored); the accumulators of a
 * pass are gathered from it into list order instead of being traced.  Everything downstream of the accumulators is the product path: the
 * same kernels, the same loop, the same accumulate, refine, resolve, export and import calls.  Asking for a sample index at or past
 * sample_count (an accumulate past it, a refine whose maxSpp is above it) is refused with 1. */
int ptr_frame_debug_create(uint32_t width, uint32_t height, const float* samples, uint32_t sample_count, int device, PtrFrame** out_frame,
                           char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_FRAME_H */
