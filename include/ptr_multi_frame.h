/* Resumable frames on several devices: the per-pixel sample state of an adaptive frame (ptr_frame.h) kept on all devices of a node
 * between calls, each device holding the bands ptr_multi.h gives it.  One handle, one scene preparation, one upload per device: a
 * 16-spp preview goes on to 256 spp, a threshold is tightened, a render is checkpointed and continued on another number of devices,
 * without rendering the first samples again and without uploading the scene again.
 * Kernels: those of ptr_frame.h, ptr_adaptive.h and ptr_multi.h, and csrc/kernels/multi.hip's k_multi_state_pack / k_multi_state_unpack
 * (bodies in csrc/kernels/multi.h).  Host: csrc/host/multi_frame.cpp, with ptr_frame.h's round loop and count classes
 * (csrc/host/frame_rounds.cpp, csrc/host/frame_classes.h), the exchange, the gather and the partition threads of multi.cpp
 * (csrc/host/multi_host.h) and csrc/host/round_barrier.h.  Restatement in numpy (the tests' reference): tests/multi_frame_ref.py.
 *
 * Scope: the devices of one process, the non-counting build of the kernels; the bands of a partition are fixed for the frame's life.
 *
 * ---- The specification (kernels and restatement are written from this text) ---------------------------------------------------------
 *
 * A PtrMultiFrame belongs to one scene description, one PtrSettings, whose width and height are fixed for its life, and a list of P
 * devices: P partitions.
 *
 * Partitions, bands and each partition's first list are those of ptr_multi.h, word for word: partition p owns the 8-row bands b with
 * b mod P = p; its first list is its own pixels, its bands top to bottom, each walked in 8x8 blocks left to right, each block row-major.
 * Update, Select, e, E and the Outputs are those of ptr_adaptive.h.  Accumulate, Refine, Resolve, Export / Import and Reset mean what
 * they mean in ptr_frame.h.
 *
 * State.  Each partition holds the state of ptr_frame.h - sum, mean, M, n, e - of its own pixels, in image-order arrays.  Its e array
 * knows the rows of other partitions only through the halo; what its arrays hold on any other row is never read.  The state starts at
 * zero.
 *
 * Halo invariant.  Whenever a partition runs Select (the start-list Select of a Refine included), the row above and the row below each
 * of its bands, where those rows are in the image, hold their owners' CURRENT e.  It is kept in two halves, as in ptr_multi.h:
 *   publish  a partition that changed e makes the first and the last row of each of its bands known to the others - whole rows.  That
 *            is: behind the last sub-pass of an Accumulate, behind the last sub-pass of the Update of a Refine round, behind an Import,
 *            behind a Reset (which publishes zeros);
 *   collect  a partition that is about to select reads the rows above and below its bands from what their owners published last and
 *            writes them into its own e array.
 * Between a publish and the collect that must see it, and between a collect and the next publish, all partitions meet.  With P = 1
 * there is no neighbour and no exchange.
 *
 * Accumulate(spp): that of ptr_frame.h on every partition over its first list; publish.
 *
 * Refine(minSpp, maxSpp, stepSpp, threshold):
 *
 *       if the frame is empty: Accumulate(minSpp) on every partition (with its publish); all partitions meet
 *       otherwise minSpp is not read, and every pixel must have n >= 2
 *       collect;  L_p = Select over partition p's first list;  all partitions meet and sum |L_p|
 *       while some L_p is not empty:
 *           n_min = the smallest n over ALL lists
 *           S_p   = the entries of L_p with n == n_min, in L_p's order.  It may be empty: such a partition does no device work in this
 *                   round and still meets the others
 *           k     = min(stepSpp, maxSpp - n_min)
 *           Update over S_p (samples n_min .. n_min + k - 1; sub-passes as in ptr_frame.h);  publish;  all partitions meet
 *           collect;  Select on S_p only, merged into L_p in L_p's order;  all partitions meet and sum |L_p|
 *
 *   PtrAdaptiveInfo of a Refine is that of ptr_frame.h with |L| = the sum of |L_p|.
 *
 * Bit for bit.  For every P and any sequence of calls, the five state arrays (each pixel taken from its owner) are those of a
 * single-device PtrFrame given the same calls; so are the resolved rgb, cov and count, and every PtrAdaptiveInfo: rounds, activeAfter
 * (summed over the partitions), totalSamples, pixelsAtMax.  The union of the L_p is the single-device L in another order, and nothing
 * observable depends on that order.
 *
 * Resolve: the Outputs of ptr_adaptive.h in image order, each pixel from its owner; the state stays.  albedo / normal are the first-hit
 * feature buffers of sample 0 (ptr_render_aovs), rendered by the first partition's resident scene.
 *
 * Export / Import: the five arrays of ptr_frame_export in image order, each pixel from its owner; Import gives each partition its own
 * bands and publishes.  A checkpoint does not depend on P.  The law: export from P partitions -> import into Q partitions, or into a
 * PtrFrame, or the reverse -> continue gives the bits of the single-device frame that was never interrupted.
 * The state travels between a partition and the host as ONE dense buffer in band layout ([bands_p][8][width], rows of a ragged last band
 * outside the image neither read nor written), planar: sum [B][3], mean [B][3], M [B][6], n [B], e [B], one plane after the other, B the
 * partition's band pixels (14 words per pixel).  k_multi_state_pack / k_multi_state_unpack move the partition's own pixels between it and
 * the image-order state.
 *
 * Reset: the state back to zero on every partition; settings of the same size replace the stored ones.
 *
 * Devices.  n_devices <= 0 means all visible devices; more than are visible is refused with 2, more than PTR_MULTI_MAX_PARTS with 1;
 * never more partitions than bands.  These are the rules of ptr_render_multi.
 *
 * Errors.  Null pointers (the nullable ones are named), a zero size, spp == 0, parameters outside the ranges of ptr_adaptive.h, a
 * non-uniform frame given to accumulate, a pixel with n < 2 given to refine, another size given to reset, an empty or over-long id
 * list and an id at or past the visible count are refused with 1 and a message that starts with the function's name, before any device
 * call; 2 and "no CPU fallback" without a HIP device.  Output buffers are left untouched in both cases and the frame is as it was.
 * A failure on one device ends the call on all of them and is reported with that device's id; after such a failure every call on the
 * frame but release refuses with 1.
 */
#ifndef PTR_MULTI_FRAME_H
#define PTR_MULTI_FRAME_H

#include <stddef.h>
#include <stdint.h>

#include "ptr_abi.h"
#include "ptr_adaptive.h"
#include "ptr_frame.h"
#include "ptr_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrMultiFrame PtrMultiFrame;

/* An empty frame for `scene` and `settings` on n_devices devices (see Devices).  The scene is prepared once and uploaded to every
 * device concurrently; scenes, streams, state and exchange memory live as long as the frame.  `scene` is not read after the call. */
int ptr_multi_frame_create(const PtrSceneDesc* scene, const PtrSettings* settings, int n_devices, PtrMultiFrame** out_frame, char* err,
                           size_t err_cap);
void ptr_multi_frame_release(PtrMultiFrame* frame);

/* Reset.  settings may be null (the stored ones stay). */
int ptr_multi_frame_reset(PtrMultiFrame* frame, const PtrSettings* settings, char* err, size_t err_cap);

/* Accumulate.  stats (nullable): the slowest partition's time, launches summed, the samples of this call. */
int ptr_multi_frame_accumulate(PtrMultiFrame* frame, uint32_t spp, PtrRenderStats* stats, char* err, size_t err_cap);

/* Refine.  stats and info are nullable. */
int ptr_multi_frame_refine(PtrMultiFrame* frame, const PtrAdaptiveParams* params, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                           size_t err_cap);

/* Resolve into host buffers: out_rgb width*height*3; out_cov (width*height*6), out_count (width*height uint32), out_albedo and
 * out_normal (width*height*4 each; refused on a frame without a scene) are nullable. */
int ptr_multi_frame_resolve(PtrMultiFrame* frame, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo, float* out_normal,
                            char* err, size_t err_cap);

/* Resolve into image-order buffers on the FIRST device of the frame (d_out_cov and d_out_count nullable) on `stream`, a stream of that
 * device, which is joined before the call returns: ptr_denoise_cov_device can follow without a host round trip. */
int ptr_multi_frame_resolve_device(PtrMultiFrame* frame, void* d_out_rgb, void* d_out_cov, void* d_out_count, void* stream, char* err,
                                   size_t err_cap);

/* Size and counts (no device call: the frame keeps the number of pixels at every count on the host) and, in multi_info (nullable), the
 * partitions of the last accumulate, refine or resolve: samples added, seconds, of those waiting; stagedParts of the last resolve. */
int ptr_multi_frame_info(const PtrMultiFrame* frame, PtrFrameInfo* out, PtrMultiInfo* multi_info);

/* Export / Import: sum[wh][3], mean[wh][3], m[wh][6], n[wh], e[wh], image order; none nullable. */
int ptr_multi_frame_export(PtrMultiFrame* frame, float* sum, float* mean, float* m, uint32_t* n, float* e, char* err, size_t err_cap);
int ptr_multi_frame_import(PtrMultiFrame* frame, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e,
                           char* err, size_t err_cap);

/* Test only: create on an explicit list of 1 .. PTR_MULTI_MAX_PARTS device ids, with the semantics of ptr_multi_debug_adaptive_on: an id
 * may appear more than once, which lets a one-GPU machine run every partition and the exchange, and an id given as -(id + 1) sends that
 * partition's bands through the pinned-host staging path of a resolve's gather.  A list longer than the image has bands leaves the
 * partitions past the last band without pixels. */
int ptr_multi_frame_debug_create_on(const PtrSceneDesc* scene, const PtrSettings* settings, const int* device_ids, int n,
                                    PtrMultiFrame** out_frame, char* err, size_t err_cap);

/* Test only: the scene-less frame of ptr_frame_debug_create on partitions.  samples[sample_count][height][width][4] holds rgb (w
 * ignored); the accumulators of a pass are gathered from it.  A sample index at or past sample_count is refused with 1. */
int ptr_multi_frame_debug_create(uint32_t width, uint32_t height, const float* samples, uint32_t sample_count, const int* device_ids, int n,
                                 PtrMultiFrame** out_frame, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_MULTI_FRAME_H */
