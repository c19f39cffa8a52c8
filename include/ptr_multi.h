/* Frames on several devices that carry more than an image: the covariance of the pixel means (ptr_stats.h) and adaptive sampling
 * (ptr_adaptive.h), with the first-hit feature buffers the denoiser (ptr_post.h) wants.  ptr_render_multi (ptr_abi.h) renders a uniform
 * image on all devices of a node; these calls do the same for a frame that can be sampled adaptively and denoised with its own variance.
 * Kernels: csrc/kernels/multi.hip (k_multi_halo_pack, k_multi_halo_unpack, k_multi_finish_bands, k_multi_interleave,
 * k_multi_gather_items), bodies in csrc/kernels/multi.h.  Host: csrc/host/multi.cpp, csrc/host/round_barrier.h.
 * The tests' reference is the single-device restatement tests/adaptive_ref.py: the frame does not depend on the number of partitions.
 *
 * Scope: the devices of one process.  The multi-process path (bench.py --gpus N) and the counting kernels are not supported, and the
 * bands of a partition are fixed for the frame (partSamples shows the imbalance adaptive sampling leaves).
 *
 * ---- The specification -----------------------------------------------------------------------------------------------------------------
 *
 * Partitions and first lists.  Partition p of P owns the 8-row bands b with b mod P = p (ptr_part_band_count of them).  Its first
 * active list is its own pixels in its local-pixel order: its bands top to bottom, each walked in 8x8 blocks left to right, each block
 * row-major.  With P = 1 this is the first list of ptr_adaptive.h.
 *
 * Rounds.  All partitions share the round number and the count n of ptr_adaptive.h: round 0 gives every pixel minSpp samples, round
 * r >= 1 gives every active pixel min(stepSpp, maxSpp - n) more.  A partition whose list is empty stays in the protocol and does no
 * device work.  The protocol ends when every list is empty or n = maxSpp.  Update is that header's, per partition, over its own list,
 * in sub-passes when a round's accumulators do not fit one pass.
 *
 * Halo.  Select looks at the 3x3 window of the error e, and every band edge is a partition edge.  After the last sub-pass of a round a
 * partition publishes e for every pixel of the first and the last row of each of its bands - whole rows, so a pixel that stopped earlier
 * contributes its last e; a partition with an empty list leaves what it published before.  Once every partition has published, each
 * partition reads the row above and the row below each of its bands, where those rows are in the image, and writes them into its own
 * image-order e array.  Only then does it run select and compact of ptr_adaptive.h on its own list.  With P = 1 there is no neighbour
 * and no exchange.
 *
 * Outputs.  rgb, cov and count are in image order and defined exactly as in ptr_adaptive.h; consequently they are bit for bit the
 * outputs of ptr_render_adaptive on one device, for every P.  PtrAdaptiveInfo is the single-device frame's: the same rounds,
 * activeAfter[r] the sum over the partitions, the same totalSamples and pixelsAtMax.  The uniform frame of ptr_render_multi_cov is bit
 * for bit ptr_render_bands_cov of one partition; its rgb is ptr_render_multi's.
 *
 * AOVs.  albedo / normal are the first-hit feature buffers of sample 0 (ptr_render_aovs: width*height*4 floats each), rendered by the
 * first partition's already uploaded scene, so a caller that denoises does not prepare and upload the scene a second time.
 *
 * Devices.  n_devices <= 0 means all visible devices; more than are visible is refused with 2, more than PTR_MULTI_MAX_PARTS with 1;
 * never more partitions than bands.  These are the rules of ptr_render_multi.
 *
 * Errors.  Null pointers, a zero size, spp < 2, bad PtrAdaptiveParams, an empty or over-long id list and an id at or past the visible
 * count are refused with 1 and a message that starts with the function's name, before anything is allocated or launched; a machine
 * without a HIP device gives 2 and "no CPU fallback".  Output buffers are left untouched in both cases.  A
 * failure on one device ends the frame on all of them and is reported with that device's id.
 */
#ifndef PTR_MULTI_H
#define PTR_MULTI_H

#include <stddef.h>
#include <stdint.h>

#include "ptr_abi.h"
#include "ptr_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_MULTI_MAX_PARTS 64

typedef struct PtrMultiInfo {
    uint32_t parts;                                     /* partitions the frame ran on */
    uint32_t stagedParts;                               /* partitions whose bands reached the first device through pinned host memory */
    uint64_t partSamples[PTR_MULTI_MAX_PARTS];          /* samples partition p traced (the sum of n over its pixels) */
    double partRenderSeconds[PTR_MULTI_MAX_PARTS];      /* from its first launch to the hand-over of its bands, waits included */
    double partWaitSeconds[PTR_MULTI_MAX_PARTS];        /* of those, spent waiting for the other partitions (0 for a uniform frame) */
} PtrMultiInfo;

/* A uniform frame of spp >= 2 samples per pixel over several devices with the covariance of the pixel means: out_rgb width*height*3,
 * out_cov (nullable) width*height*6 {rr, gg, bb, rg, rb, gb}, image order.  out_albedo / out_normal (nullable): see AOVs.  stats
 * (nullable) as ptr_render_multi fills it.  multi_info (nullable). */
int ptr_render_multi_cov(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, int n_devices, int verbose, float* out_rgb,
                         float* out_cov, float* out_albedo, float* out_normal, PtrRenderStats* stats, PtrMultiInfo* multi_info, char* err,
                         size_t err_cap);

/* An adaptive frame over several devices.  out_cov, out_count (width*height uint32), out_albedo, out_normal, stats, adaptive_info and
 * multi_info are nullable.  stats: the slowest partition's time, launches summed, samples = the sum of n_p. */
int ptr_render_multi_adaptive(const PtrSceneDesc* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, int n_devices,
                              int verbose, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo, float* out_normal,
                              PtrRenderStats* stats, PtrAdaptiveInfo* adaptive_info, PtrMultiInfo* multi_info, char* err, size_t err_cap);

/* Test only: the two calls above on an explicit list of 1 .. PTR_MULTI_MAX_PARTS device ids, with the semantics of
 * ptr_debug_render_multi_on: an id may appear more than once, which lets a one-GPU machine run the whole path (exchange included), and
 * an id given as -(id + 1) sends that partition's bands through the pinned-host staging path of the final gather.  A list longer than
 * the image has bands leaves the partitions past the last band without pixels. */
int ptr_multi_debug_cov_on(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, const int* device_ids, int n,
                           float* out_rgb, float* out_cov, float* out_albedo, float* out_normal, PtrRenderStats* stats,
                           PtrMultiInfo* multi_info, char* err, size_t err_cap);
int ptr_multi_debug_adaptive_on(const PtrSceneDesc* scene, const PtrSettings* settings, const PtrAdaptiveParams* params,
                                const int* device_ids, int n, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo,
                                float* out_normal, PtrRenderStats* stats, PtrAdaptiveInfo* adaptive_info, PtrMultiInfo* multi_info,
                                char* err, size_t err_cap);

/* Test only: the whole protocol without a scene.  The partition loop of ptr_render_multi_adaptive - the same kernels, exchange, finish
 * and gather - on samples[maxSpp][height][width][4] (rgb, w ignored): the accumulators of a pass are gathered from `samples` into list
 * order by k_multi_gather_items instead of being traced.  out_cov, out_count and adaptive_info are nullable. */
int ptr_multi_debug_adaptive_frame(uint32_t width, uint32_t height, const PtrAdaptiveParams* params, const float* samples,
                                   const int* device_ids, int n, float* out_rgb, float* out_cov, uint32_t* out_count,
                                   PtrAdaptiveInfo* adaptive_info, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_MULTI_H */
