/*
 * ptr_debug_path.h - test-only entry point of libptr_hip.so: the path state of the wavefront integrator (csrc/kernels/wavefront.hip
 * shadeSlot: medium stack, packed flags word, Russian roulette, lastPdf / lastDelta / specDepth, and when radiance reaches `accum` and
 * `itemAccum`), vertex by vertex, for the tests that hold that bookkeeping to a float64 statement of it (tests/path_state_ref.py).
 * A header and a signature table of its own, like every entry point added after ptr_abi.h and ptr_debug.h.
 */
#ifndef PTR_DEBUG_PATH_H
#define PTR_DEBUG_PATH_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_PATH_STATE_WORDS 48u        /* words per slot and iteration of ptr_debug_path_states */
#define PTR_PATH_MAX_PIXELS (1u << 20)  /* the most pixels it takes */

/* Sample `sample` of the n pixels `pixels` (y * width + x each) through the production kernels and launchers, driven by the production
 * loop (tracePass: k_generate, then k_extend, k_shade, k_connect - with the chain kernel when MNEE secondary is on - per iteration) over
 * a pool of exactly n slots in one group, without the tail kernels; busy lists as that loop chooses.  With n work items and n slots
 * k_generate assigns item i to slot i and no slot claims a second item.  After every iteration the streams are joined and the pool is
 * copied out.  out_states: max_iterations * n * 48 words, iteration k of slot i at (k * n + i) * 48:
 *   0..3 ray0 {next origin, direction x}, 4..7 ray1 {direction y, z, lastPdf, bits(flags)}, 8..9 hit {t, bits(hit word)} (what this
 *   iteration's k_extend found along the ray of the previous snapshot, and its k_shade shaded), 10..13 thr {throughput, bits(rng)}, 14..17 accum {radiance, bits(item)},
 *   18..21 medium (zero without the medium stack), 22..23 cone (zero without one), 24..28 the kind word of record slots 0..4 (dir.w bits;
 *   meaningful where the pending bit of the flags is set), 29 flushItem, 30..31 0, 32..46 the `a` row (rgb) of record slots 0..4 as
 *   k_connect left it, 47 0.
 * Iterations past max_iterations run but are not recorded.  *out_iterations: the iterations the loop ran.  out_items n*4: itemAccum.
 * Non-zero, before any launch, for a NULL argument, n == 0, n > PTR_PATH_MAX_PIXELS, max_iterations == 0 or a pixel outside the image. */
int ptr_debug_path_states(PtrDeviceScene* scene, const PtrSettings* settings, const uint32_t* pixels, uint64_t n, uint32_t sample,
                          uint32_t max_iterations, uint32_t* out_states, uint32_t* out_iterations, float* out_items, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DEBUG_PATH_H */
