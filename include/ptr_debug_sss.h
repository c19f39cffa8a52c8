/*
 * ptr_debug_sss.h - test-only entry points of libptr_hip.so: the random-walk subsurface path of the Metal integrator (PTR_METAL_SSS with
 * sssMode == 2; csrc/kernels/bsdf.h sssWalkBegin / sssWalkStep and the part of shadeSlot that parks, resumes and ends a walk), function
 * by function and walk by walk, for the tests that hold it to a float64 statement of the rule (tests/sss_walk_ref.py, DESIGN.md section
 * 4.5b).  A header and a signature table of its own, like every entry point added after ptr_abi.h and ptr_debug.h.
 *
 * All three run in the instantiation launchShade picks for the settings (the Metal-semantics one exactly when a Metal-only model is on)
 * and return non-zero, before any launch, for a NULL argument, n == 0 or settings->sssMaxSteps > 64.
 */
#ifndef PTR_DEBUG_SSS_H
#define PTR_DEBUG_SSS_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_SSS_MAX_STEPS 64u    /* the largest sssMaxSteps the probes take */
#define PTR_SSS_BEGIN_IN 12u
#define PTR_SSS_BEGIN_OUT 16u
#define PTR_SSS_STEP_IN 20u
#define PTR_SSS_STEP_OUT 24u
#define PTR_SSS_WALK_STEP 24u    /* words per recorded step of ptr_debug_sss_walks */
#define PTR_SSS_WALK_FINAL 24u   /* words per sample of its final record */

/* sssWalkBegin.  in n*12 floats {point, entry normal, wo, incident}.  out n*16 floats {outcome (0 fallback, 1 sample, 2 walking); then,
 * the two being exclusive, columns 1..8 as ptr_debug_sample_bsdf lays a sample out {direction, weight, pdf, isDelta} when the outcome is
 * 1, and when it is 2 the walk state {direction (1..3), throughput (4..6), 0, 0}; walk position (9..11, outcome 2); 0 (12..15)}.  What an
 * outcome does not define reads 0.  out_states: the random state afterwards. */
int ptr_debug_sss_walk_begin(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* rng_states, uint64_t n,
                             float* out, uint32_t* out_states, char* err, size_t err_cap);

/* sssWalkStep with maxSteps = settings->sssMaxSteps as given (0 included: the function itself takes it as 1).  in n*20 words: floats {walk
 * position, direction, throughput}, uint32 {step}, floats {hitBoundary (non-zero: a hit), hitT, hit point, outward normal, 0, 0}.  out n*24
 * words: floats {outcome, walk position, direction, throughput}, uint32 {step}, floats {exit sample: direction, weight, pdf, hasExit, exit
 * point}, 0, 0: the walk state as the function left it whatever the outcome, the sample 0 unless the outcome is 1. */
int ptr_debug_sss_walk_step(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* rng_states, uint64_t n,
                            float* out, uint32_t* out_states, char* err, size_t err_cap);

/* The whole first bounce of the camera samples xys n*3 {x, y, sample}, by the device code shadeSlot calls: cameraRay, the closest-hit
 * traversal, reconstruct, then sssWalkBegin where shadeSlot would call it (a front-face hit of a random-walk material) and a loop of
 * max(sssMaxSteps, 1) rounds of one closest-hit query and one sssWalkStep (a kernel each, the loop on the host: the wavefront's own
 * shape; the step limit has ended every walk by then); the end as shadeSlot ends it: the exit sample, or the ordinary sample
 * with the parked shading normal (a walk abandoned) or at the hit itself (no walk, or the coat sample), the next origin by sssExitOrigin
 * or offsetOrigin, clampThroughput.  It takes no light sample: it is meaningful only on scenes with no rectangle light and no sampled
 * environment, where shadeSlot draws nothing between the hit and the walk, and whose first hits are neither emitters nor textured
 * metallic-roughness surfaces nor dielectrics with the medium stack on (such a sample reads unsupported = 1 and nothing else).
 * out_steps n * step_cap * 24 words, step k of sample i at (i * step_cap + k) * 24: what sssWalkStep received and made of it: floats
 * {walk position, direction, throughput}, uint32 {step}, floats {hitBoundary, hitT, hit point, outward normal}, uint32 {random state
 * before}, floats {outcome}, uint32 {random state afterwards}, 0, 0, 0.  Steps past step_cap are not recorded (queries still counts them).
 * out_final n*24 words: floats {first hit (1/0), walk started (1/0), closest-hit queries of the walk, final outcome (of the last
 * sssWalkStep, or of sssWalkBegin when no query followed; -1 without a first hit), path goes on (1: a next ray exists), next origin, next
 * direction, path throughput afterwards}, uint32 {random state}, floats {the next ray escapes the scene (one more closest-hit query),
 * unsupported, the entry normal parked for the fallback sample xyz}, uint32 {random state after the camera ray}, 0, 0, 0. */
int ptr_debug_sss_walks(PtrDeviceScene* scene, const PtrSettings* settings, const uint32_t* xys, uint64_t n, uint32_t step_cap, float* out_steps,
                        float* out_final, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DEBUG_SSS_H */
