/*
 * ptr_debug_pbr.h - test-only entry point of libptr_hip.so: the per-hit material of the textured metallic-roughness model on a batch
 * of rays, for the tests that hold it to a float64 statement of the rule (tests/pbr_hit_domain.py).  A header
 * and a signature table of its own, like every entry point added after ptr_abi.h and ptr_debug.h: those two keep their sizes.
 */
#ifndef PTR_DEBUG_PBR_H
#define PTR_DEBUG_PBR_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-hit material of the textured metallic-roughness model (csrc/kernels/wavefront.hip applyPbrTextures) at the closest hit of a
 * batch of rays, whatever the settings' metalSemantics.  in n*20 words: floats {origin xyz, direction xyz, cone width, cone spread}, then
 * uint32 {random state, material index to shade with (0xFFFFFFFF: the hit's own), instantiation (0: applyPbrTextures<false> without
 * gradients; 1: applyPbrTextures<true> with the row's own)}, floats {uv gradients of set 0 {dudx, dvdx, dudy, dvdy}, of set 1}, uint32
 * {valid bits: bit k = set k has gradients}.  The kernel traces the closest hit, reconstructs the surface and calls the production
 * function with wo = -normalize(direction) and the hit distance, as k_shade does.  out n*32 words: floats {hit (1/0), t}, uint32 {mesh,
 * triangle} as PtrHit reports them, floats {bu, bv, front face, geometric normal xyz, the hit's shading normal xyz, textured (1: a mesh hit
 * shaded with a metallic-roughness material in a scene with textures; else 0 and the rest but the random state 0), base colour rgb,
 * roughness, emissive rgb, metallic, transmission, occlusion, shading normal xyz, two-sided, alpha-test discard}, uint32 {random state
 * afterwards, basis of the normal map: 0 no normal map, 1 the vertex tangent, 2 the uv derivatives, 3 an arbitrary frame, + 4 when the
 * mapped normal was turned to the geometric side}, 0.  The material outputs are 0 where the hit is discarded. */
int ptr_debug_pbr_hits(PtrDeviceScene* scene, const float* in, uint64_t n, float* out, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DEBUG_PBR_H */
