// Host-callable launchers of the wavefront kernels (defined in wavefront.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "ptr_abi.h"

namespace ptrk {

struct LaunchConfig {
    uint32_t traceGrid;      // blocks of kTraceBlock threads for extend / connect (grid-stride)
    uint32_t* spill;         // traversal stack spill area: (kTraversalStackDepth-kLdsStackLevels) * traceGrid*kTraceBlock words
    uint32_t* workCounters;  // [2] work-queue heads of k_extend / k_connect, zeroed by the host before each launch
    int refillBelow;         // persistent waves hand out new rays once fewer than this many lanes are traversing
    uint32_t feederChunk = 256;   // slots a wave claims per atomic on the work head
};

void launchGenerate(const RenderParams& rp, const PathPool& pool, hipStream_t stream);
// The node format launchExtend / launchConnect instantiate the persistent kernels for: 0 float, 1 quantised binary, 2 four-wide, 3 the
// counting build (which reads the scene's flag at run time)
int traversalNodeFormat(const SceneView& sc, bool count);
// aliveOut (nullable): += number of live slots the launch traced (host termination check)
void launchExtend(const SceneView& sc, const PathPool& pool, const LaunchConfig& cfg, uint32_t* aliveOut, bool count, hipStream_t stream);
// words k_shade sets to zero for the launches that follow it (each may be null)
struct ShadeResets {
    uint32_t* extendHead;    // work head of the next k_extend
    uint32_t* connectHead;   // work head of this iteration's k_connect
    uint32_t* nextAlive;     // live-slot counter of the next k_extend
    uint32_t drained;        // nonzero once most slots are dead: waves look at the state word alone before loading the rest
};
// env: PTR_METAL_ENV_LOD (device_types.h; all null without the bit)
void launchShade(const RenderParams& rp, const SceneView& sc, const PathPool& pool, const ShadeResets& resets, const EnvLodView& env, bool count,
                 hipStream_t stream);
// the material / feature set of the k_shade instantiation launchShade picks (bsdf.h kAllMaterials = the full kernel)
uint32_t shadeKernelSet(const RenderParams& rp, const SceneView& sc, bool count);
void launchConnect(const RenderParams& rp, const SceneView& sc, const PathPool& pool, const LaunchConfig& cfg, bool count,
                   hipStream_t stream);
// End of the frame: every busy slot of `pool` (the WHOLE pool) is run to the end of its path by one lane (k_tail_collect + k_tail_run).
// dList: pool.slots words; dListCount / dListHead: single words, zero on entry.
void launchTail(const RenderParams& rp, const SceneView& sc, const PathPool& pool, const EnvLodView& env, const LaunchConfig& cfg, uint32_t* dList,
                uint32_t* dListCount, uint32_t* dListHead, bool count, hipStream_t stream);
// Adds outstanding light connections, reduces the slots of each pixel in fixed order and writes
// out[((localBand*PTR_BAND_ROWS + row) * width + x) * 3 + c] = sum / spp.
void launchResolve(const RenderParams& rp, const PathPool& pool, uint32_t partCount, float* dOut, hipStream_t stream);
// The `pixelCount` image pixels dPixels names, whose camera rays cannot reach the scene (csrc/host/background_cull.h): all rp.spp samples
// of the pass, written to dOut as launchResolve writes the traced pixels (same band layout, same pass logic).  rp: the pass's, with
// sampleBase, sppTotal and passFlags set.  Touches no pool.
void launchBackground(const RenderParams& rp, const SceneView& sc, const uint32_t* dPixels, uint32_t pixelCount, uint32_t partCount, float* dOut,
                      hipStream_t stream);
// After launchResolve of the same pass (defined in stats.hip; include/ptr_stats.h): the covariance of every pixel's mean, six floats per
// pixel in the band layout of dOut.  dMean: localPixels float4, the running mean between the passes of a frame; dCov holds the
// unnormalised sums until the last pass.
void launchResolveCov(const RenderParams& rp, const PathPool& pool, uint32_t partCount, float4* dMean, float* dCov, hipStream_t stream);

void launchTraceRays(const SceneView& sc, const float4* dRays, uint64_t n, bool anyHit, PtrHit* dOut, const LaunchConfig& cfg,
                     uint64_t* dCounters, hipStream_t stream);

// First-hit feature buffers for every pixel of the frame (row 0 = top): albedo rgb|hit flag, encoded normal|distance.
void launchAovs(const RenderParams& rp, const SceneView& sc, uint32_t sample, float4* dAlbedo, float4* dNormal, const LaunchConfig& cfg,
                hipStream_t stream);

// The surface records of a temporal step (include/ptr_temporal.h) for every pixel of the frame: dR0, dR1, dR2, and the two buffers of
// launchAovs (sample 0) when dAlbedo / dNormal are not null.  dPrevTris / dPrevSpheres: the rows of the previous pose, laid out like
// sc.tris / sc.spheres (which they may be).
void launchSurface(const RenderParams& rp, const SceneView& sc, const float4* dPrevTris, const float4* dPrevSpheres, float4* dR0, float4* dR1,
                   float4* dR2, float4* dAlbedo, float4* dNormal, const LaunchConfig& cfg, hipStream_t stream);

// ---- tests only: debug / known-answer kernels (ptr_debug.h) ----
// evaluate and sample a material for a batch of inputs
void launchDebugEvalBsdf(const float4* dMaterial, const RenderParams& rp, const float* dIn, uint64_t n, float* dOut,
                         hipStream_t stream);
void launchDebugSampleBsdf(const float4* dMaterial, const RenderParams& rp, const float* dIn, const uint32_t* dFront,
                           const uint32_t* dRng, uint64_t n, float* dOut, uint32_t* dRngOut, hipStream_t stream);
// sample_bsdf's lobe bookkeeping: out n x 3 {lobe, lobe roughness, isDelta} + out[3 n] = the material's environment-lighting roughness;
// dSample n x 8 as launchDebugSampleBsdf
void launchDebugSampleLobes(const float4* dMaterial, const RenderParams& rp, const float* dIn, const uint32_t* dFront, const uint32_t* dRng,
                            uint64_t n, float* dOut, float* dSample, uint32_t* dRngOut, hipStream_t stream);
// PTR_METAL_ENV_LOD lookups: in n x {direction, roughness} -> out n x {LOD, radiance}
void launchDebugEnvLookup(const RenderParams& rp, const SceneView& sc, const EnvLodView& env, const float4* dIn, uint64_t n, float4* dOut,
                          hipStream_t stream);
void launchDebugTexSample(const SceneView& sc, uint32_t texture, const float* dIn, uint64_t n, float4* dOut, hipStream_t stream);
// PTR_METAL_RAY_DIFF: the gradient sample (in n x 6 {u, v, dudx, dvdx, dudy, dvdy}) and the first hit's textured material of the camera rays
// of n {x, y, sample} (out n x 36 floats, ptr_debug.h ptr_debug_first_hit_textures)
void launchDebugTexSampleGrad(const SceneView& sc, uint32_t texture, const float* dIn, uint64_t n, float4* dOut, hipStream_t stream);
void launchDebugFirstHit(const RenderParams& rp, const SceneView& sc, const uint32_t* dXys, uint64_t n, float* dOut, const LaunchConfig& cfg,
                         hipStream_t stream);
// ptr_debug_pbr_hits: applyPbrTextures at the closest hit of n rays with each row's own cone, random state, material and instantiation
// (in n x 20, out n x 32 words)
void launchDebugPbrHits(const SceneView& sc, const float* dIn, uint64_t n, float* dOut, const LaunchConfig& cfg, hipStream_t stream);
// ptr_debug_extend_rays: k_extend's hit words (dHits, n) of the rays dRays (n x 2 float4) as PtrHit records
void launchDebugHitRecords(const SceneView& sc, const float4* dRays, const float2* dHits, uint64_t n, uint32_t triCount, uint32_t sphereCount,
                           PtrHit* dOut, hipStream_t stream);
// closest hit, surface record and next-ray origin per input ray: in n x 9 floats {origin, direction, next direction}, out n x 16 floats
void launchDebugSurfaceHits(const SceneView& sc, const float* dIn, uint64_t n, float* dOut, const LaunchConfig& cfg, hipStream_t stream);
void launchDebugCameraRays(const RenderParams& rp, const uint32_t* dXys, uint64_t n, float* dOut, uint32_t* dRngOut,
                           hipStream_t stream);
// The light side of a path vertex (ptr_debug.h): environment sampling and level-0 lookups (out: 2 n / n float4), rectLightNee at the hits of
// a batch of rays (record 0 of `pool` and dHead receive the result; dMaterial null = the hit's own material), settled connections
void launchDebugEnvSample(const RenderParams& rp, const SceneView& sc, const float* dU, uint64_t n, float4* dOut, hipStream_t stream);
void launchDebugEnvEval(const RenderParams& rp, const SceneView& sc, const float* dDir, uint64_t n, float4* dOut, hipStream_t stream);
void launchDebugRectLightNee(const RenderParams& rp, const SceneView& sc, const PathPool& pool, const float4* dMaterial, const float* dRays,
                             const float* dThr, const uint32_t* dRng, uint64_t n, float4* dHead, uint32_t* dRngOut, const LaunchConfig& cfg,
                             hipStream_t stream);
void launchDebugLightConnection(const RenderParams& rp, const SceneView& sc, const float* dIn, uint64_t n, float* dOut, hipStream_t stream);
// The random-walk subsurface path (ptr_debug_sss.h): sssWalkBegin (in n x 12, out n x 16), sssWalkStep with the step limit as given (in n x
// 20, out n x 24 words), and the first bounce of n camera samples with its whole walk (dSteps n x stepCap x 24, dFinal n x 24 words)
void launchDebugSssBegin(const float4* dMaterial, const RenderParams& rp, const float* dIn, const uint32_t* dRng, uint64_t n, float* dOut,
                         uint32_t* dRngOut, hipStream_t stream);
void launchDebugSssStep(const float4* dMaterial, uint32_t maxSteps, const float* dIn, const uint32_t* dRng, uint64_t n, float* dOut, uint32_t* dRngOut,
                        hipStream_t stream);
// (scratch of the whole walk, per sample: the record of kSssWalkStateWords words, the step probe's row of 20 words, random state and
// material index in, and its 24 words and random state out)
constexpr uint32_t kSssWalkStateWords = 48;
struct SssWalkScratch {
    float* state;
    float* rows;
    uint32_t* rowRng;
    uint32_t* rowMaterial;
    float* stepOut;
    uint32_t* stepRng;
};
void launchDebugSssWalks(const RenderParams& rp, const SceneView& sc, const uint32_t* dXys, uint64_t n, uint32_t stepCap, float* dSteps, float* dFinal,
                         const SssWalkScratch& scratch, const LaunchConfig& cfg, hipStream_t stream);

}  // namespace ptrk
