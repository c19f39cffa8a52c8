// Launchers of the appearance kernels (appearance.hip; include/ptr_appearance.h): the shade keys of the triangle rows after a material
// changed type, the mip chain of a texture or of the environment map level by level, and the environment map's importance tables.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptrk {

// Most entries of one alias table (a row of the map, or its column of row sums): scaled values and two work lists, 12 B each, in LDS.
constexpr uint32_t kAppAliasMaxEntries = 4096u;

// Every triangle row (3 float4 each) takes the key of its material (dKeys: one byte per material, the row's index clamped to the table
// as the upload clamps it) into the key field of its meta word, written only where it differs; *dChanged counts the rows written.
// A row whose key field is 0 was never keyed (every material has a key of at least 1) and is left alone: the object-space corner rows of
// a dynamic scene carry the same w words for the bake to copy, and zeros where a rectangle's halves are.
void launchAppRekey(float4* dTris, uint32_t triCount, const uint8_t* dKeys, uint32_t materialCount, uint32_t* dChanged, hipStream_t stream);

// Level l + 1 (nw x nh, at dDst) of a mip chain from level l (w x h, at dSrc): ((a + b) + (c + d)) * 0.25f, the second tap clamped.
void launchAppMipLevel(const float4* dSrc, float4* dDst, uint32_t w, uint32_t h, uint32_t nw, uint32_t nh, hipStream_t stream);

// Environment tables.  dCell: the per-row cell weights (host-computed).
// weight[y][x] = max(luminance, 0) * cell[y]; rowWeight[y] = their sum left to right
void launchAppEnvWeights(const float4* dRgba, const float* dCell, uint32_t width, uint32_t height, float* dWeight, float* dRowWeight, hipStream_t stream);
// *dTotal = the running float sum of weight[0 .. count) in order
void launchAppEnvTotal(const float* dWeight, uint64_t count, float* dTotal, hipStream_t stream);
// the conditional table of every row and the marginal table (Vose's method as ptr::BuildEnvImportanceDistribution runs it)
void launchAppEnvAlias(const float* dWeight, const float* dRowWeight, const float* dTotal, uint32_t width, uint32_t height, float2* dCond, float2* dMarg,
                       hipStream_t stream);
void launchAppEnvPdf(const float* dWeight, const float* dCell, const float* dTotal, uint32_t width, uint32_t height, float* dPdf, hipStream_t stream);

}  // namespace ptrk
