// The host half of include/ptr_appearance.h that needs no device: what the calls refuse about their lists, the facts the upload derives
// from materials (type mask, random-walk flag, shade keys), the rectangle-light table of a set of rectangles under a material table, and
// the level sizes of a mip chain.  Plain C++ (g++), so tools/appearance_host_check.cpp runs it under sanitizers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "ptr_abi.h"
#include "scene_geometry.h"

namespace ptr {

constexpr uint32_t kCompactMaterialFloats = 64u;   // kernels/device_types.h kMaterialVec4 float4: the rows compactMaterial writes
constexpr uint32_t kNoTextureIndex = 0xFFFFFFFFu;

// What ptr_scene_set_materials refuses about its list on a scene of `materialCount` materials and `textureCount` textures (0: uploaded
// without textures), or "".
std::string MaterialListProblem(const uint32_t* indices, const PtrMaterial* materials, uint32_t count, uint32_t materialCount, uint32_t textureCount);

// Of one compact material row (kCompactMaterialFloats floats): the type as the upload reads it, its shade key (kernels/bvh_layout.h:
// type + 1, types above 7 as 7), whether it is a random-walk subsurface material.
uint32_t CompactMaterialType(const float* row);
inline uint32_t ShadeKeyOfType(uint32_t type) { return (type < 7u ? type : 7u) + 1u; }
bool CompactMaterialRandomWalk(const float* row);
// SceneView::materialTypes and the random-walk flag of a whole table of compact rows
void MaterialTableFacts(const float* rows, uint32_t materialCount, uint32_t& typeMask, bool& randomWalk);
// one byte per material: its shade key (k_app_rekey's table)
void BuildShadeKeyTable(const float* rows, uint32_t materialCount, std::vector<uint8_t>& keys);

// The rectangle-light table, for the upload (prepareScene) and for ptr_scene_set_materials alike: DiffuseLight rectangles with non-zero
// emission, from the rectangles' records, the leaf places of their triangles (2 per rectangle, 0xFFFFFFFF: not in the geometry) and the
// compact material rows (a material index past the table reads its last row).  A light's own two triangle rows are written as the
// geometry writes them (WriteRectTriangles under the shade key of the rectangle's material), so they are the leaf-order records.
struct RectLightTable {
    std::vector<float> lights;               // kRectLightFloats per light
    std::vector<int32_t> lightIndexByRect;   // -1: no light
    std::vector<float> rectEmission;         // 3 per rectangle (zeros for one that is no light)
    std::vector<uint32_t> rectShadeKey;      // per rectangle
    uint32_t lightCount = 0;
    bool lightsHaveTriangles = true;
};
RectLightTable DeriveRectLights(const PtrRect* rects, uint32_t rectCount, const uint32_t* rectTriLeaf, const float* materialRows, uint32_t materialCount);

// The sizes of the levels of a mip chain over a width x height image, level 0 first: each size halves down to at least 1, at most 16 levels.
struct MipLevel {
    uint32_t width, height;
};
void MipChainLevels(uint32_t width, uint32_t height, std::vector<MipLevel>& levels);

// the per-row cell weights of an environment map (BuildEnvImportanceDistribution's cell[y]), which depend on the size alone
void EnvCellWeights(uint32_t width, uint32_t height, std::vector<float>& cell);

}  // namespace ptr
