#include "appearance_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "index_rule.h"

namespace ptr {
namespace {

constexpr uint32_t kRowTypeEta = 1u, kRowEmission = 2u, kRowSssParams = 15u;   // kernels/device_types.h MaterialSlot

bool allFinite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(p[i])) return false;
    }
    return true;
}

// every float member of a PtrMaterial: the 17 rows ahead of the texture indices, then pbrParams .. pbrExtras, then the transforms
bool materialFinite(const PtrMaterial& m) {
    return allFinite(m.baseColorRoughness, 17u * 4u) && allFinite(m.pbrParams, 4u) && allFinite(m.pbrExtras, 4u) && allFinite(&m.textureTransform[0][0], 48u);
}

}  // namespace

std::string MaterialListProblem(const uint32_t* indices, const PtrMaterial* materials, uint32_t count, uint32_t materialCount, uint32_t textureCount) {
    if (!indices || !materials) return "null material list";
    if (count == 0u) return "count is 0";
    std::vector<uint8_t> named(materialCount, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t index = indices[i];
        const std::string bad = NamedIndexProblem("material", "materials", index, named);
        if (!bad.empty()) return bad;
        const PtrMaterial& m = materials[i];
        const std::string name = "material " + std::to_string(index);
        if (!materialFinite(m)) return name + " has a non-finite entry";
        const uint32_t slots[6] = {m.textureIndices0[0], m.textureIndices0[1], m.textureIndices0[2], m.textureIndices0[3], m.textureIndices1[0], m.textureIndices1[1]};
        for (uint32_t s : slots) {
            if (s == kNoTextureIndex) continue;
            if (textureCount == 0u) return name + " names texture " + std::to_string(s) + " and the scene was uploaded without textures";
            if (s >= textureCount) return name + " names texture " + std::to_string(s) + " (the scene has " + std::to_string(textureCount) + " textures)";
        }
    }
    return "";
}

uint32_t CompactMaterialType(const float* row) { return static_cast<uint32_t>(row[kRowTypeEta * 4u]); }

bool CompactMaterialRandomWalk(const float* row) { return CompactMaterialType(row) == PTR_MAT_SUBSURFACE && row[kRowSssParams * 4u + 1u] >= 0.5f; }

void MaterialTableFacts(const float* rows, uint32_t materialCount, uint32_t& typeMask, bool& randomWalk) {
    typeMask = 0u, randomWalk = false;
    for (uint32_t i = 0; i < materialCount; ++i) {
        const float* row = rows + static_cast<size_t>(i) * kCompactMaterialFloats;
        typeMask |= 1u << std::min(CompactMaterialType(row), 7u);
        randomWalk = randomWalk || CompactMaterialRandomWalk(row);
    }
}

void BuildShadeKeyTable(const float* rows, uint32_t materialCount, std::vector<uint8_t>& keys) {
    keys.resize(materialCount);
    for (uint32_t i = 0; i < materialCount; ++i) keys[i] = static_cast<uint8_t>(ShadeKeyOfType(CompactMaterialType(rows + static_cast<size_t>(i) * kCompactMaterialFloats)));
}

RectLightTable DeriveRectLights(const PtrRect* rects, uint32_t rectCount, const uint32_t* rectTriLeaf, const float* materialRows, uint32_t materialCount) {
    RectLightTable out;
    out.lightIndexByRect.assign(rectCount, -1);
    out.rectEmission.assign(static_cast<size_t>(rectCount) * 3u, 0.0f);
    out.rectShadeKey.assign(rectCount, 0u);
    if (rectCount == 0u || materialCount == 0u) return out;
    for (uint32_t i = 0; i < rectCount; ++i) {
        const PtrRect& r = rects[i];
        const float* m = materialRows + static_cast<size_t>(std::min(r.materialTwoSided[0], materialCount - 1u)) * kCompactMaterialFloats;
        const uint32_t type = CompactMaterialType(m);
        out.rectShadeKey[i] = ShadeKeyOfType(type);
        if (type != PTR_MAT_DIFFUSE_LIGHT) continue;
        const float* e = m + kRowEmission * 4u;
        if (!((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > 0.0f)) continue;
        const uint32_t t0 = rectTriLeaf[static_cast<size_t>(i) * 2u], t1 = rectTriLeaf[static_cast<size_t>(i) * 2u + 1u];
        const bool haveTris = t0 != 0xFFFFFFFFu && t1 != 0xFFFFFFFFu;
        out.lightsHaveTriangles = out.lightsHaveTriangles && haveTris;
        float tri[2][12], nrm[2][12];
        BuildPrim half[2];
        WriteRectTriangles(r, i, out.rectShadeKey[i], tri, nrm, half);
        float row[kRectLightFloats];
        WriteRectLightRow(r, i, e, haveTris ? tri[0] : nullptr, haveTris ? tri[1] : nullptr, row);
        out.lights.insert(out.lights.end(), row, row + kRectLightFloats);
        std::memcpy(&out.rectEmission[static_cast<size_t>(i) * 3u], e, 12);
        out.lightIndexByRect[i] = static_cast<int32_t>(out.lightCount++);
    }
    return out;
}

void MipChainLevels(uint32_t width, uint32_t height, std::vector<MipLevel>& levels) {
    levels.clear();
    uint32_t w = width, h = height;
    levels.push_back(MipLevel{w, h});
    while ((w > 1u || h > 1u) && levels.size() < 16u) {
        w = std::max(w / 2u, 1u), h = std::max(h / 2u, 1u);
        levels.push_back(MipLevel{w, h});
    }
}

void EnvCellWeights(uint32_t width, uint32_t height, std::vector<float>& cell) {
    constexpr float kPi = 3.14159265358979323846f;
    const float dTheta = kPi / static_cast<float>(height);
    const float dPhi = (2.0f * kPi) / static_cast<float>(width);
    cell.resize(height);
    for (uint32_t y = 0; y < height; ++y) cell[y] = std::max(std::sin((static_cast<float>(y) + 0.5f) * dTheta), 0.0f) * dTheta * dPhi;
}

}  // namespace ptr
