// A stand-alone check of the host side of include/ptr_appearance.h, meant to be built with sanitizers and run on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -pthread -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host \
//       -Imetal-pathtracer-arm64_amd/csrc/kernels tools/appearance_host_check.cpp metal-pathtracer-arm64_amd/csrc/host/appearance_host.cpp \
//       metal-pathtracer-arm64_amd/csrc/host/scene_geometry.cpp metal-pathtracer-arm64_amd/csrc/host/bvh_builder.cpp \
//       metal-pathtracer-arm64_amd/csrc/host/knobs.cpp -o /tmp/appearance_host_check
//
// For descriptions of 0 to 512 materials and 0 to 128 rectangles (material indices past the table included, which the upload clamps) it
// runs the validation of ptr_scene_set_materials on good and bad lists, the derivation of the rectangle-light table against the
// geometry's own leaf rows, and the shade-key table against the meta words of the geometry's triangles; then the level sizes of mip
// chains, and the index rule every update call's list shares (index_rule.h) with its three message forms.  Prints one line per
// description; exits 1 on the first difference.  No GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "bvh_layout.h"
#include "appearance_host.h"
#include "index_rule.h"

namespace {

struct Scene {
    std::vector<PtrMaterial> materials;
    std::vector<PtrRect> rects;
    std::vector<float> rows;   // the compact rows of the materials: the members the rules read, where compactMaterial puts them
    PtrSceneDesc desc;
};

void fillNoTextures(PtrMaterial& m) {
    for (uint32_t& t : m.textureIndices0) t = ptr::kNoTextureIndex;
    for (uint32_t& t : m.textureIndices1) t = ptr::kNoTextureIndex;
}

void makeScene(uint32_t materials, uint32_t rects, Scene& s) {
    std::mt19937 rng(materials * 2654435761u + rects * 40503u + 7u);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    s.materials.assign(materials, PtrMaterial{});
    s.rows.assign(static_cast<size_t>(materials) * ptr::kCompactMaterialFloats, 0.0f);
    for (uint32_t i = 0; i < materials; ++i) {
        PtrMaterial& m = s.materials[i];
        fillNoTextures(m);
        m.typeEta[0] = static_cast<float>(rng() % 9u);   // type 8 is past the enum: the upload keys it as 7
        if (rng() % 3u) m.emission[0] = 4.0f * std::fabs(uni(rng)), m.emission[1] = 2.0f, m.emission[2] = 1.0f;
        m.sssParams[1] = (rng() & 1u) ? 1.0f : 0.0f;
        float* row = &s.rows[static_cast<size_t>(i) * ptr::kCompactMaterialFloats];
        std::memcpy(row + 4, m.typeEta, 16), std::memcpy(row + 8, m.emission, 16), std::memcpy(row + 60, m.sssParams, 16);
    }
    s.rects.assign(rects, PtrRect{});
    for (uint32_t i = 0; i < rects; ++i) {
        PtrRect& r = s.rects[i];
        const float c[3] = {uni(rng) * 5.0f, uni(rng) * 5.0f, uni(rng) * 5.0f};
        const float u[3] = {1.0f + uni(rng) * 0.5f, uni(rng) * 0.2f, 0.0f}, v[3] = {0.0f, 1.0f + uni(rng) * 0.5f, uni(rng) * 0.2f};
        const float n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), flip = (i & 1u) ? -1.0f : 1.0f;
        for (int a = 0; a < 3; ++a) r.corner[a] = c[a], r.edgeU[a] = u[a], r.edgeV[a] = v[a], r.normalAndPlane[a] = flip * n[a] / len;
        r.materialTwoSided[0] = materials ? rng() % (materials + 2u) : 0u;   // up to two past the table
        r.materialTwoSided[1] = rng() & 1u;
    }
    s.desc = PtrSceneDesc{};
    s.desc.materials = s.materials.data(), s.desc.materialCount = materials;
    s.desc.rects = s.rects.data(), s.desc.rectCount = rects;
}

bool fail(uint32_t materials, uint32_t rects, const char* what) {
    std::printf("%u materials, %u rectangles: %s\n", materials, rects, what);
    return false;
}

bool startsWith(const std::string& s, const char* head) { return s.rfind(head, 0) == 0; }

bool checkValidation(uint32_t materials, uint32_t rects, const Scene& s) {
    auto bad = [&](const char* what) { return fail(materials, rects, what); };
    std::vector<uint32_t> all(materials);
    for (uint32_t i = 0; i < materials; ++i) all[i] = materials - 1u - i;
    if (!startsWith(ptr::MaterialListProblem(nullptr, s.materials.data(), 1, materials, 0), "null material list")) return bad("null indices accepted");
    if (!startsWith(ptr::MaterialListProblem(all.data(), nullptr, 1, materials, 0), "null material list")) return bad("null materials accepted");
    const PtrMaterial none{};
    const uint32_t zero = 0;
    if (ptr::MaterialListProblem(&zero, &none, 0, materials, 0) != "count is 0") return bad("count 0 accepted");
    if (ptr::MaterialListProblem(&materials, &none, 1, materials, 0).find("out of range") == std::string::npos) return bad("index past the table accepted");
    if (materials == 0u) return true;
    std::vector<PtrMaterial> reversed(s.materials.rbegin(), s.materials.rend());
    if (!ptr::MaterialListProblem(all.data(), reversed.data(), materials, materials, 0).empty()) return bad("the whole table refused");
    if (materials >= 2u) {
        std::vector<uint32_t> twice = all;
        twice.back() = twice.front();
        if (ptr::MaterialListProblem(twice.data(), reversed.data(), materials, materials, 0).find("named twice") == std::string::npos) return bad("an index named twice accepted");
    }
    // one non-finite float in each region of the struct, at its first and last member
    const size_t floatsAt[][2] = {{offsetof(PtrMaterial, baseColorRoughness), 68}, {offsetof(PtrMaterial, pbrParams), 8}, {offsetof(PtrMaterial, textureTransform), 48}};
    const float poison[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (const auto& region : floatsAt) {
        for (size_t k : {size_t(0), region[1] - 1u}) {
            for (float p : poison) {
                PtrMaterial m = s.materials[0];
                std::memcpy(reinterpret_cast<char*>(&m) + region[0] + k * 4u, &p, 4);
                if (ptr::MaterialListProblem(&zero, &m, 1, materials, 0).find("non-finite") == std::string::npos) return bad("a non-finite float accepted");
            }
        }
    }
    // texture indices: none on a scene without textures, below the count on one with
    for (int slot = 0; slot < 6; ++slot) {
        PtrMaterial m = s.materials[0];
        (slot < 4 ? m.textureIndices0[slot] : m.textureIndices1[slot - 4]) = 2u;
        if (ptr::MaterialListProblem(&zero, &m, 1, materials, 0).find("without textures") == std::string::npos) return bad("a texture on an untextured scene accepted");
        if (ptr::MaterialListProblem(&zero, &m, 1, materials, 2).find("names texture 2") == std::string::npos) return bad("a texture past the count accepted");
        if (!ptr::MaterialListProblem(&zero, &m, 1, materials, 3).empty()) return bad("a texture below the count refused");
    }
    return true;
}

bool checkTables(uint32_t materials, uint32_t rects, const Scene& s) {
    auto bad = [&](const char* what) { return fail(materials, rects, what); };
    ptr::SceneGeometry geo;
    std::string error;
    if (!ptr::BuildSceneGeometry(s.desc, 0, geo, error, nullptr)) return bad(error.c_str());
    // the key table against the meta word of every triangle the geometry wrote
    std::vector<uint8_t> keys;
    ptr::BuildShadeKeyTable(s.rows.data(), materials, keys);
    if (keys.size() != materials) return bad("key table size");
    for (uint32_t t = 0; t < geo.triCount; ++t) {
        uint32_t material, meta;
        std::memcpy(&material, &geo.triData[static_cast<size_t>(t) * 12u + 3u], 4), std::memcpy(&meta, &geo.triData[static_cast<size_t>(t) * 12u + 7u], 4);
        const uint32_t want = materials ? keys[std::min(material, materials - 1u)] : 0u;
        if (((meta >> ptrk::kHitKeyShift) & ptrk::kHitKeyMask) != want) return bad("a triangle's key is not the table's");
    }
    uint32_t mask = 0, wantMask = 0;
    bool walk = false, wantWalk = false;
    ptr::MaterialTableFacts(s.rows.data(), materials, mask, walk);
    for (const PtrMaterial& m : s.materials) {
        const uint32_t type = static_cast<uint32_t>(m.typeEta[0]);
        wantMask |= 1u << std::min(type, 7u);
        wantWalk = wantWalk || (type == PTR_MAT_SUBSURFACE && m.sssParams[1] >= 0.5f);
    }
    if (mask != wantMask || walk != wantWalk) return bad("type mask or random-walk flag");
    // the light table against the upload's rule, with the light's own triangles taken from the geometry's leaf rows
    const ptr::RectLightTable got = ptr::DeriveRectLights(s.rects.data(), rects, geo.rectTriLeaf.data(), s.rows.data(), materials);
    if (got.lightIndexByRect.size() != rects || got.rectEmission.size() != static_cast<size_t>(rects) * 3u || got.rectShadeKey.size() != rects) return bad("light table sizes");
    std::vector<float> want;
    uint32_t count = 0;
    for (uint32_t i = 0; i < rects && materials > 0u; ++i) {
        const PtrMaterial& m = s.materials[std::min(s.rects[i].materialTwoSided[0], materials - 1u)];
        const bool light = static_cast<uint32_t>(m.typeEta[0]) == PTR_MAT_DIFFUSE_LIGHT && (m.emission[0] * m.emission[0] + m.emission[1] * m.emission[1]) + m.emission[2] * m.emission[2] > 0.0f;
        if ((got.lightIndexByRect[i] >= 0) != light) return bad("which rectangles are lights");
        if (!light) continue;
        if (got.lightIndexByRect[i] != static_cast<int32_t>(count++)) return bad("light order");
        const uint32_t t0 = geo.rectTriLeaf[static_cast<size_t>(i) * 2u], t1 = geo.rectTriLeaf[static_cast<size_t>(i) * 2u + 1u];
        const bool have = t0 != 0xFFFFFFFFu && t1 != 0xFFFFFFFFu;
        float row[ptr::kRectLightFloats];
        ptr::WriteRectLightRow(s.rects[i], i, m.emission, have ? &geo.triData[static_cast<size_t>(t0) * 12u] : nullptr, have ? &geo.triData[static_cast<size_t>(t1) * 12u] : nullptr, row);
        want.insert(want.end(), row, row + ptr::kRectLightFloats);
        if (std::memcmp(&got.rectEmission[static_cast<size_t>(i) * 3u], m.emission, 12) != 0) return bad("a light's emission record");
    }
    if (got.lightCount != count || got.lights.size() != want.size()) return bad("light count");
    if (!want.empty() && std::memcmp(got.lights.data(), want.data(), want.size() * 4u) != 0) return bad("light rows differ from the geometry's");
    return true;
}

bool checkMips() {
    const uint32_t sizes[][3] = {{1, 1, 1}, {1, 7, 3}, {5, 3, 3}, {8, 8, 4}, {16, 2, 5}, {7, 16, 5}, {65536, 1, 16}, {65536, 65536, 16}, {4096, 2048, 13}};
    for (const auto& s : sizes) {
        std::vector<ptr::MipLevel> levels;
        ptr::MipChainLevels(s[0], s[1], levels);
        if (levels.size() != s[2] || levels[0].width != s[0] || levels[0].height != s[1]) return false;
        for (size_t l = 1; l < levels.size(); ++l) {
            if (levels[l].width != std::max(levels[l - 1].width / 2u, 1u) || levels[l].height != std::max(levels[l - 1].height / 2u, 1u)) return false;
        }
    }
    std::vector<float> cell;
    ptr::EnvCellWeights(3, 5, cell);
    return cell.size() == 5u && cell[0] > 0.0f && cell[4] > 0.0f && cell[2] > cell[1] && cell[2] > cell[3];
}

// the index rule on scenes of 0, 1 and 300 entities, for two kinds whose plurals differ: the three message forms, literally
bool checkIndexRule() {
    const char* const kinds[2][2] = {{"mesh", "meshes"}, {"texture", "textures"}};
    for (const auto& k : kinds) {
        const std::string kind = k[0], plural = k[1];
        for (uint32_t count : {0u, 1u, 300u}) {
            std::vector<uint8_t> named(count, 0);
            const std::string past = kind + " index " + std::to_string(count) + " out of range (the scene has " + std::to_string(count) + " " + plural + ")";
            if (ptr::NamedIndexProblem(k[0], k[1], count, named) != past) return false;   // the first index past the table; any index of an empty scene
            if (ptr::NamedIndexProblem(k[0], k[1], 0xFFFFFFFFu, named) != kind + " index 4294967295 out of range (the scene has " + std::to_string(count) + " " + plural + ")") return false;
            for (uint8_t byte : named) {
                if (byte) return false;   // a refused index marks nothing
            }
            if (count == 0u) continue;
            const uint32_t last = count - 1u;
            if (!ptr::NamedIndexProblem(k[0], k[1], last, named).empty() || !named[last]) return false;   // the last valid index
            if (ptr::NamedIndexProblem(k[0], k[1], last, named) != kind + " index " + std::to_string(last) + " named twice") return false;
            if (ptr::NamedIndexProblem(k[0], k[1], last, named) != kind + " index " + std::to_string(last) + " named twice") return false;   // and a third time
            if (count > 1u && (!ptr::NamedIndexProblem(k[0], k[1], 0u, named).empty() || ptr::NamedIndexProblem(k[0], k[1], 0u, named) != kind + " index 0 named twice")) return false;
        }
    }
    std::vector<uint8_t> named(3, 0);
    return ptr::NamedIndexProblem("rectangle", "rectangles", 3u, named) == "rectangle index 3 out of range (the scene has 3 rectangles)" &&
           ptr::NamedIndexProblem("mesh", "meshes", 7u, named) == "mesh index 7 out of range (the scene has 3 meshes)" &&
           ptr::NamedIndexProblem("mesh", "meshes", 2u, named).empty() && ptr::NamedIndexProblem("mesh", "meshes", 2u, named) == "mesh index 2 named twice";
}

}  // namespace

int main() {
    const uint32_t materialCounts[] = {0u, 1u, 2u, 9u, 255u, 512u}, rectCounts[] = {0u, 1u, 2u, 9u, 128u};
    for (uint32_t materials : materialCounts) {
        for (uint32_t rects : rectCounts) {
            Scene s;
            makeScene(materials, rects, s);
            if (!checkValidation(materials, rects, s) || !checkTables(materials, rects, s)) return 1;
            std::printf("%u materials, %u rectangles: ok\n", materials, rects);
        }
    }
    if (!checkMips()) {
        std::printf("mip levels and cell weights: differ\n");
        return 1;
    }
    if (!checkIndexRule()) {
        std::printf("the index rule: differs\n");
        return 1;
    }
    std::printf("mip levels and cell weights: ok\n");
    return 0;
}
