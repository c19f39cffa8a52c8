// Appearance updates of a resident scene (include/ptr_appearance.h): ptr_scene_set_materials, ptr_scene_set_textures and
// ptr_scene_set_environment with their device-pointer forms, and the header's test-only probe.  Every call is a check half (its rules, on
// the host, against the records uploadScene filled: fillAppearanceRecords) and a run half (the device work on one scene and one stream,
// the records following once it is joined), declared in dynamic_host.h beside the geometry calls' halves.  The rules that need no device
// are in appearance_host.cpp (plain C++); the kernels are in kernels/appearance.hip.  Compiled with hipcc (host code only), like
// dynamic.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "../kernels/appearance.h"
#include "../kernels/dynamic.h"
#include "appearance_host.h"
#include "device_scene.h"
#include "dynamic_host.h"
#include "ptr_appearance.h"
#include "ptr_deform.h"

using namespace ptrk;
using namespace ptrhost;

namespace {

using Clock = UpdateClock;
constexpr uint32_t kTexInfoWords = 20u;   // kernels/texture.h: width, height, levels, wrap / filter, then the 16 level offsets
constexpr uint32_t kRowFloats = ptr::kCompactMaterialFloats;
static_assert(kRowFloats == kMaterialVec4 * 4u && kRowFloats == kMaterialTexVec4 * 4u, "material row layouts");
static_assert(PTR_APPEARANCE_ENV_MAX_DIM == kAppAliasMaxEntries, "the header's bound is the kernel's");

double msSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// The scratch of the runs, made at the first call that needs it (the scene's device is current)
AppearanceState& stateOf(PtrDeviceScene& ds) {
    if (ds.appearance) return *ds.appearance;
    auto st = std::make_unique<AppearanceState>();
    for (hipEvent_t& e : st->events) HIP_CHECK(hipEventCreate(&e));
    st->words.ensure(64);
    ds.appearance = std::move(st);
    return *ds.appearance;
}

// what every run ends with: the figures of the call that began at `began`, `steps` of them between the state's events
void report(AppearanceState& st, const SceneView& v, Clock::time_point began, double stagingMs, int steps, uint32_t lightsBefore, uint64_t rowsRekeyed,
            uint64_t texelsWritten, PtrAppearanceInfo* out) {
    if (!out) return;
    PtrAppearanceInfo info{};
    info.stagingMs = stagingMs;
    for (int g = 0; g < steps; ++g) {
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, st.events[g], st.events[g + 1]));
        info.kernelMs[g] = ms;
    }
    info.rowsRekeyed = rowsRekeyed, info.texelsWritten = texelsWritten;
    info.lightsBefore = lightsBefore, info.lightsAfter = v.rectLightCount;
    info.envSampling = v.envSampling;
    info.totalSeconds = std::chrono::duration<double>(Clock::now() - began).count();
    *out = info;
}

// firstNonFinite (dynamic_host.h) over `n` of the caller's device arrays with the state's scratch: rows(r) is row r.  pinned: checkBytes(n)
// of the run's pinned block, 16 B aligned, behind whatever else the run keeps there.
size_t checkBytes(size_t n) { return n * sizeof(DynCheckRow) + ((n + 31u) / 32u) * sizeof(uint32_t) + 16u; }
template <typename RowOf>
int firstNonFiniteOf(AppearanceState& st, char* pinned, size_t n, RowOf&& rowOf, hipStream_t stream) {
    st.checkRows.ensure(n);
    st.words.ensure(1u + (n + 31u) / 32u);
    DynCheckRow* rows = reinterpret_cast<DynCheckRow*>(pinned);
    for (size_t r = 0; r < n; ++r) rows[r] = rowOf(r);
    return firstNonFinite(rows, n, reinterpret_cast<DynCheckRow*>(st.checkRows.ptr), st.words.ptr + 1, reinterpret_cast<uint32_t*>(rows + n), stream);
}

// levels 1 .. of a chain whose level 0 is at `level0` and whose level l >= 1 is at base + offsets[l]; returns the texels written
uint64_t writeMipChain(const float4* level0, float4* base, const std::vector<uint64_t>& offsets, const std::vector<ptr::MipLevel>& levels, hipStream_t stream) {
    uint64_t written = 0;
    for (size_t l = 1; l < levels.size(); ++l) {
        const float4* src = l == 1u ? level0 : base + offsets[l - 1u];
        launchAppMipLevel(src, base + offsets[l], levels[l - 1u].width, levels[l - 1u].height, levels[l].width, levels[l].height, stream);
        written += static_cast<uint64_t>(levels[l].width) * levels[l].height;
    }
    return written;
}

}  // namespace

namespace ptrhost {

void fillAppearanceRecords(const PtrSceneDesc& desc, const PreparedScene& ps, AppearanceRecords& rec) {
    rec.materialRows = ps.mats;
    rec.rectMaterial.resize(desc.rectCount);
    for (uint32_t i = 0; i < desc.rectCount; ++i) rec.rectMaterial[i] = desc.rects[i].materialTwoSided[0];
    rec.texInfo = ps.texInfo;
}

// ---------------------------------------------------------------------------------------------------------------- materials
std::string checkMaterials(const PtrDeviceScene* scene, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, MaterialsUpdate& out) {
    out.began = Clock::now();
    const SceneView& v = scene->view;
    const AppearanceRecords& rec = scene->appearanceRecords;
    const uint32_t materialCount = v.materialCount;
    const std::string problem = ptr::MaterialListProblem(indices, materials, count, materialCount, v.textureCount);
    if (!problem.empty()) return problem;
    const bool keepsPrimitives = scene->dynamic && (scene->dynamic->flags & PTR_DYNAMIC_PRIMITIVES);
    std::vector<uint8_t> named(materialCount, 0);
    for (uint32_t i = 0; i < count; ++i) named[indices[i]] = 1;
    for (uint32_t r = 0; r < v.rectCount && !out.touchesRects; ++r) out.touchesRects = named[std::min(rec.rectMaterial[r], materialCount - 1u)] != 0;
    if (out.touchesRects && !keepsPrimitives) {
        return "a rectangle uses a named material and the scene does not keep its rectangles (upload it with ptr_scene_upload_dynamic_ex and "
               "PTR_DYNAMIC_PRIMITIVES)";
    }
    // the new rows: compact rows, texture rows, and what follows from the table with them in it
    const bool textured = v.textureCount > 0u;
    out.index.assign(indices, indices + count);
    out.rows.reserve(static_cast<size_t>(count) * kRowFloats);
    out.texRows.resize(textured ? static_cast<size_t>(count) * kRowFloats : 0u);
    for (uint32_t i = 0; i < count; ++i) {
        compactMaterial(materials[i], out.rows);
        if (textured) materialTexRow(materials[i], &out.texRows[static_cast<size_t>(i) * kRowFloats]);
    }
    std::vector<float> next = rec.materialRows;
    for (uint32_t i = 0; i < count; ++i) {
        float* dst = &next[static_cast<size_t>(indices[i]) * kRowFloats];
        const float* src = &out.rows[static_cast<size_t>(i) * kRowFloats];
        out.keyChanged = out.keyChanged || ptr::ShadeKeyOfType(ptr::CompactMaterialType(dst)) != ptr::ShadeKeyOfType(ptr::CompactMaterialType(src));
        std::memcpy(dst, src, kRowFloats * sizeof(float));
    }
    ptr::MaterialTableFacts(next.data(), materialCount, out.typeMask, out.randomWalk);
    if (out.touchesRects) {
        const PrimitiveRecords& prims = scene->dynamic->prims;
        out.lights = ptr::DeriveRectLights(prims.rects.data(), static_cast<uint32_t>(prims.rects.size()), prims.rectTriLeaf.data(), next.data(), materialCount);
    }
    if (out.keyChanged) ptr::BuildShadeKeyTable(next.data(), materialCount, out.keys);
    return "";
}

void runMaterials(PtrDeviceScene& ds, const MaterialsUpdate& u, hipStream_t stream, PtrAppearanceInfo* infoOut) {
    AppearanceState& st = stateOf(ds);
    SceneView& v = ds.view;
    const ptr::RectLightTable& lights = u.lights;
    const uint32_t count = static_cast<uint32_t>(u.index.size());
    // one pinned block: rows | texture rows | light rows | lightIndexByRect | keys | the counter's landing place
    const size_t rowBytes = u.rows.size() * 4u, texBytes = u.texRows.size() * 4u, lightBytes = lights.lights.size() * 4u;
    const size_t indexBytes = lights.lightIndexByRect.size() * 4u, keyBytes = (u.keys.size() + 15u) & ~size_t(15);
    char* pinned = static_cast<char*>(st.pinned.pinnedFor(rowBytes + texBytes + lightBytes + indexBytes + keyBytes + 16u));
    char* pTex = pinned + rowBytes;
    char* pLights = pTex + texBytes;
    char* pIndex = pLights + lightBytes;
    char* pKeys = pIndex + indexBytes;
    uint32_t* pChanged = reinterpret_cast<uint32_t*>(pKeys + keyBytes);
    std::memcpy(pinned, u.rows.data(), rowBytes);
    if (texBytes) std::memcpy(pTex, u.texRows.data(), texBytes);
    if (lightBytes) std::memcpy(pLights, lights.lights.data(), lightBytes);
    if (indexBytes) std::memcpy(pIndex, lights.lightIndexByRect.data(), indexBytes);
    if (!u.keys.empty()) std::memcpy(pKeys, u.keys.data(), u.keys.size());
    *pChanged = 0u;
    if (u.touchesRects) {
        ds.rectLights.ensure(lights.lights.size() / 4u);   // (a table that grows moves; every row of it is written below)
        v.rectLights = ds.rectLights.ptr;
    }
    if (u.keyChanged) st.keys.ensure(u.keys.size());
    const double stagingMs = msSince(u.began);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    for (uint32_t i = 0; i < count; ++i) {
        const size_t at = static_cast<size_t>(u.index[i]) * kMaterialVec4;
        HIP_CHECK(hipMemcpyAsync(ds.materials.ptr + at, pinned + static_cast<size_t>(i) * kRowFloats * 4u, kRowFloats * 4u, hipMemcpyHostToDevice, stream));
        if (texBytes) HIP_CHECK(hipMemcpyAsync(ds.materialTex.ptr + at, pTex + static_cast<size_t>(i) * kRowFloats * 4u, kRowFloats * 4u, hipMemcpyHostToDevice, stream));
    }
    if (u.touchesRects) {
        if (lightBytes) HIP_CHECK(hipMemcpyAsync(ds.rectLights.ptr, pLights, lightBytes, hipMemcpyHostToDevice, stream));
        if (indexBytes) HIP_CHECK(hipMemcpyAsync(ds.lightIndexByRect.ptr, pIndex, indexBytes, hipMemcpyHostToDevice, stream));
    }
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    if (u.keyChanged) {
        HIP_CHECK(hipMemcpyAsync(st.keys.ptr, pKeys, u.keys.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(st.words.ptr, 0, sizeof(uint32_t), stream));
        launchAppRekey(ds.tris.ptr, static_cast<uint32_t>(ds.info[2]), st.keys.ptr, v.materialCount, st.words.ptr, stream);
        HIP_CHECK(hipMemcpyAsync(pChanged, st.words.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        // a dynamic scene bakes the w words of its triangle rows out of the object-space corner rows: they follow (counted apart)
        if (ds.dynamic) launchAppRekey(ds.dynamic->objPos.ptr, ds.dynamic->triCount, st.keys.ptr, v.materialCount, st.words.ptr + 1, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    HIP_CHECK(hipStreamSynchronize(stream));

    // the host's records follow
    const uint32_t lightsBefore = v.rectLightCount;
    for (uint32_t i = 0; i < count; ++i) {
        std::memcpy(&ds.appearanceRecords.materialRows[static_cast<size_t>(u.index[i]) * kRowFloats], &u.rows[static_cast<size_t>(i) * kRowFloats], kRowFloats * 4u);
    }
    v.materialTypes = u.typeMask;
    ds.hasRandomWalkMaterial = u.randomWalk;
    if (u.touchesRects) {
        PrimitiveRecords& prims = ds.dynamic->prims;
        v.rectLightCount = lights.lightCount;
        v.settleRectLights = (lights.lightCount > 0u && lights.lightCount <= kSettleLightsMax && lights.lightsHaveTriangles) ? 1u : 0u;
        ds.info[7] = lights.lightCount;
        prims.lightIndexByRect = lights.lightIndexByRect;
        prims.rectEmission = lights.rectEmission;
        prims.rectShadeKey = lights.rectShadeKey;
    }
    report(st, v, u.began, stagingMs, 2, lightsBefore, *pChanged, 0u, infoOut);
}

// ---------------------------------------------------------------------------------------------------------------- textures
std::string checkTextures(const PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, int arraysDevice,
                          TexturesUpdate& out) {
    out.began = Clock::now();
    const uint32_t textureCount = scene->view.textureCount;
    if (textureCount == 0u) return "the scene has no textures";
    const std::string bad = listProblem(textures, count, "null texture list");
    if (!bad.empty()) return bad;
    const std::vector<uint32_t>& texInfo = scene->appearanceRecords.texInfo;
    out.fromDevice = fromDevice;
    out.entry.resize(count);
    out.records.resize(static_cast<size_t>(count) * kTexInfoWords);
    std::vector<uint8_t> named(textureCount, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const PtrTextureUpdate& t = textures[i];
        const std::string problem = ptr::NamedIndexProblem("texture", "textures", t.textureIndex, named);
        if (!problem.empty()) return problem;
        const std::string name = "texture " + std::to_string(t.textureIndex);
        if (!t.rgba) return name + " has null pixels";
        const uint32_t* rec = &texInfo[static_cast<size_t>(t.textureIndex) * kTexInfoWords];
        if (t.width != rec[0] || t.height != rec[1]) {
            return name + " was uploaded at " + std::to_string(rec[0]) + " x " + std::to_string(rec[1]) + ", not " + std::to_string(t.width) + " x " +
                   std::to_string(t.height);
        }
        const size_t n = static_cast<size_t>(t.width) * t.height * 4u;
        if (fromDevice) {
            const std::string pointer = devicePointerProblem(t.rgba, n * sizeof(float), arraysDevice);
            if (!pointer.empty()) return "the pixel array of " + name + " " + pointer;
        }
        out.entry[i] = TexturesUpdate::Entry{t.textureIndex, t.rgba, n};
        if (!fromDevice) out.floats += n;
        // the record as it is, but for the word wrap and filter share
        uint32_t* next = &out.records[static_cast<size_t>(i) * kTexInfoWords];
        std::memcpy(next, rec, kTexInfoWords * 4u);
        next[3] = (t.wrapS & 3u) | ((t.wrapT & 3u) << 2) | ((t.filter ? 1u : 0u) << 4);
    }
    return "";
}

std::string stageTextures(const TexturesUpdate& u, float* pinned) {
    for (const TexturesUpdate::Entry& e : u.entry) {
        if (!stageFinite(e.rgba, e.floats, pinned)) return "texture " + std::to_string(e.texture) + " has a non-finite component";
        pinned += e.floats;
    }
    return "";
}

void runTextures(const char* who, PtrDeviceScene& ds, const TexturesUpdate& u, const float* staged, bool checkGiven, hipStream_t stream,
                 PtrAppearanceInfo* infoOut, const InputsEnqueued& enqueued) {
    AppearanceState& st = stateOf(ds);
    const size_t count = u.entry.size();
    // one pinned block: the records, then the rows and the flag words of the device form's check
    const size_t recordBytes = u.records.size() * 4u;
    char* pinned = static_cast<char*>(st.pinned.pinnedFor(recordBytes + checkBytes(count)));
    uint32_t* records = reinterpret_cast<uint32_t*>(pinned);
    std::memcpy(records, u.records.data(), recordBytes);
    const double stagingMs = msSince(u.began);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    if (u.fromDevice && checkGiven) {
        const int bad = firstNonFiniteOf(st, pinned + recordBytes, count, [&](size_t r) { return DynCheckRow{u.entry[r].rgba, u.entry[r].floats}; }, stream);
        if (bad >= 0) throw Refused{std::string(who) + ": texture " + std::to_string(u.entry[bad].texture) + " has a non-finite component"};
    }
    float4* texels = ds.texels.ptr;
    uint64_t written = 0;
    for (size_t i = 0; i < count; ++i) {
        const TexturesUpdate::Entry& e = u.entry[i];
        const uint32_t* rec = records + i * kTexInfoWords;
        HIP_CHECK(hipMemcpyAsync(texels + rec[4], u.fromDevice ? e.rgba : staged, e.floats * sizeof(float), u.fromDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(reinterpret_cast<uint32_t*>(ds.texInfo.ptr) + static_cast<size_t>(e.texture) * kTexInfoWords, rec, kTexInfoWords * 4u,
                                 hipMemcpyHostToDevice, stream));
        if (!u.fromDevice) staged += e.floats;
        written += e.floats / 4u;
    }
    if (enqueued) enqueued();
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    for (size_t i = 0; i < count; ++i) {
        const uint32_t* rec = records + i * kTexInfoWords;
        std::vector<ptr::MipLevel> levels;
        ptr::MipChainLevels(rec[0], rec[1], levels);
        if (levels.size() != rec[2]) throw HipError{std::string(who) + ": the texture record's level count is not the chain's"};
        std::vector<uint64_t> offsets(levels.size());
        for (size_t l = 0; l < levels.size(); ++l) offsets[l] = rec[4u + l];
        written += writeMipChain(texels + rec[4], texels, offsets, levels, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t i = 0; i < count; ++i) {
        std::memcpy(&ds.appearanceRecords.texInfo[static_cast<size_t>(u.entry[i].texture) * kTexInfoWords], records + i * kTexInfoWords, kTexInfoWords * 4u);
    }
    report(st, ds.view, u.began, stagingMs, 2, ds.view.rectLightCount, 0u, written, infoOut);
}

// ---------------------------------------------------------------------------------------------------------------- environment
std::string checkEnvironment(const PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, bool fromDevice, int arraysDevice,
                             EnvironmentUpdate& out) {
    out.began = Clock::now();
    const SceneView& v = scene->view;
    if (!v.envRgba || v.envWidth == 0u || v.envHeight == 0u) return "the scene was uploaded without an environment map";
    if (!rgba) return "null pixels";
    if (width != v.envWidth || height != v.envHeight) {
        return "the map was uploaded at " + std::to_string(v.envWidth) + " x " + std::to_string(v.envHeight) + ", not " + std::to_string(width) + " x " +
               std::to_string(height);
    }
    if (width > PTR_APPEARANCE_ENV_MAX_DIM || height > PTR_APPEARANCE_ENV_MAX_DIM) {
        return "a map of " + std::to_string(width) + " x " + std::to_string(height) + " is above the " +
               std::to_string(static_cast<uint32_t>(PTR_APPEARANCE_ENV_MAX_DIM)) + " entries an alias table may have here";
    }
    if (fromDevice) {
        const std::string bad = devicePointerProblem(rgba, static_cast<size_t>(width) * height * sizeof(float4), arraysDevice);
        if (!bad.empty()) return "the pixel array " + bad;
    }
    out.fromDevice = fromDevice, out.rgba = rgba, out.width = width, out.height = height;
    ptr::EnvCellWeights(width, height, out.cell);
    return "";
}

std::string stageEnvironment(const EnvironmentUpdate& u, float* pinned) {
    return stageFinite(u.rgba, static_cast<size_t>(u.width) * u.height * 4u, pinned) ? "" : "the map has a non-finite component";
}

void runEnvironment(const char* who, PtrDeviceScene& ds, const EnvironmentUpdate& u, const float* staged, bool checkGiven, hipStream_t stream,
                    PtrAppearanceInfo* infoOut, const InputsEnqueued& enqueued) {
    AppearanceState& st = stateOf(ds);
    SceneView& v = ds.view;
    const uint32_t w = u.width, h = u.height;
    const size_t texels = static_cast<size_t>(w) * h;
    const size_t cellBytes = (static_cast<size_t>(h) * 4u + 4u + 15u) & ~size_t(15);   // the cell weights, then the total's landing place
    char* pinned = static_cast<char*>(st.pinned.pinnedFor(cellBytes + checkBytes(1)));
    float* pCell = reinterpret_cast<float*>(pinned);
    float* pTotal = pCell + h;
    char* checkScratch = pinned + cellBytes;   // (behind them: the check must not write over the weights)
    std::memcpy(pCell, u.cell.data(), static_cast<size_t>(h) * 4u);
    st.envWeight.ensure(texels), st.envRowWeight.ensure(h), st.envCell.ensure(h), st.envTotal.ensure(1);
    const double stagingMs = msSince(u.began);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    if (u.fromDevice) {
        if (checkGiven && firstNonFiniteOf(st, checkScratch, 1u, [&](size_t) { return DynCheckRow{u.rgba, static_cast<uint64_t>(texels) * 4u}; }, stream) >= 0) {
            throw Refused{std::string(who) + ": the map has a non-finite component"};
        }
        HIP_CHECK(hipMemcpyAsync(ds.envRgba.ptr, u.rgba, texels * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    } else {
        HIP_CHECK(hipMemcpyAsync(ds.envRgba.ptr, staged, texels * sizeof(float4), hipMemcpyHostToDevice, stream));
    }
    HIP_CHECK(hipMemcpyAsync(st.envCell.ptr, pCell, static_cast<size_t>(h) * 4u, hipMemcpyHostToDevice, stream));
    if (enqueued) enqueued();
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    launchAppEnvWeights(ds.envRgba.ptr, st.envCell.ptr, w, h, st.envWeight.ptr, st.envRowWeight.ptr, stream);
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    launchAppEnvTotal(st.envWeight.ptr, texels, st.envTotal.ptr, stream);
    HIP_CHECK(hipEventRecord(st.events[3], stream));
    HIP_CHECK(hipMemcpyAsync(pTotal, st.envTotal.ptr, sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const bool lit = !(*pTotal <= 0.0f);   // a fresh upload keeps the distribution unless the total is <= 0
    if (lit) {
        ds.envCond.ensure(texels), ds.envMarg.ensure(h), ds.envPdf.ensure(texels);
        launchAppEnvAlias(st.envWeight.ptr, st.envRowWeight.ptr, st.envTotal.ptr, w, h, ds.envCond.ptr, ds.envMarg.ptr, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[4], stream));
    if (lit) launchAppEnvPdf(st.envWeight.ptr, st.envCell.ptr, st.envTotal.ptr, w, h, ds.envPdf.ptr, stream);
    HIP_CHECK(hipEventRecord(st.events[5], stream));
    uint64_t written = texels;
    if (ds.envMipLevels > 0u) {
        // the chain's record is followed by levels 1 .., their offsets counted from the first texel after the record (ensureEnvMips)
        std::vector<ptr::MipLevel> levels;
        ptr::MipChainLevels(w, h, levels);
        if (levels.size() != ds.envMipLevels) throw HipError{std::string(who) + ": the environment chain's level count is not the map's"};
        std::vector<uint64_t> offsets(levels.size(), 0u);
        for (size_t l = 2; l < levels.size(); ++l) offsets[l] = offsets[l - 1u] + static_cast<uint64_t>(levels[l - 1u].width) * levels[l - 1u].height;
        written += writeMipChain(ds.envRgba.ptr, ds.envMips.ptr + kTexInfoWords / 4u, offsets, levels, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[6], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    v.envSampling = lit ? 1u : 0u;
    v.envCond = lit ? ds.envCond.ptr : nullptr;
    v.envMarg = lit ? ds.envMarg.ptr : nullptr;
    v.envPdf = lit ? ds.envPdf.ptr : nullptr;
    report(st, v, u.began, stagingMs, 6, v.rectLightCount, 0u, written, infoOut);
}

}  // namespace ptrhost

namespace {

int setTextures(const char* who, PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, void* stream, PtrAppearanceInfo* info,
                char* err, size_t err_cap) {
    TexturesUpdate u;
    float* staged = nullptr;
    return updateCall(who, scene, err, err_cap,
                      [&] {
                          const std::string problem = checkTextures(scene, textures, count, fromDevice, scene->device, u);
                          if (!problem.empty() || fromDevice) return problem;
                          // staging: the pixels into the scene's pinned buffer, each component looked at on the way
                          HIP_CHECK(hipSetDevice(scene->device));
                          staged = static_cast<float*>(stateOf(*scene).staged.pinnedFor(u.floats * sizeof(float)));
                          return stageTextures(u, staged);
                      },
                      [&] { runTextures(who, *scene, u, staged, true, static_cast<hipStream_t>(stream), info); });
}

int setEnvironment(const char* who, PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, bool fromDevice, void* stream,
                   PtrAppearanceInfo* info, char* err, size_t err_cap) {
    EnvironmentUpdate u;
    float* staged = nullptr;
    return updateCall(who, scene, err, err_cap,
                      [&] {
                          const std::string problem = checkEnvironment(scene, rgba, width, height, fromDevice, scene->device, u);
                          if (!problem.empty() || fromDevice) return problem;
                          // staging, as for the textures
                          HIP_CHECK(hipSetDevice(scene->device));
                          staged = static_cast<float*>(stateOf(*scene).staged.pinnedFor(static_cast<size_t>(width) * height * sizeof(float4)));
                          return stageEnvironment(u, staged);
                      },
                      [&] { runEnvironment(who, *scene, u, staged, true, static_cast<hipStream_t>(stream), info); });
}

}  // namespace

extern "C" {

int ptr_scene_set_materials(PtrDeviceScene* scene, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, void* stream,
                            PtrAppearanceInfo* info, char* err, size_t err_cap) {
    MaterialsUpdate u;
    return updateCall("ptr_scene_set_materials", scene, err, err_cap, [&] { return checkMaterials(scene, indices, materials, count, u); },
                      [&] { runMaterials(*scene, u, static_cast<hipStream_t>(stream), info); });
}

int ptr_scene_set_textures(PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, void* stream, PtrAppearanceInfo* info, char* err,
                           size_t err_cap) {
    return setTextures("ptr_scene_set_textures", scene, textures, count, false, stream, info, err, err_cap);
}

int ptr_scene_set_textures_device(PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, void* stream, PtrAppearanceInfo* info,
                                  char* err, size_t err_cap) {
    return setTextures("ptr_scene_set_textures_device", scene, textures, count, true, stream, info, err, err_cap);
}

int ptr_scene_set_environment(PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, void* stream, PtrAppearanceInfo* info,
                              char* err, size_t err_cap) {
    return setEnvironment("ptr_scene_set_environment", scene, rgba, width, height, false, stream, info, err, err_cap);
}

int ptr_scene_set_environment_device(PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, void* stream, PtrAppearanceInfo* info,
                                     char* err, size_t err_cap) {
    return setEnvironment("ptr_scene_set_environment_device", scene, rgba, width, height, true, stream, info, err, err_cap);
}

int ptr_debug_appearance_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out) {
    if (!scene || !size_out) return 1;
    const PtrDeviceScene& ds = *scene;
    const SceneView& v = ds.view;
    const uint64_t envTexels = static_cast<uint64_t>(v.envWidth) * v.envHeight;
    const bool sampled = v.envSampling != 0u;
    uint32_t scalars[6];
    const void* src = nullptr;
    uint64_t bytes = 0;
    bool host = false;
    switch (which) {
        case PTR_APPEARANCE_MATERIALS: src = ds.materials.ptr, bytes = static_cast<uint64_t>(v.materialCount) * kMaterialVec4 * 16u; break;
        case PTR_APPEARANCE_MATERIAL_TEX: src = ds.materialTex.ptr, bytes = v.textureCount ? static_cast<uint64_t>(v.materialCount) * kMaterialTexVec4 * 16u : 0u; break;
        case PTR_APPEARANCE_RECT_LIGHTS: src = ds.rectLights.ptr, bytes = static_cast<uint64_t>(v.rectLightCount) * kRectLightVec4 * 16u; break;
        case PTR_APPEARANCE_LIGHT_INDEX_BY_RECT: src = ds.lightIndexByRect.ptr, bytes = static_cast<uint64_t>(v.rectCount) * 4u; break;
        case PTR_APPEARANCE_TEXELS: {
            // every level of every texture: the last texture's last level ends the array
            uint64_t texels = 0;
            for (uint32_t t = 0; t < v.textureCount; ++t) {
                const uint32_t* rec = &ds.appearanceRecords.texInfo[static_cast<size_t>(t) * kTexInfoWords];
                std::vector<ptr::MipLevel> levels;
                ptr::MipChainLevels(rec[0], rec[1], levels);
                const ptr::MipLevel last = levels.back();
                texels = std::max<uint64_t>(texels, static_cast<uint64_t>(rec[4u + levels.size() - 1u]) + static_cast<uint64_t>(last.width) * last.height);
            }
            src = ds.texels.ptr, bytes = texels * 16u;
            break;
        }
        case PTR_APPEARANCE_TEX_INFO: src = ds.texInfo.ptr, bytes = static_cast<uint64_t>(v.textureCount) * kTexInfoWords * 4u; break;
        case PTR_APPEARANCE_ENV_RGBA: src = ds.envRgba.ptr, bytes = v.envRgba ? envTexels * 16u : 0u; break;
        case PTR_APPEARANCE_ENV_COND: src = ds.envCond.ptr, bytes = sampled ? envTexels * 8u : 0u; break;
        case PTR_APPEARANCE_ENV_MARG: src = ds.envMarg.ptr, bytes = sampled ? static_cast<uint64_t>(v.envHeight) * 8u : 0u; break;
        case PTR_APPEARANCE_ENV_PDF: src = ds.envPdf.ptr, bytes = sampled ? envTexels * 4u : 0u; break;
        case PTR_APPEARANCE_ENV_MIPS: {
            uint64_t texels = 0;
            if (ds.envMipLevels > 0u) {
                std::vector<ptr::MipLevel> levels;
                ptr::MipChainLevels(v.envWidth, v.envHeight, levels);
                for (size_t l = 1; l < levels.size(); ++l) texels += static_cast<uint64_t>(levels[l].width) * levels[l].height;
                texels += kTexInfoWords / 4u;
            }
            src = ds.envMips.ptr, bytes = texels * 16u;
            break;
        }
        case PTR_APPEARANCE_SCALARS:
            scalars[0] = v.materialTypes, scalars[1] = v.rectLightCount, scalars[2] = v.settleRectLights, scalars[3] = ds.hasRandomWalkMaterial ? 1u : 0u;
            scalars[4] = v.envSampling, scalars[5] = ds.envMipLevels;
            src = scalars, bytes = sizeof(scalars), host = true;
            break;
        default: return 1;
    }
    return probeArrayTail(ds.device, src, host, bytes, out, cap_bytes, size_out);
}

}  // extern "C"
