// Appearance updates of a resident scene (include/ptr_appearance.h): ptr_scene_set_materials, ptr_scene_set_textures and
// ptr_scene_set_environment with their device-pointer forms, and the header's test-only probe.  The rules that need no device are in
// appearance_host.cpp (plain C++); the kernels are in kernels/appearance.hip.  Compiled with hipcc (host code only), like dynamic.cpp.
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

using Clock = std::chrono::steady_clock;
constexpr uint32_t kTexInfoWords = 20u;   // kernels/texture.h: width, height, levels, wrap / filter, then the 16 level offsets
constexpr uint32_t kRowFloats = ptr::kCompactMaterialFloats;
static_assert(kRowFloats == kMaterialVec4 * 4u && kRowFloats == kMaterialTexVec4 * 4u, "material row layouts");

double msSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// The state of the appearance calls, made at the first of them: the mirrors come from the device arrays as they are now.
AppearanceState& stateOf(PtrDeviceScene& ds) {
    if (ds.appearance) return *ds.appearance;
    auto st = std::make_unique<AppearanceState>();
    const SceneView& v = ds.view;
    st->materialRows.resize(static_cast<size_t>(v.materialCount) * kRowFloats);
    if (v.materialCount) HIP_CHECK(hipMemcpy(st->materialRows.data(), ds.materials.ptr, st->materialRows.size() * sizeof(float), hipMemcpyDeviceToHost));
    st->rectMaterial.resize(v.rectCount);
    if (v.rectCount) {
        std::vector<PtrRect> rects(v.rectCount);
        HIP_CHECK(hipMemcpy(rects.data(), ds.rects.ptr, rects.size() * sizeof(PtrRect), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < v.rectCount; ++i) st->rectMaterial[i] = rects[i].materialTwoSided[0];
    }
    st->texInfo.resize(static_cast<size_t>(v.textureCount) * kTexInfoWords);
    if (v.textureCount) HIP_CHECK(hipMemcpy(st->texInfo.data(), ds.texInfo.ptr, st->texInfo.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (hipEvent_t& e : st->events) HIP_CHECK(hipEventCreate(&e));
    st->words.ensure(64);
    ds.appearance = std::move(st);
    return *ds.appearance;
}

void elapsed(AppearanceState& st, int steps, PtrAppearanceInfo& info) {
    for (int g = 0; g < steps; ++g) {
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, st.events[g], st.events[g + 1]));
        info.kernelMs[g] = ms;
    }
}

// k_dyn_check_finite over the caller's device arrays (`arrays[r]`: floats[r] floats): a set bit ends the call before anything the renderer
// reads has been written.  Returns the first array with a non-finite float, or -1.  pinned: checkBytes(n) of the caller's pinned block,
// 16 B aligned, which the caller lays out beside whatever else it keeps there.
size_t checkBytes(size_t n) { return n * sizeof(DynCheckRow) + ((n + 31u) / 32u) * sizeof(uint32_t) + 16u; }
int firstNonFinite(AppearanceState& st, char* pinned, const std::vector<const float*>& arrays, const std::vector<uint64_t>& floats, hipStream_t stream) {
    const size_t n = arrays.size(), words = (n + 31u) / 32u;
    st.checkRows.ensure(n);
    st.words.ensure(1u + words);
    DynCheckRow* rows = reinterpret_cast<DynCheckRow*>(pinned);
    uint32_t* flags = reinterpret_cast<uint32_t*>(pinned + n * sizeof(DynCheckRow));
    uint64_t largest = 0;
    for (size_t r = 0; r < n; ++r) rows[r] = DynCheckRow{arrays[r], floats[r]}, largest = std::max(largest, floats[r]);
    HIP_CHECK(hipMemcpyAsync(st.checkRows.ptr, rows, n * sizeof(DynCheckRow), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(st.words.ptr + 1, 0, words * sizeof(uint32_t), stream));
    launchDynCheckFinite(reinterpret_cast<const DynCheckRow*>(st.checkRows.ptr), static_cast<uint32_t>(n), largest, st.words.ptr + 1, stream);
    HIP_CHECK(hipMemcpyAsync(flags, st.words.ptr + 1, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t r = 0; r < n; ++r) {
        if (flags[r >> 5] >> (r & 31u) & 1u) return static_cast<int>(r);
    }
    return -1;
}

// copies `n` floats into `dst`; false when one of them is not finite
bool stageFinite(const float* src, size_t n, float* dst) {
    bool finite = true;
    for (size_t k = 0; k < n; ++k) {
        finite = finite && std::isfinite(src[k]);
        dst[k] = src[k];
    }
    return finite;
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

// ---------------------------------------------------------------------------------------------------------------- materials
void runMaterials(const char* who, PtrDeviceScene& ds, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, hipStream_t stream,
                  PtrAppearanceInfo* infoOut) {
    const auto t0 = Clock::now();
    AppearanceState& st = stateOf(ds);
    SceneView& v = ds.view;
    const uint32_t materialCount = v.materialCount;
    const bool keepsPrimitives = ds.dynamic && (ds.dynamic->flags & PTR_DYNAMIC_PRIMITIVES);
    std::vector<uint8_t> named(materialCount, 0);
    for (uint32_t i = 0; i < count; ++i) named[indices[i]] = 1;
    bool touchesRects = false;
    for (uint32_t r = 0; r < v.rectCount && !touchesRects; ++r) touchesRects = named[std::min(st.rectMaterial[r], materialCount - 1u)] != 0;
    if (touchesRects && !keepsPrimitives) {
        throw Refused{std::string(who) + ": a rectangle uses a named material and the scene does not keep its rectangles (upload it with "
                                         "ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_PRIMITIVES)"};
    }
    const bool textured = v.textureCount > 0u;

    // the new rows on the host: compact rows, texture rows, and what follows from them
    std::vector<float> rows, texRows(textured ? static_cast<size_t>(count) * kRowFloats : 0u);
    rows.reserve(static_cast<size_t>(count) * kRowFloats);
    for (uint32_t i = 0; i < count; ++i) {
        compactMaterial(materials[i], rows);
        if (textured) materialTexRow(materials[i], &texRows[static_cast<size_t>(i) * kRowFloats]);
    }
    std::vector<float> next = st.materialRows;
    bool keyChanged = false;
    for (uint32_t i = 0; i < count; ++i) {
        float* dst = &next[static_cast<size_t>(indices[i]) * kRowFloats];
        const float* src = &rows[static_cast<size_t>(i) * kRowFloats];
        keyChanged = keyChanged || ptr::ShadeKeyOfType(ptr::CompactMaterialType(dst)) != ptr::ShadeKeyOfType(ptr::CompactMaterialType(src));
        std::memcpy(dst, src, kRowFloats * sizeof(float));
    }
    uint32_t typeMask = 0;
    bool randomWalk = false;
    ptr::MaterialTableFacts(next.data(), materialCount, typeMask, randomWalk);
    ptr::RectLightTable lights;
    if (touchesRects) {
        const PrimitiveRecords& prims = ds.dynamic->prims;
        ptr::DeriveRectLights(prims.rects.data(), static_cast<uint32_t>(prims.rects.size()), prims.rectTriLeaf.data(), next.data(), materialCount, lights);
    }
    std::vector<uint8_t> keys;
    if (keyChanged) ptr::BuildShadeKeyTable(next.data(), materialCount, keys);

    // one pinned block: rows | texture rows | light rows | lightIndexByRect | keys | the counter's landing place
    const size_t rowBytes = rows.size() * 4u, texBytes = texRows.size() * 4u, lightBytes = lights.lights.size() * 4u;
    const size_t indexBytes = lights.lightIndexByRect.size() * 4u, keyBytes = (keys.size() + 15u) & ~size_t(15);
    char* pinned = static_cast<char*>(st.pinnedFor(rowBytes + texBytes + lightBytes + indexBytes + keyBytes + 16u));
    char* pTex = pinned + rowBytes;
    char* pLights = pTex + texBytes;
    char* pIndex = pLights + lightBytes;
    char* pKeys = pIndex + indexBytes;
    uint32_t* pChanged = reinterpret_cast<uint32_t*>(pKeys + keyBytes);
    std::memcpy(pinned, rows.data(), rowBytes);
    if (texBytes) std::memcpy(pTex, texRows.data(), texBytes);
    if (lightBytes) std::memcpy(pLights, lights.lights.data(), lightBytes);
    if (indexBytes) std::memcpy(pIndex, lights.lightIndexByRect.data(), indexBytes);
    if (!keys.empty()) std::memcpy(pKeys, keys.data(), keys.size());
    *pChanged = 0u;
    if (touchesRects) {
        ds.rectLights.ensure(lights.lights.size() / 4u);   // (a table that grows moves; every row of it is written below)
        v.rectLights = ds.rectLights.ptr;
    }
    if (keyChanged) st.keys.ensure(keys.size());
    const double stagingMs = msSince(t0);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    for (uint32_t i = 0; i < count; ++i) {
        const size_t at = static_cast<size_t>(indices[i]) * kMaterialVec4;
        HIP_CHECK(hipMemcpyAsync(ds.materials.ptr + at, pinned + static_cast<size_t>(i) * kRowFloats * 4u, kRowFloats * 4u, hipMemcpyHostToDevice, stream));
        if (textured) HIP_CHECK(hipMemcpyAsync(ds.materialTex.ptr + at, pTex + static_cast<size_t>(i) * kRowFloats * 4u, kRowFloats * 4u, hipMemcpyHostToDevice, stream));
    }
    if (touchesRects) {
        if (lightBytes) HIP_CHECK(hipMemcpyAsync(ds.rectLights.ptr, pLights, lightBytes, hipMemcpyHostToDevice, stream));
        if (indexBytes) HIP_CHECK(hipMemcpyAsync(ds.lightIndexByRect.ptr, pIndex, indexBytes, hipMemcpyHostToDevice, stream));
    }
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    if (keyChanged) {
        HIP_CHECK(hipMemcpyAsync(st.keys.ptr, pKeys, keys.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(st.words.ptr, 0, sizeof(uint32_t), stream));
        launchAppRekey(ds.tris.ptr, static_cast<uint32_t>(ds.info[2]), st.keys.ptr, materialCount, st.words.ptr, stream);
        HIP_CHECK(hipMemcpyAsync(pChanged, st.words.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        // a dynamic scene bakes the w words of its triangle rows out of the object-space corner rows: they follow (counted apart)
        if (ds.dynamic) launchAppRekey(ds.dynamic->objPos.ptr, ds.dynamic->triCount, st.keys.ptr, materialCount, st.words.ptr + 1, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    HIP_CHECK(hipStreamSynchronize(stream));

    // the host's records follow
    const uint32_t lightsBefore = v.rectLightCount;
    st.materialRows.swap(next);
    v.materialTypes = typeMask;
    ds.hasRandomWalkMaterial = randomWalk;
    if (touchesRects) {
        PrimitiveRecords& prims = ds.dynamic->prims;
        v.rectLights = ds.rectLights.ptr;
        v.rectLightCount = lights.lightCount;
        v.settleRectLights = (lights.lightCount > 0u && lights.lightCount <= kSettleLightsMax && lights.lightsHaveTriangles) ? 1u : 0u;
        ds.info[7] = lights.lightCount;
        prims.lightIndexByRect = lights.lightIndexByRect;
        prims.rectEmission = lights.rectEmission;
        prims.rectShadeKey = lights.rectShadeKey;
    }
    if (infoOut) {
        PtrAppearanceInfo info{};
        info.stagingMs = stagingMs;
        elapsed(st, 2, info);
        info.rowsRekeyed = *pChanged;
        info.lightsBefore = lightsBefore, info.lightsAfter = v.rectLightCount;
        info.envSampling = v.envSampling;
        info.totalSeconds = std::chrono::duration<double>(Clock::now() - t0).count();
        *infoOut = info;
    }
}

// ---------------------------------------------------------------------------------------------------------------- textures
void runTextures(const char* who, PtrDeviceScene& ds, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, hipStream_t stream,
                 PtrAppearanceInfo* infoOut) {
    const auto t0 = Clock::now();
    AppearanceState& st = stateOf(ds);
    const uint32_t textureCount = ds.view.textureCount;
    std::vector<uint8_t> named(textureCount, 0);
    size_t floats = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const PtrTextureUpdate& t = textures[i];
        const std::string name = "texture " + std::to_string(t.textureIndex);
        if (t.textureIndex >= textureCount) {
            throw Refused{std::string(who) + ": texture index " + std::to_string(t.textureIndex) + " out of range (the scene has " + std::to_string(textureCount) + " textures)"};
        }
        if (named[t.textureIndex]++) throw Refused{std::string(who) + ": texture index " + std::to_string(t.textureIndex) + " named twice"};
        if (!t.rgba) throw Refused{std::string(who) + ": " + name + " has null pixels"};
        const uint32_t* rec = &st.texInfo[static_cast<size_t>(t.textureIndex) * kTexInfoWords];
        if (t.width != rec[0] || t.height != rec[1]) {
            throw Refused{std::string(who) + ": " + name + " was uploaded at " + std::to_string(rec[0]) + " x " + std::to_string(rec[1]) + ", not " +
                          std::to_string(t.width) + " x " + std::to_string(t.height)};
        }
        const size_t n = static_cast<size_t>(t.width) * t.height * 4u;
        if (fromDevice) {
            const std::string bad = devicePointerProblem(t.rgba, n * sizeof(float), ds.device);
            if (!bad.empty()) throw Refused{std::string(who) + ": the pixel array of " + name + " " + bad};
        }
        floats += n;
    }
    // the records (wrap and filter may change) ride behind the pixels of a host call in one pinned block
    const size_t pixelBytes = fromDevice ? 0u : floats * sizeof(float);
    const size_t recordBytes = static_cast<size_t>(count) * kTexInfoWords * 4u;
    char* pinned = static_cast<char*>(st.pinnedFor(pixelBytes + recordBytes + checkBytes(count)));
    uint32_t* records = reinterpret_cast<uint32_t*>(pinned + pixelBytes);
    char* checkScratch = pinned + pixelBytes + recordBytes;   // (behind the records: the check must not write over them)
    if (!fromDevice) {
        float* at = reinterpret_cast<float*>(pinned);
        for (uint32_t i = 0; i < count; ++i) {
            const size_t n = static_cast<size_t>(textures[i].width) * textures[i].height * 4u;
            if (!stageFinite(textures[i].rgba, n, at)) {
                throw Refused{std::string(who) + ": texture " + std::to_string(textures[i].textureIndex) + " has a non-finite component"};
            }
            at += n;
        }
    }
    for (uint32_t i = 0; i < count; ++i) {
        const PtrTextureUpdate& t = textures[i];
        std::memcpy(records + static_cast<size_t>(i) * kTexInfoWords, &st.texInfo[static_cast<size_t>(t.textureIndex) * kTexInfoWords], kTexInfoWords * 4u);
        records[static_cast<size_t>(i) * kTexInfoWords + 3u] = (t.wrapS & 3u) | ((t.wrapT & 3u) << 2) | ((t.filter ? 1u : 0u) << 4);
    }
    const double stagingMs = msSince(t0);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    if (fromDevice) {
        std::vector<const float*> arrays(count);
        std::vector<uint64_t> sizes(count);
        for (uint32_t i = 0; i < count; ++i) arrays[i] = textures[i].rgba, sizes[i] = static_cast<uint64_t>(textures[i].width) * textures[i].height * 4u;
        const int bad = firstNonFinite(st, checkScratch, arrays, sizes, stream);
        if (bad >= 0) throw Refused{std::string(who) + ": texture " + std::to_string(textures[bad].textureIndex) + " has a non-finite component"};
    }
    float4* texels = ds.texels.ptr;
    uint64_t written = 0;
    const float* staged = reinterpret_cast<const float*>(pinned);
    std::vector<std::vector<ptr::MipLevel>> chains(count);
    for (uint32_t i = 0; i < count; ++i) {
        const PtrTextureUpdate& t = textures[i];
        const uint32_t* rec = records + static_cast<size_t>(i) * kTexInfoWords;
        const size_t n = static_cast<size_t>(t.width) * t.height;
        HIP_CHECK(hipMemcpyAsync(texels + rec[4], fromDevice ? t.rgba : staged, n * sizeof(float4), fromDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(reinterpret_cast<uint32_t*>(ds.texInfo.ptr) + static_cast<size_t>(t.textureIndex) * kTexInfoWords, rec, kTexInfoWords * 4u,
                                 hipMemcpyHostToDevice, stream));
        if (!fromDevice) staged += n * 4u;
        written += n;
    }
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t* rec = records + static_cast<size_t>(i) * kTexInfoWords;
        std::vector<ptr::MipLevel> levels;
        ptr::MipChainLevels(rec[0], rec[1], levels);
        if (levels.size() != rec[2]) throw HipError{std::string(who) + ": the texture record's level count is not the chain's"};
        std::vector<uint64_t> offsets(levels.size());
        for (size_t l = 0; l < levels.size(); ++l) offsets[l] = rec[4u + l];
        written += writeMipChain(texels + rec[4], texels, offsets, levels, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < count; ++i) {
        std::memcpy(&st.texInfo[static_cast<size_t>(textures[i].textureIndex) * kTexInfoWords], records + static_cast<size_t>(i) * kTexInfoWords, kTexInfoWords * 4u);
    }
    if (infoOut) {
        PtrAppearanceInfo info{};
        info.stagingMs = stagingMs;
        elapsed(st, 2, info);
        info.texelsWritten = written;
        info.lightsBefore = info.lightsAfter = ds.view.rectLightCount;
        info.envSampling = ds.view.envSampling;
        info.totalSeconds = std::chrono::duration<double>(Clock::now() - t0).count();
        *infoOut = info;
    }
}

// ---------------------------------------------------------------------------------------------------------------- environment
void runEnvironment(const char* who, PtrDeviceScene& ds, const float* rgba, bool fromDevice, hipStream_t stream, PtrAppearanceInfo* infoOut) {
    const auto t0 = Clock::now();
    AppearanceState& st = stateOf(ds);
    SceneView& v = ds.view;
    const uint32_t w = v.envWidth, h = v.envHeight;
    const size_t texels = static_cast<size_t>(w) * h;
    if (fromDevice) {
        const std::string bad = devicePointerProblem(rgba, texels * sizeof(float4), ds.device);
        if (!bad.empty()) throw Refused{std::string(who) + ": the pixel array " + bad};
    }
    std::vector<float> cell;
    ptr::EnvCellWeights(w, h, cell);
    const size_t pixelBytes = fromDevice ? 0u : texels * sizeof(float4);
    const size_t cellBytes = (static_cast<size_t>(h) * 4u + 4u + 15u) & ~size_t(15);   // the cell weights, then the total's landing place
    char* pinned = static_cast<char*>(st.pinnedFor(pixelBytes + cellBytes + checkBytes(1)));
    float* pCell = reinterpret_cast<float*>(pinned + pixelBytes);
    float* pTotal = pCell + h;
    char* checkScratch = pinned + pixelBytes + cellBytes;   // (behind them: the check must not write over the weights)
    if (!fromDevice && !stageFinite(rgba, texels * 4u, reinterpret_cast<float*>(pinned))) throw Refused{std::string(who) + ": the map has a non-finite component"};
    std::memcpy(pCell, cell.data(), static_cast<size_t>(h) * 4u);
    st.envWeight.ensure(texels), st.envRowWeight.ensure(h), st.envCell.ensure(h), st.envTotal.ensure(1);
    const double stagingMs = msSince(t0);

    HIP_CHECK(hipEventRecord(st.events[0], stream));
    if (fromDevice) {
        if (firstNonFinite(st, checkScratch, {rgba}, {static_cast<uint64_t>(texels) * 4u}, stream) >= 0) throw Refused{std::string(who) + ": the map has a non-finite component"};
        HIP_CHECK(hipMemcpyAsync(ds.envRgba.ptr, rgba, texels * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    } else {
        HIP_CHECK(hipMemcpyAsync(ds.envRgba.ptr, pinned, texels * sizeof(float4), hipMemcpyHostToDevice, stream));
    }
    HIP_CHECK(hipMemcpyAsync(st.envCell.ptr, pCell, static_cast<size_t>(h) * 4u, hipMemcpyHostToDevice, stream));
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
    if (infoOut) {
        PtrAppearanceInfo info{};
        info.stagingMs = stagingMs;
        elapsed(st, 6, info);
        info.texelsWritten = written;
        info.lightsBefore = info.lightsAfter = v.rectLightCount;
        info.envSampling = v.envSampling;
        info.totalSeconds = std::chrono::duration<double>(Clock::now() - t0).count();
        *infoOut = info;
    }
}

int setTextures(const char* who, PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, void* stream, PtrAppearanceInfo* info,
                char* err, size_t err_cap) {
    if (!scene) return nullArgument(who, err, err_cap);
    if (scene->view.textureCount == 0u) return refuse(err, err_cap, std::string(who) + ": the scene has no textures");
    const std::string bad = listProblem(textures, count, "null texture list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    return deviceCall(who, scene, true, err, err_cap, [&] { runTextures(who, *scene, textures, count, fromDevice, static_cast<hipStream_t>(stream), info); });
}

int setEnvironment(const char* who, PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, bool fromDevice, void* stream,
                   PtrAppearanceInfo* info, char* err, size_t err_cap) {
    if (!scene) return nullArgument(who, err, err_cap);
    const SceneView& v = scene->view;
    if (!v.envRgba || v.envWidth == 0u || v.envHeight == 0u) return refuse(err, err_cap, std::string(who) + ": the scene was uploaded without an environment map");
    if (!rgba) return refuse(err, err_cap, std::string(who) + ": null pixels");
    if (width != v.envWidth || height != v.envHeight) {
        return refuse(err, err_cap, std::string(who) + ": the map was uploaded at " + std::to_string(v.envWidth) + " x " + std::to_string(v.envHeight) + ", not " +
                                        std::to_string(width) + " x " + std::to_string(height));
    }
    if (width > PTR_APPEARANCE_ENV_MAX_DIM || height > PTR_APPEARANCE_ENV_MAX_DIM) {
        return refuse(err, err_cap, std::string(who) + ": a map of " + std::to_string(width) + " x " + std::to_string(height) + " is above the " +
                                        std::to_string(static_cast<uint32_t>(PTR_APPEARANCE_ENV_MAX_DIM)) + " entries an alias table may have here");
    }
    return deviceCall(who, scene, true, err, err_cap, [&] { runEnvironment(who, *scene, rgba, fromDevice, static_cast<hipStream_t>(stream), info); });
}

static_assert(PTR_APPEARANCE_ENV_MAX_DIM == kAppAliasMaxEntries, "the header's bound is the kernel's");

}  // namespace

extern "C" {

int ptr_scene_set_materials(PtrDeviceScene* scene, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, void* stream,
                            PtrAppearanceInfo* info, char* err, size_t err_cap) {
    static const char* const who = "ptr_scene_set_materials";
    if (!scene) return nullArgument(who, err, err_cap);
    try {
        const std::string problem = ptr::MaterialListProblem(indices, materials, count, scene->view.materialCount, scene->view.textureCount);
        if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    }
    PTR_CATCH_ALL(err, err_cap)
    return deviceCall(who, scene, true, err, err_cap, [&] { runMaterials(who, *scene, indices, materials, count, static_cast<hipStream_t>(stream), info); });
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
            if (v.textureCount) {
                std::vector<uint32_t> info(static_cast<size_t>(v.textureCount) * kTexInfoWords);
                if (hipSetDevice(ds.device) != hipSuccess || hipMemcpy(info.data(), ds.texInfo.ptr, info.size() * 4u, hipMemcpyDeviceToHost) != hipSuccess) return 3;
                for (uint32_t t = 0; t < v.textureCount; ++t) {
                    const uint32_t* rec = &info[static_cast<size_t>(t) * kTexInfoWords];
                    std::vector<ptr::MipLevel> levels;
                    ptr::MipChainLevels(rec[0], rec[1], levels);
                    const ptr::MipLevel last = levels.back();
                    texels = std::max<uint64_t>(texels, static_cast<uint64_t>(rec[4u + levels.size() - 1u]) + static_cast<uint64_t>(last.width) * last.height);
                }
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
    *size_out = bytes;
    if (!out) return 0;
    if (cap_bytes < bytes) return 2;
    if (bytes == 0u) return 0;
    if (host) {
        std::memcpy(out, src, bytes);
        return 0;
    }
    if (hipSetDevice(ds.device) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}

}  // extern "C"
