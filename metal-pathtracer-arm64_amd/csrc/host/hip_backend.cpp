// Device side of the C-ABI: scene upload (BVH build + SoA flattening + H2D), the wavefront render loop,
// and ray-batch queries.  Compiled with hipcc (host code only; kernels live in kernels/wavefront.hip).
//
// Reference counterparts: SceneResources::rebuildAccelerationStructures (src/renderer/SceneResources.mm:2055-2259),
// SoftwareBvhAccel::rebuild (src/renderer/SceneAccel.mm:23-325), the per-sample dispatch loop
// (src/renderer/RenderLoop.mm:366-386, src/headless/MetalHeadlessRenderer.mm:64-92) and the Embree backend's
// scene assembly (src/headless/EmbreeHeadlessRenderer.mm:2077-2300, 2484-2522).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <functional>
#include <vector>

#include "bvh_builder.h"
#include "device_scene.h"
#include "env_importance_sampler.h"
#include "geometry_cache.h"
#include "knobs.h"
#include "dynamic_host.h"
#include "ptr_deform_device.h"
#include "ptr_dynamic.h"
#include "scene_geometry.h"
#include "vecmath.h"

using namespace ptrk;
using namespace ptrhost;

namespace {

using ptr::float3;

// per-group scalars: [0] unused, [1] k_extend work head, [2] k_connect work head, [3] pad,
//                    [4..19] ring of live-slot counters (one per iteration, written by k_extend at the end of a frame)
constexpr uint32_t kAliveRing = 16;
constexpr uint32_t kAliveBase = 4;
constexpr uint32_t kScalarCount = kAliveBase + kAliveRing;
constexpr uint64_t kHalfGridGroupSlots = 3ull << 20;   // groups at least this large launch k_extend / k_connect on half the wave slots
constexpr uint32_t kMaxPoolGroups = 8;        // one block of scalars / one spill area per group
constexpr uint32_t kPinnedHeadsOffset = 16;
constexpr uint32_t kTexInfoWords = 20;   // kernels/texture.h kTexInfoVec4 uint4 per texture   // pinned staging: [0..15] per-group live-slot counts, then kItemHeads range heads

// Stack spill area of one pool group: the stack levels beyond kLdsStackLevels, one column per thread of the persistent grid.  The
// four-wide walk pushes at most three entries per step (two binary levels), plus the root beside an oversize leaf: a tree of binary
// depth d needs 3 ceil(d / 2) + 2 entries, not the worst case kTraversalStackDepth (1 GB of HBM per scene for 8 groups).
size_t spillWordsPerGroup(const PtrDeviceScene& ds) { return static_cast<size_t>(ds.spillLevels) * ds.traceGrid * kTraceGridUnit; }

}  // namespace

namespace ptrhost {

// 576 B MaterialData -> the 13 float4 the integrator reads (kernels/device_types.h MaterialSlot).
void compactMaterial(const PtrMaterial& m, std::vector<float>& out) {
    const float* rows[kMaterialVec4] = {m.baseColorRoughness, m.typeEta,        m.emission,           m.conductorEta,
                                        m.conductorK,         m.coatParams,     m.coatTint,           m.coatAbsorption,
                                        m.carpaintBaseParams, m.carpaintFlakeParams, m.carpaintBaseEta, m.carpaintBaseK,
                                        m.dielectricSigmaA,   m.sssSigmaA,      m.sssSigmaS,          m.sssParams};
    for (uint32_t r = 0; r < kMaterialVec4; ++r) {
        float v[4] = {rows[r][0], rows[r][1], rows[r][2], rows[r][3]};
        if (r == kMatCoatTint) v[3] = m.pbrParams[0];   // PBR metallic rides in the free w lane
        if (r == kMatDielectricSigmaA) v[3] = m.pbrExtras[2];   // PBR transmission factor (KHR_materials_transmission), Metal PBR model only
        out.insert(out.end(), v, v + 4);
    }
}

// The per-material texture record (kernels/device_types.h kMaterialTexVec4 float4) of one material.
void materialTexRow(const PtrMaterial& m, float* o) {
    for (int r = 0; r < 12; ++r) std::memcpy(o + r * 4, m.textureTransform[r], 16);
    for (int k = 0; k < 4; ++k) o[48 + k] = bitsToFloat(m.textureIndices0[k]);
    o[52] = bitsToFloat(m.textureIndices1[0]);
    o[53] = bitsToFloat(m.textureIndices1[1]);
    const uint32_t uvSets = (std::min(m.textureUvSet0[0], 1u) << 0) | (std::min(m.textureUvSet0[1], 1u) << 1) | (std::min(m.textureUvSet0[2], 1u) << 2) |
                            (std::min(m.textureUvSet0[3], 1u) << 3) | (std::min(m.textureUvSet1[0], 1u) << 4) | (std::min(m.textureUvSet1[1], 1u) << 5);
    o[54] = bitsToFloat(uvSets);
    o[55] = bitsToFloat(m.materialFlags);
    std::memcpy(o + 56, m.pbrParams, 16);
    std::memcpy(o + 60, m.pbrExtras, 16);
}

// Mip chain of one texture appended to `texels`: level l + 1 halves both sizes (at least 1) and averages the 2x2 block of level
// l under each of its texels, the second tap clamped at the edge of odd-sized levels; sums in the order ((a + b) + (c + d)) * 0.25.
void appendTextureWithMips(const PtrTexture& t, std::vector<float>& texels, std::vector<uint32_t>& info) {
    uint32_t w = t.width, h = t.height, levels = 1;
    for (uint32_t a = w, b = h; a > 1u || b > 1u; a = std::max(a / 2u, 1u), b = std::max(b / 2u, 1u)) ++levels;
    levels = std::min(levels, 16u);
    const size_t head = info.size();
    info.resize(head + kTexInfoWords, 0u);
    info[head + 0] = t.width;
    info[head + 1] = t.height;
    info[head + 2] = levels;
    info[head + 3] = (t.wrapS & 3u) | ((t.wrapT & 3u) << 2) | ((t.filter ? 1u : 0u) << 4);
    size_t prev = texels.size() / 4u;
    info[head + 4] = static_cast<uint32_t>(prev);
    texels.insert(texels.end(), t.rgba, t.rgba + static_cast<size_t>(w) * h * 4u);
    for (uint32_t l = 1; l < levels; ++l) {
        const uint32_t nw = std::max(w / 2u, 1u), nh = std::max(h / 2u, 1u);
        const size_t at = texels.size() / 4u;
        info[head + 4 + l] = static_cast<uint32_t>(at);
        texels.resize(texels.size() + static_cast<size_t>(nw) * nh * 4u);
        for (uint32_t y = 0; y < nh; ++y) {
            const uint32_t y0 = std::min(2u * y, h - 1u), y1 = std::min(2u * y + 1u, h - 1u);
            for (uint32_t x = 0; x < nw; ++x) {
                const uint32_t x0 = std::min(2u * x, w - 1u), x1 = std::min(2u * x + 1u, w - 1u);
                const float* a = &texels[(prev + static_cast<size_t>(y0) * w + x0) * 4u];
                const float* b = &texels[(prev + static_cast<size_t>(y0) * w + x1) * 4u];
                const float* c = &texels[(prev + static_cast<size_t>(y1) * w + x0) * 4u];
                const float* d = &texels[(prev + static_cast<size_t>(y1) * w + x1) * 4u];
                float* o = &texels[(at + static_cast<size_t>(y) * nw + x) * 4u];
                for (int ch = 0; ch < 4; ++ch) o[ch] = ((a[ch] + b[ch]) + (c[ch] + d[ch])) * 0.25f;
            }
        }
        prev = at;
        w = nw;
        h = nh;
    }
}

}  // namespace ptrhost

namespace ptrhost {

// The geometry half of the preparation: everything a geometry cache file holds (host/geometry_cache.h).
void prepareGeometry(const PtrSceneDesc& desc, ptr::PreparedGeometry& pg, ptr::DynamicTables* dyn) {
    const ptr::Knobs knobs = ptr::readKnobs();
    std::string geoError;
    if (!ptr::BuildSceneGeometry(desc, 0, pg.geo, geoError, dyn)) throw HipError{geoError};
    // 32 B quantised nodes halve the node fetches; use them unless the 16-bit grid is coarse next to the primitives (cell > 1/8 of
    // the mean primitive extent would inflate leaf boxes noticeably)
    const ptr::FlatBvh& bvh = pg.geo.bvh;
    const float maxCell = std::max(std::max(bvh.gridCell[0], bvh.gridCell[1]), bvh.gridCell[2]);
    pg.useQuantized = bvh.nodeCount > 0 && maxCell * 8.0f <= bvh.meanPrimExtent;
    if (knobs.quantizedNodes >= 0) pg.useQuantized = bvh.nodeCount > 0 && knobs.quantizedNodes != 0;
    // four-wide nodes for the persistent traversal kernels; the binary array stays for the cold kernels and the counting build
    if (pg.useQuantized && knobs.wideNodes != 0) {
        // (a tree so lopsided that the by-area wide tree would outgrow the traversal stack keeps the by-level collapse, whose depth is half
        // the binary tree's)
        std::vector<uint32_t>* source = dyn ? &dyn->wideSource : nullptr;
        pg.wideCount = ptr::BuildWideNodes(bvh, knobs.wideNodes == 2 ? ptr::WideCollapse::ByLevel : ptr::WideCollapse::ByArea, pg.wide, &pg.wideDepth, source);
        if (3u * pg.wideDepth + 4u > kTraversalStackDepth) pg.wideCount = ptr::BuildWideNodes(bvh, ptr::WideCollapse::ByLevel, pg.wide, &pg.wideDepth, source);
        if (static_cast<uint64_t>(pg.wideCount) * 64u > 0xFFFFFFFFull) throw HipError{"scene exceeds the 4 GiB node array limit"};
    }
}

// rectangle lights: DiffuseLight rectangles with non-zero emission (:2484-2522), by the one derivation of appearance_host.h
static_assert(ptr::kRectLightFloats == kRectLightVec4 * 4u && ptr::kCompactMaterialFloats == kMaterialVec4 * 4u, "light and material row layouts");
ptr::RectLightTable rectLightsOf(const PtrSceneDesc& desc, const ptr::SceneGeometry& geo) {
    std::vector<float> mats;
    for (uint32_t i = 0; i < desc.materialCount; ++i) compactMaterial(desc.materials[i], mats);
    return ptr::DeriveRectLights(desc.rects, desc.rectCount, geo.rectTriLeaf.data(), mats.data(), desc.materialCount);
}

constexpr uint32_t kMaxMaterials = 65536u;   // material ids 0 .. 0xFFFF
std::string tooManyMaterials(uint32_t count) {
    return std::to_string(count) + " materials; at most 65536 (the medium stack holds 16-bit material ids)";
}

void prepareScene(const PtrSceneDesc& desc, PreparedScene& ps, const char* cachePath, bool dynamic, uint32_t dynamicFlags) {
    using ptr::float3;
    if (desc.materialCount > kMaxMaterials) throw HipError{tooManyMaterials(desc.materialCount)};   // (uploads that do not come through uploadTo)
    const auto t0 = std::chrono::steady_clock::now();
    if (cachePath && *cachePath) {
        std::string error;
        if (!ptr::ReadGeometryCache(cachePath, ptr::SceneFingerprint(desc), ps.pg, error)) throw HipError{error};
        ps.geometryFromCache = true;
    } else {
        ps.dynamic = dynamic;
        ps.dyn.flags = dynamic ? dynamicFlags : 0u;
        prepareGeometry(desc, ps.pg, dynamic ? &ps.dyn : nullptr);
    }
    ps.geometrySeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const ptr::SceneGeometry& geoRef = ps.pg.geo;

    // compact materials
    ps.mats.reserve(static_cast<size_t>(desc.materialCount) * kMaterialVec4 * 4);
    for (uint32_t i = 0; i < desc.materialCount; ++i) compactMaterial(desc.materials[i], ps.mats);
    for (uint32_t i = 0; i < desc.materialCount; ++i) {
        const PtrMaterial& m = desc.materials[i];
        if (static_cast<uint32_t>(m.typeEta[0]) == PTR_MAT_SUBSURFACE && m.sssParams[1] >= 0.5f) ps.hasRandomWalkMaterial = true;
    }

    ps.rectLights = ptr::DeriveRectLights(desc.rects, desc.rectCount, geoRef.rectTriLeaf.data(), ps.mats.data(), desc.materialCount);
    if (desc.envRgba && desc.envWidth > 0 && desc.envHeight > 0) {
        ps.hasEnvDist = ptr::BuildEnvImportanceDistribution(desc.envRgba, desc.envWidth, desc.envHeight, &ps.envDist);
    }
    if (desc.textures && desc.textureCount > 0 && !geoRef.triUv.empty()) {
        for (uint32_t i = 0; i < desc.textureCount; ++i) {
            if (!desc.textures[i].rgba || desc.textures[i].width == 0 || desc.textures[i].height == 0) throw HipError{"texture without pixels"};
            appendTextureWithMips(desc.textures[i], ps.texels, ps.texInfo);
            if (ps.texels.size() / 4u > 0xFFFFFFF0ull) throw HipError{"textures exceed the 4 G texel limit"};
        }
        ps.materialTex.assign(static_cast<size_t>(desc.materialCount) * kMaterialTexVec4 * 4u, 0.0f);
        for (uint32_t i = 0; i < desc.materialCount; ++i) materialTexRow(desc.materials[i], &ps.materialTex[static_cast<size_t>(i) * kMaterialTexVec4 * 4u]);
    }
    ps.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ps.shadingSeconds = ps.seconds - ps.geometrySeconds;
}

void uploadScene(const PtrSceneDesc& desc, const PreparedScene& ps, PtrDeviceScene& ds) {
    const auto t0 = std::chrono::steady_clock::now();
    const ptr::SceneGeometry& geo = ps.pg.geo;
    const ptr::FlatBvh& bvh = geo.bvh;
    const uint32_t triCount = geo.triCount;
    const uint32_t lightCount = ps.rectLights.lightCount;
    ds.hasRandomWalkMaterial = ps.hasRandomWalkMaterial;

    HIP_CHECK(hipSetDevice(ds.device));
    // only the node array the kernels will read goes to the device (a 29 M-triangle scene: 0.5 GB instead of 1.5 GB of nodes)
    const ptr::Knobs knobs = ptr::readKnobs();
    const bool useQuantized = ps.pg.useQuantized;
    if (useQuantized) {
        ds.nodes.release();
        ds.qnodes.upload(reinterpret_cast<const uint4*>(bvh.qnodes.data()), bvh.qnodes.size() / 4);
    } else {
        ds.qnodes.release();
        ds.nodes.upload(reinterpret_cast<const float4*>(bvh.nodes.data()), bvh.nodes.size() / 4);
    }
    ds.tris.upload(reinterpret_cast<const float4*>(geo.triData.data()), geo.triData.size() / 4);
    ds.triNormals.upload(reinterpret_cast<const float4*>(geo.triNormals.data()), geo.triNormals.size() / 4);
    ds.spheres.upload(reinterpret_cast<const float4*>(geo.sphereData.data()), geo.sphereData.size() / 4);
    ds.sphereInfo.upload(reinterpret_cast<const uint2*>(geo.sphereInfo.data()), geo.sphereInfo.size() / 2);
    ds.materials.upload(reinterpret_cast<const float4*>(ps.mats.data()), ps.mats.size() / 4);
    ds.rects.upload(reinterpret_cast<const float4*>(desc.rects), static_cast<size_t>(desc.rectCount) * 5);
    ds.rectLights.upload(reinterpret_cast<const float4*>(ps.rectLights.lights.data()), ps.rectLights.lights.size() / 4);
    ds.lightIndexByRect.upload(ps.rectLights.lightIndexByRect.data(), ps.rectLights.lightIndexByRect.size());

    SceneView& v = ds.view;
    std::memset(&v, 0, sizeof(v));
    v.nodes = ds.nodes.ptr;
    v.tris = ds.tris.ptr;
    v.triNormals = ds.triNormals.ptr;
    v.spheres = ds.spheres.ptr;
    v.sphereInfo = ds.sphereInfo.ptr;
    v.materials = ds.materials.ptr;
    v.rects = ds.rects.ptr;
    v.rectLights = ds.rectLights.ptr;
    v.lightIndexByRect = ds.lightIndexByRect.ptr;
    v.qnodes = ds.qnodes.ptr;
    std::memcpy(v.gridOrigin, bvh.gridOrigin, sizeof(v.gridOrigin));
    std::memcpy(v.gridCell, bvh.gridCell, sizeof(v.gridCell));
    for (int a = 0; a < 3; ++a) v.gridInvCell[a] = 1.0f / bvh.gridCell[a];
    v.useQuantized = useQuantized ? 1u : 0u;
    if (ps.pg.wideCount > 0u) {
        ds.wnodes.upload(reinterpret_cast<const uint4*>(ps.pg.wide.get()), static_cast<size_t>(ps.pg.wideCount) * 4u);
        v.wnodes = ds.wnodes.ptr;
        v.wideBytes = static_cast<uint32_t>(static_cast<size_t>(ps.pg.wideCount) * 64u);
        v.useWide = 1u;
    }
    const size_t nodeBytes = v.useQuantized ? bvh.qnodes.size() * 4u : bvh.nodes.size() * 4u;
    const size_t triBytes = geo.triData.size() * 4u;
    if (nodeBytes > 0xFFFFFFFFull || triBytes > 0xFFFFFFFFull) throw HipError{"scene exceeds the 4 GiB node/triangle array limit"};
    v.nodeBytes = static_cast<uint32_t>(nodeBytes);
    v.triBytes = static_cast<uint32_t>(triBytes);
    v.rootRef = bvh.rootRef;
    v.oversizeRef = bvh.oversizeRef;
    v.materialCount = desc.materialCount;
    v.rectCount = desc.rectCount;
    v.rectLightCount = lightCount;
    for (uint32_t i = 0; i < desc.materialCount; ++i) v.materialTypes |= 1u << std::min(static_cast<uint32_t>(desc.materials[i].typeEta[0]), 7u);
    v.settleRectLights = (lightCount > 0u && lightCount <= kSettleLightsMax && ps.rectLights.lightsHaveTriangles) ? 1u : 0u;

    if (desc.envRgba && desc.envWidth > 0 && desc.envHeight > 0) {
        const size_t texels = static_cast<size_t>(desc.envWidth) * desc.envHeight;
        ds.envRgba.upload(reinterpret_cast<const float4*>(desc.envRgba), texels);
        v.envRgba = ds.envRgba.ptr;
        v.envWidth = desc.envWidth;
        v.envHeight = desc.envHeight;
        if (ps.hasEnvDist) {
            const ptr::EnvImportanceDistribution& dist = ps.envDist;
            static_assert(sizeof(ptr::AliasEntry) == sizeof(float2), "alias entry layout");
            ds.envCond.upload(reinterpret_cast<const float2*>(dist.conditional.data()), dist.conditional.size());
            ds.envMarg.upload(reinterpret_cast<const float2*>(dist.marginal.data()), dist.marginal.size());
            ds.envPdf.upload(dist.texelPdf.data(), dist.texelPdf.size());
            v.envCond = ds.envCond.ptr;
            v.envMarg = ds.envMarg.ptr;
            v.envPdf = ds.envPdf.ptr;
            v.envSampling = 1u;
        }
    }

    if (!ps.texels.empty()) {
        ds.triUv.upload(reinterpret_cast<const float4*>(geo.triUv.data()), geo.triUv.size() / 4);
        ds.triTangent.upload(reinterpret_cast<const float4*>(geo.triTangent.data()), geo.triTangent.size() / 4);
        ds.texels.upload(reinterpret_cast<const float4*>(ps.texels.data()), ps.texels.size() / 4);
        ds.texInfo.upload(reinterpret_cast<const uint4*>(ps.texInfo.data()), ps.texInfo.size() / 4);
        ds.materialTex.upload(reinterpret_cast<const float4*>(ps.materialTex.data()), ps.materialTex.size() / 4);
        v.triUv = ds.triUv.ptr;
        v.triTangent = ds.triTangent.ptr;
        v.texels = ds.texels.ptr;
        v.texInfo = ds.texInfo.ptr;
        v.materialTex = ds.materialTex.ptr;
        v.textureCount = desc.textureCount;
    }

    ds.worldBounds = ptr::boundsOfPrimitives(geo.triData.data(), geo.triData.size() / 12u, geo.sphereData.data(), geo.sphereData.size() / 4u);

    if (ps.dynamic) uploadDynamicTables(desc, ps, ds);   // dynamic.cpp
    fillAppearanceRecords(desc, ps, ds.appearanceRecords);   // appearance.cpp

    ds.info[0] = bvh.nodeCount;
    ds.info[1] = bvh.leafCount;
    ds.info[2] = triCount;
    ds.info[3] = desc.sphereCount;
    ds.info[4] = bvh.maxDepth;
    ds.info[5] = bvh.maxLeafSize;
    ds.info[6] = static_cast<uint64_t>(bvh.sahCost * 1000.0);
    ds.info[7] = lightCount;

    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, ds.device));
    ds.deviceTotalBytes = prop.totalGlobalMem;
    const uint32_t cus = prop.multiProcessorCount > 0 ? static_cast<uint32_t>(prop.multiProcessorCount) : 256u;
    ds.traceGrid = cus * 8u;   // 8 blocks of 256 threads per CU: fills the wave slots, grid-stride the rest
    if (knobs.refillBelow > 0) ds.refillBelow = knobs.refillBelow;
    // Half the wave slots when the pool runs as several groups of large launches: the kernels of the other groups (k_shade above all,
    // which needs 128 VGPRs a wave) then always find room beside a traversal kernel instead of queueing behind its last waves, and each
    // persistent wave sees twice as many rays before its own tail.  Measured on configs 2 / 3 / 4: +3.5 / +1.5 / +1.5 %, one rank of
    // eight 47.7 -> 44.5 ms; frames of a few milliseconds (config 1) lose 10 % and keep the full grid (profiles/r2_ab_grid_pool_knobs.txt).
    ds.traceGridHalf = cus * 4u;
    if (knobs.tailBelow >= 0) ds.tailBelow = static_cast<uint64_t>(knobs.tailBelow);
    if (knobs.poolSlots != 0) ds.poolSlots = knobs.poolSlots;
    if (knobs.poolGroups != 0) ds.poolGroups = knobs.poolGroups;
    ds.connectOverlap = knobs.connectOverlap != 0;
    // stack entries a ray of this tree can need: one per binary level for the two-box walk, three per level of the wide tree for the
    // four-wide walk (prepareGeometry keeps 3 x depth + 4 within the stack), the root beside an oversize leaf, and a margin
    const uint32_t wideLevels = ps.pg.wideCount > 0u ? ps.pg.wideDepth : 0u;
    const uint32_t stackNeed = std::min<uint32_t>(kTraversalStackDepth, std::max(3u * wideLevels, static_cast<uint32_t>(bvh.maxDepth)) + 4u);
    v.stackLimit = std::max(stackNeed, kLdsStackLevels);
    ds.wideDepth = wideLevels;
    ds.spillLevels = v.stackLimit - kLdsStackLevels;
    ds.spill.ensure(std::max<size_t>(spillWordsPerGroup(ds) * ds.maxPoolGroups() * 2u, 1u));   // a group's k_extend and k_connect may run side by side: an area each
    ds.scalars.ensure(static_cast<size_t>(kScalarCount) * kMaxPoolGroups);
    ds.counters.ensure(kCounterSlots);
    ds.zeros.ensure(16);
    HIP_CHECK(hipMemset(ds.zeros.ptr, 0, 16 * sizeof(uint32_t)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ds.pinnedAlive), sizeof(uint32_t) * (kPinnedHeadsOffset + kItemHeads), hipHostMallocDefault));
    const double copySeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ds.uploadSeconds = ps.seconds + copySeconds;
    ds.timings[0] = ps.geometrySeconds;
    ds.timings[1] = ps.shadingSeconds;
    ds.timings[2] = copySeconds;
    ds.timings[3] = ps.geometryFromCache ? 1.0 : 0.0;
    if (knobs.verboseBuild) std::fprintf(stderr, "[upload] prepare %.2f s, copies to the device %.2f s\n", ps.seconds, copySeconds);
}

}  // namespace ptrhost

namespace {

// ptr_scene_upload and, with the path of a geometry cache file, ptr_scene_upload_prepared
int uploadTo(const char* who, const PtrSceneDesc* scene, const char* cachePath, int device, PtrDeviceScene** outScene, char* err, size_t cap,
             bool dynamic = false, uint32_t dynamicFlags = 0) {
    if (!scene || !outScene) return nullArgument(who, err, cap);
    // The medium stack of the Metal media semantics keeps material ids in 16 bits (csrc/kernels/wavefront.hip mediumWithEntry), and which
    // semantics a render asks for is not known here: a table the ids cannot address is refused for every one of them.
    if (scene->materialCount > kMaxMaterials) return refuse(err, cap, std::string(who) + ": " + tooManyMaterials(scene->materialCount));
    if (ptr_device_count() <= device || device < 0) {
        setErr(err, cap, std::string(who) + ": no such HIP device (the HIP path has no CPU fallback)");
        return 2;
    }
    try {
        auto ds = std::make_unique<PtrDeviceScene>();
        ds->device = device;
        PreparedScene ps;
        prepareScene(*scene, ps, cachePath, dynamic, dynamicFlags);
        uploadScene(*scene, ps, *ds);
        *outScene = ds.release();
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

}  // namespace

std::string ptrhost::dynamicFlagsProblem(uint32_t flags, uint32_t known) {
    if (flags & ~known) return "unknown flag";
    if ((flags & PTR_DYNAMIC_VERTEX_NORMALS) && !(flags & PTR_DYNAMIC_DEFORMABLE)) return "PTR_DYNAMIC_VERTEX_NORMALS needs PTR_DYNAMIC_DEFORMABLE";
    return "";
}

namespace {

// The three uploads of a dynamic scene: `known` is the mask of the PTR_DYNAMIC_* flags the entry point `who` knows
int uploadDynamic(const char* who, uint32_t known, const PtrSceneDesc* scene, int device, uint32_t flags, PtrDeviceScene** out_scene, char* err,
                  size_t err_cap) {
    const std::string problem = dynamicFlagsProblem(flags, known);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    if (scene && out_scene && ptr_device_count() < 1) return noDevice(who, err, err_cap);
    return uploadTo(who, scene, nullptr, device, out_scene, err, err_cap, true, flags);
}

// Camera basis on the host (BuildCamera, EmbreeHeadlessRenderer.mm:150-198).
void buildCamera(const PtrSettings& s, CameraParams& c) {
    constexpr float kPiF = 3.14159265358979323846f;
    const float aspect = s.width > 0 ? static_cast<float>(s.width) / static_cast<float>(s.height) : 1.0f;
    const float vfov = std::min(std::max(s.cameraVerticalFov, 1.0f), 179.0f);
    const float defocus = std::max(s.cameraDefocusAngle, 0.0f);
    const float theta = vfov * (kPiF / 180.0f);
    const float h = std::tan(theta * 0.5f);
    const float viewportHeight = 2.0f * h;
    const float viewportWidth = aspect * viewportHeight;
    const float distance = std::max(s.cameraDistance, 0.1f);
    const float cp = std::cos(s.cameraPitch), sp = std::sin(s.cameraPitch);
    const float cy = std::cos(s.cameraYaw), sy = std::sin(s.cameraYaw);
    const float3 offset{distance * cp * cy, distance * sp, distance * cp * sy};
    const float3 lookAt{s.cameraTarget[0], s.cameraTarget[1], s.cameraTarget[2]};
    const float3 lookFrom = lookAt + offset;
    const float3 w = ptr::normalize(lookFrom - lookAt);
    const float3 u = ptr::normalize(ptr::cross(float3{0.0f, 1.0f, 0.0f}, w));
    const float3 v = ptr::cross(w, u);
    float focus = s.cameraFocusDistance;
    if (focus <= 0.0f) focus = distance;
    const float3 horizontal = (focus * viewportWidth) * u;
    const float3 vertical = (focus * viewportHeight) * v;
    const float3 lowerLeft = ((lookFrom - 0.5f * horizontal) - 0.5f * vertical) - focus * w;
    auto st = [](float* d, const float3& a) {
        d[0] = a.x;
        d[1] = a.y;
        d[2] = a.z;
    };
    st(c.origin, lookFrom);
    st(c.lowerLeft, lowerLeft);
    st(c.horizontal, horizontal);
    st(c.vertical, vertical);
    st(c.u, u);
    st(c.v, v);
    c.lensRadius = focus * std::tan((defocus * 0.5f) * (kPiF / 180.0f));
}

}  // namespace

namespace ptrhost {

// PTR_METAL_ENV_LOD: the mip chain of the scene's environment map by the rule of the material textures (appendTextureWithMips), once per
// device scene and only when a render asks for it: scenes and renders without the bit keep their memory and upload time.  Level 0 stays
// where it is (envRgba); the device gets the chain's record (kernels/texture.h layout, offsets counted from the first texel after it)
// and levels 1...  Returns the milliseconds it took (0 when the chain was there).
double ensureEnvMips(PtrDeviceScene& ds) {
    if (ds.envMipLevels > 0u || ds.view.envRgba == nullptr || ds.view.envWidth == 0u || ds.view.envHeight == 0u) return 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipSetDevice(ds.device));
    const uint32_t w = ds.view.envWidth, h = ds.view.envHeight;
    const size_t level0 = static_cast<size_t>(w) * h;
    std::vector<float> rgba(level0 * 4u);
    HIP_CHECK(hipMemcpy(rgba.data(), ds.view.envRgba, level0 * sizeof(float4), hipMemcpyDeviceToHost));
    const PtrTexture t{rgba.data(), w, h, 0u, 0u, 1u, 0u};   // repeat / repeat, linear
    std::vector<float> chain;
    std::vector<uint32_t> info;
    appendTextureWithMips(t, chain, info);
    const uint32_t levels = info[2];
    for (uint32_t l = 1; l < levels; ++l) info[4 + l] -= static_cast<uint32_t>(level0);   // levels 1.. move down over level 0
    static_assert(kTexInfoWords == 4u * 5u, "texture record layout");
    std::vector<float> upload(kTexInfoWords + (chain.size() - level0 * 4u));
    std::memcpy(upload.data(), info.data(), kTexInfoWords * sizeof(uint32_t));
    std::copy(chain.begin() + static_cast<std::ptrdiff_t>(level0 * 4u), chain.end(), upload.begin() + kTexInfoWords);
    ds.envMips.upload(reinterpret_cast<const float4*>(upload.data()), upload.size() / 4u);
    ds.envMipLevels = levels;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ptr::readKnobs().verboseBuild) std::fprintf(stderr, "[upload] environment mip chain: %ux%u, %u levels, %.2f ms\n", w, h, levels, ms);
    return ms;
}

void fillRenderParams(const PtrSettings& s, uint32_t spp, RenderParams& rp) {
    std::memset(&rp, 0, sizeof(rp));
    buildCamera(s, rp.cam);
    rp.width = s.width;
    rp.byWidth = makeDivU32(s.width);
    rp.height = s.height;
    rp.maxDepth = std::min(s.maxDepth, kFlagFieldMask);
    rp.shadowSlack = (s.debugShadowSlack > 0.0f && s.debugShadowSlack < 1.0f) ? s.debugShadowSlack : 0.0f;
    rp.seedBase = s.seed != 0 ? s.seed : 0x9e3779b9u;
    rp.spp = std::max(1u, spp);
    rp.sampleBase = 0u;
    rp.sppTotal = rp.spp;
    rp.passFlags = 3u;   // one pass: first and last
    rp.enableRussianRoulette = s.enableRussianRoulette;
    rp.enableSpecularNee = s.enableSpecularNee;
    rp.enableMnee = s.enableMnee;
    rp.enableMneeSecondary = s.enableMneeSecondary;
    rp.backgroundMode = s.backgroundMode;
    std::memcpy(rp.backgroundColor, s.backgroundColor, sizeof(rp.backgroundColor));
    rp.envRotation = s.environmentRotation;
    rp.envIntensity = s.environmentIntensity;
    rp.clampFactor = std::max(s.fireflyClampFactor, 0.0f);   // MakeFireflyParams, :381-391
    rp.clampFloor = std::max(s.fireflyClampFloor, 0.0f);
    rp.throughputClamp = std::max(s.throughputClamp, 0.0f);
    rp.tailClampBase = std::max(s.specularTailClampBase, 0.0f);
    rp.tailClampRoughnessScale = std::max(s.specularTailClampRoughnessScale, 0.0f);
    rp.minSpecularPdf = std::max(s.minSpecularPdf, 1.0e-8f);
    rp.clampEnabled = s.fireflyClampEnabled ? 1.0f : 0.0f;
    rp.emissionScale = (s.emissionScale > 0.0f && std::isfinite(s.emissionScale)) ? s.emissionScale : 1.0f;
    rp.mediaMode = s.metalSemantics & (PTR_METAL_MEDIA | PTR_METAL_THIN | PTR_METAL_FACE_NORMAL | PTR_METAL_SPECULAR | PTR_METAL_SSS | PTR_METAL_PBR |
                                       PTR_METAL_CLAMPS | PTR_METAL_ENV_LOD | PTR_METAL_RAY_DIFF);
    rp.clampMaxContribution = std::max(s.fireflyClampMaxContribution, 0.0f);   // make_firefly_params, pathtrace.metal:3545
    rp.minSpecularPdfRaw = s.minSpecularPdf;
    rp.sssMode = s.sssMode;
    rp.sssMaxSteps = std::max(s.sssMaxSteps, 1u);
}

// Launch configuration of the one-off traversal kernels (ray batches, AOVs, debug queries): whole grid, group 0's heads and spill area
LaunchConfig coldLaunchConfig(const PtrDeviceScene& ds) { return LaunchConfig{ds.traceGrid, ds.spill.ptr, ds.scalars.ptr + 1, ds.refillBelow}; }

void downloadFirstHit(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t sample, DeviceBuffer<float4>& albedo, DeviceBuffer<float4>& normal,
                      float* outAlbedo, float* outNormal) {
    RenderParams rp;
    fillRenderParams(settings, 1u, rp);
    const size_t pixels = static_cast<size_t>(settings.width) * settings.height;
    albedo.ensure(pixels);
    normal.ensure(pixels);
    launchAovs(rp, ds.view, sample, albedo.ptr, normal.ptr, coldLaunchConfig(ds), nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (outAlbedo) albedo.download(reinterpret_cast<float4*>(outAlbedo), pixels);
    if (outNormal) normal.download(reinterpret_cast<float4*>(outNormal), pixels);
}

// Local pixel order of a partition: its PTR_BAND_ROWS-row bands top to bottom, each walked in 8x8 blocks so the
// 64 lanes of a wave start with a compact, coherent bundle of primary rays.
void partitionPixels(uint32_t width, uint32_t height, uint32_t part, uint32_t parts, std::vector<uint32_t>& out) {
    out.clear();
    const uint32_t bands = (height + PTR_BAND_ROWS - 1u) / PTR_BAND_ROWS;
    for (uint32_t b = part; b < bands; b += parts) {
        const uint32_t y0 = b * PTR_BAND_ROWS, y1 = std::min(y0 + PTR_BAND_ROWS, height);
        for (uint32_t ty = y0; ty < y1; ty += 8u) {
            for (uint32_t tx = 0; tx < width; tx += 8u) {
                for (uint32_t y = ty; y < std::min(ty + 8u, y1); ++y) {
                    for (uint32_t x = tx; x < std::min(tx + 8u, width); ++x) out.push_back(y * width + x);
                }
            }
        }
    }
}

ptr::CullRect passCullRect(const ptr::WorldBounds& world, const PtrSettings& settings, bool covariance, int mode) {
    // (the counting build's counters mirror the reference's rays, camera rays that miss included; at maxDepth 0 a frame adds nothing,
    // not even the background; mode bit 2: the caller reads the pass's accumulators and wants every pixel's)
    if (!ptr::readKnobs().backgroundCull || covariance || (mode & 5) != 0 || settings.width == 0u || settings.height == 0u) return ptr::CullRect{};
    RenderParams rp;
    fillRenderParams(settings, 1u, rp);
    if (rp.maxDepth == 0u) return ptr::CullRect{};
    const CameraParams& c = rp.cam;
    return ptr::backgroundCullRect(ptr::CullCamera{c.origin, c.lowerLeft, c.horizontal, c.vertical, c.u, c.v, c.lensRadius}, settings.width,
                                   settings.height, world);
}

// Adds the per-launch figures of `b` to `a`: kernel times, k_extend launches, samples.
void addLaunchStats(PtrRenderStats& a, const PtrRenderStats& b) {
    a.traceKernelMs += b.traceKernelMs;
    a.shadeKernelMs += b.shadeKernelMs;
    a.shadowKernelMs += b.shadowKernelMs;
    a.tailKernelMs += b.tailKernelMs;
    a.traceLaunches += b.traceLaunches;
    a.samples += b.samples;
}

}  // namespace ptrhost

namespace {

// Bytes the per-sample accumulators of one pass may take: a quarter of the device's TOTAL memory, at most 16 GiB.  Taken
// from the device's size, never from what happens to be free: every rank of a multi-GPU render has to split a frame
// into the same passes (k_resolve adds the per-pass sums in pass order), whatever else lives on its card.
uint64_t itemBudgetBytes(const PtrDeviceScene& ds) {
    return std::max<uint64_t>(64ull << 20, std::min<uint64_t>(16ull << 30, ds.deviceTotalBytes / 4u));
}

// optional per-slot arrays: the ray cone of textured paths, the environment LOD of PTR_METAL_ENV_LOD with an environment map
bool conePaths(const PtrDeviceScene& ds, const RenderParams& rp) { return (rp.mediaMode & PTR_METAL_PBR) && ds.view.textureCount > 0u; }
bool envLodPaths(const PtrDeviceScene& ds, const RenderParams& rp) { return (rp.mediaMode & PTR_METAL_ENV_LOD) && ds.view.envWidth > 0u; }

// Grows the buffers of a pool of `slots` path slots (and the frame's per-item ones) to this pass; slotRange lays them out.
void sizeSlots(PtrDeviceScene& ds, const RenderParams& rp, bool count, uint32_t slots) {
    ds.state.ensure(static_cast<size_t>(slots) * 4u);
    ds.hit.ensure(slots);
    ds.flushItem.ensure(slots);
    if (count) ds.signature.ensure(slots);
    if (ds.tailBelow > 0) {
        ds.tailList.ensure(slots);
        ds.tailWords.ensure(4);
    }
    ds.itemAccum.ensure(rp.itemCount);
    ds.recBuf.ensure(static_cast<size_t>(slots) * kRecSlots * 4u);
    ds.itemReserve.ensure((slots + 63u) / 64u);
    if (rp.mediaMode & PTR_METAL_MEDIA) ds.medium.ensure(slots);
    if (conePaths(ds, rp)) ds.cone.ensure(slots);
    if (envLodPaths(ds, rp)) {   // the chain (first such render of the scene) and the paths' LOD
        ensureEnvMips(ds);
        ds.envLod.ensure(slots);
    }
    ds.itemHeads.ensure(kItemHeadWords);
}

// Slots [first, first + n) of the pool of `slots` slots that sizeSlots grew, and in `env` their environment LOD (all null without it).
// The shared fields (work heads, item sums, pixel map, counters) are not offset.  The connect and busy lists stay null: a group sets
// its own, and the whole pool ([0, slots): the tail kernels' view) probes the slots.
PathPool slotRange(const PtrDeviceScene& ds, const RenderParams& rp, bool count, uint32_t slots, uint32_t first, uint32_t n, EnvLodView& env) {
    PathPool p;
    std::memset(&p, 0, sizeof(p));
    float4* state = ds.state.ptr + first;
    p.ray0 = state;
    p.ray1 = state + slots;
    p.thr = state + 2ull * slots;
    p.accum = state + 3ull * slots;
    p.hit = ds.hit.ptr + first;
    p.flushItem = ds.flushItem.ptr + first;
    p.signature = count ? ds.signature.ptr + first : nullptr;
    p.medium = (rp.mediaMode & PTR_METAL_MEDIA) ? ds.medium.ptr + first : nullptr;
    p.cone = conePaths(ds, rp) ? ds.cone.ptr + first : nullptr;
    for (uint32_t k = 0; k < kRecSlots; ++k) {
        float4* base = ds.recBuf.ptr + static_cast<size_t>(k) * 4u * slots + first;
        p.rec[k] = ShadowRecordView{base, base + slots, base + 2ull * slots, base + 3ull * slots};
    }
    p.itemReserve = ds.itemReserve.ptr + first / 64u;
    p.slots = n;
    p.recStride = slots;
    p.itemAccum = ds.itemAccum.ptr;
    p.nextItem = ds.itemHeads.ptr;
    p.pixelOfLocal = ds.pixelOfLocal.ptr;
    p.counters = ds.counters.ptr;
    p.zero = reinterpret_cast<const float4*>(ds.zeros.ptr);
    env = EnvLodView{};
    if (envLodPaths(ds, rp)) env = EnvLodView{ds.envMips.ptr, ds.envLod.ptr + first, ds.envMipLevels, 0u};
    return p;
}

constexpr size_t kConnectCountWords = static_cast<size_t>(kConnectQueues) * kConnectCountStride;   // one set of sub-list counters

// One group of the pool, driven through extend -> shade -> connect on its own stream (see makeGroups).
struct PoolGroup {
    PathPool pool;
    EnvLodView env;
    LaunchConfig cfg;
    hipStream_t stream;
    hipStream_t side = nullptr;   // k_connect's stream when it runs beside the next k_extend (null: on `stream`)
    hipEvent_t shadeDone = nullptr, connectDone = nullptr;   // (with `side`) this iteration's k_shade / k_connect done
    uint32_t* sideSpill = nullptr;   // (with `side`) spill area of k_connect
    uint32_t* scalars;
    bool done = false;
    uint32_t feederChunk;   // slots per work-head atomic; grows as the group drains at the end of the frame
    size_t listWords;       // words of one connect or busy list
    uint32_t* connectCounts;   // two sets of sub-list counters, used in turn
    // busy lists (end of the frame): two lists and three counter sets in rotation.  busyStage 0: the kernels walk the slots;
    // 1: this iteration's k_shade (still walking the slots) fills the first list; 2: k_extend and k_shade walk the list of the
    // previous iteration and k_shade fills the next one
    uint32_t *busyLists, *busyCounts;
    uint32_t busyStage = 0, busyTurn = 0;
    bool shadeListed = false;

    // The lists and counters of iteration `iteration`: the connect counters by its parity (k_shade clears the set of the next one);
    // once the queue is dry, the busy lists move on by one turn per iteration.
    void selectLists(uint64_t iteration, bool queueDry) {
        pool.connectCount = connectCounts + kConnectCountWords * (iteration & 1u);
        pool.connectClear = connectCounts + kConnectCountWords * ((iteration + 1u) & 1u);
        if (busyStage != 0u) {   // the previous iteration's k_shade filled list busyTurn: walk it
            busyStage = 2u;
            ++busyTurn;
        }
        if (queueDry && busyStage == 0u) busyStage = 1u;   // the kernels decide per launch whether a list pays
        if (busyStage == 0u) return;
        // k_shade fills list `busyTurn` (counter set busyTurn % 3) and clears the set after it; in stage 2 this iteration's
        // k_extend and k_shade walk the list the previous iteration filled
        pool.busyOut = busyLists + listWords * (busyTurn & 1u);
        pool.busyCountOut = busyCounts + kConnectCountWords * (busyTurn % 3u);
        pool.busyCountClear = busyCounts + kConnectCountWords * ((busyTurn + 1u) % 3u);
        if (busyStage == 2u) {
            pool.busyIn = busyLists + listWords * ((busyTurn + 1u) & 1u);
            pool.busyCountIn = busyCounts + kConnectCountWords * ((busyTurn + 2u) % 3u);
        }
    }

    // A poll with the queue dry found `live` live slots in the group (baseChunk: the feeder chunk of a full pool).
    void polledDry(uint32_t live, uint32_t baseChunk) {
        if (live == 0u) done = true;
        // the fewer live slots, the bigger the chunks the work list is claimed in (see WaveFeeder): a chunk
        // should still hold about as many live slots as a full one does when the pool is full
        // up to the point where the static first chunks of the resident waves cover the whole list and
        // the head is not touched at all
        const uint32_t thin = pool.slots / std::max(live, 1u);
        const uint32_t waves = std::max(cfg.traceGrid * (kTraceGridUnit / 64u), 1u);
        const uint32_t perWave = ((pool.slots + waves - 1u) / waves + 63u) / 64u * 64u;
        const uint32_t cap = std::max(perWave, baseChunk);
        feederChunk = std::min(cap, baseChunk * std::max(thin, 1u));
        shadeListed = static_cast<uint64_t>(live) * 5u < static_cast<uint64_t>(pool.slots) * 2u;   // < 40 % live
    }
};

// Streams and events of `groupCount` groups (group 0 runs on the caller's stream), with `overlap` a side stream and two events each.
void ensureGroupStreams(PtrDeviceScene& ds, uint32_t groupCount, bool overlap) {
    auto newStream = [] { hipStream_t st; HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); return st; };
    auto newEvent = [] { hipEvent_t e; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return e; };
    while (ds.groupStreams.size() + 1 < groupCount) ds.groupStreams.push_back(newStream());
    while (ds.groupEvents.size() < groupCount + 1) ds.groupEvents.push_back(newEvent());
    while (overlap && ds.sideStreams.size() < groupCount) {
        ds.sideStreams.push_back(newStream());
        ds.sideEvents.push_back(newEvent());
        ds.sideEvents.push_back(newEvent());
    }
}

// The pool is cut into independent groups, each driven through extend -> shade -> connect on its own HIP
// stream.  Every launch of the persistent traversal kernels ends with a drain phase (the last rays of the
// last chunks, few lanes busy); with two groups in flight the other group's kernels fill the CUs a draining
// kernel leaves idle.  Groups share only the work-item head (one atomic per 64 items), so results do not
// depend on how they interleave.
std::vector<PoolGroup> makeGroups(PtrDeviceScene& ds, const RenderParams& rp, bool count, bool soloGroup, uint32_t slots, hipStream_t stream) {
    const uint32_t wantGroups = ds.poolGroups ? ds.poolGroups : (slots > (8u << 20) ? 2u : 4u);
    uint32_t groupCount = std::min<uint32_t>(soloGroup ? 1u : wantGroups, std::max<uint32_t>(1u, slots >> 20));   // >= 1 Mi slots per group
    const uint32_t groupSlots = ((slots + groupCount - 1u) / groupCount + 255u) & ~255u;
    groupCount = (slots + groupSlots - 1u) / groupSlots;
    // k_connect beside the next k_extend: only while the streams fit the hardware queues (two groups at most), and never in a solo
    // render, whose point is kernels that do not overlap
    const bool overlap = ds.connectOverlap && !soloGroup && groupCount <= 2u;
    ensureGroupStreams(ds, groupCount, overlap);
    const size_t spillWords = spillWordsPerGroup(ds);
    // connect lists: sub-list w % 64 takes the entries of k_shade's wave w, at most 64 each
    const uint32_t connectRegion = ((groupSlots + 63u) / 64u + kConnectQueues - 1u) / kConnectQueues * 64u;
    const size_t connectListWords = static_cast<size_t>(connectRegion) * kConnectQueues;
    if (slots >= (1u << kConnectMaskShift)) throw HipError{"path-slot pool too large for the connect lists"};   // (the pool is capped at 64 Mi slots)
    ds.connectList.ensure(connectListWords * groupCount);
    ds.connectCounts.ensure(kConnectCountWords * 2u * kMaxPoolGroups);
    ds.busyLists.ensure(connectListWords * 2u * groupCount);
    ds.busyCounts.ensure(kConnectCountWords * 3u * kMaxPoolGroups);
    std::vector<PoolGroup> groups(groupCount);
    for (uint32_t g = 0; g < groupCount; ++g) {
        PoolGroup& gr = groups[g];
        const uint32_t first = g * groupSlots;
        gr.pool = slotRange(ds, rp, count, slots, first, std::min(groupSlots, slots - first), gr.env);
        gr.pool.connectList = ds.connectList.ptr + connectListWords * g;
        gr.pool.connectRegion = connectRegion;
        gr.listWords = connectListWords;
        gr.connectCounts = ds.connectCounts.ptr + kConnectCountWords * 2u * g;
        gr.busyLists = ds.busyLists.ptr + connectListWords * 2u * g;
        gr.busyCounts = ds.busyCounts.ptr + kConnectCountWords * 3u * g;
        gr.scalars = ds.scalars.ptr + static_cast<size_t>(g) * kScalarCount;
        const bool sideBySide = groupCount > 1 && gr.pool.slots >= kHalfGridGroupSlots;
        gr.cfg = LaunchConfig{sideBySide ? ds.traceGridHalf : ds.traceGrid, ds.spill.ptr + g * spillWords, gr.scalars + 1, ds.refillBelow};
        gr.stream = g == 0 ? stream : ds.groupStreams[g - 1];
        gr.feederChunk = ds.feederChunk;
        if (overlap) {
            gr.side = ds.sideStreams[g];
            gr.shadeDone = ds.sideEvents[2 * g];
            gr.connectDone = ds.sideEvents[2 * g + 1];
            gr.sideSpill = ds.spill.ptr + (ds.maxPoolGroups() + g) * spillWords;
        }
    }
    return groups;
}

// first index of work-item range k (its head's value before any claim)
uint64_t itemRangeStart(const RenderParams& rp, uint32_t k) {
    return std::min<uint64_t>(static_cast<uint64_t>(rp.itemHeadFirst) + static_cast<uint64_t>(k) * rp.itemsPerHead, rp.itemCount);
}

// Phase 1: while unclaimed work items remain nobody needs to count survivors; the host looks at the item head
// only when it expects it to be nearly exhausted (items are claimed at a steady rate, so after the first look the
// next one is scheduled at 3/4 of the predicted remaining iterations).  Phase 2 (queue dry): k_shade counts live
// slots and every group is polled every 4 iterations until it has none left (k_extend reports how many live
// slots it traced: one atomic per persistent wave).  A poll joins all streams, which
// costs the overlap between groups once; polling every 4 iterations throughout was 5 % slower.  (Polling through
// events without joining was tried: the host then runs up to a dozen empty iterations past the end - no gain.)
constexpr uint64_t kPollEvery = 4;
constexpr uint64_t kPollDry = 2;   // once the queue is dry: how often the live slots are counted (the hand-over to the tail kernels hangs on it)

// allDone: no group has a live slot left; runTail: the last paths go to the tail kernels; queueDry: every work item is claimed;
// nextCheck: the iteration of the next poll
struct PollResult {
    bool allDone, runTail, queueDry;
    uint64_t nextCheck;
};

// A poll after `iterations` iterations: the range heads (queue not dry) or the groups' live-slot counts are copied to the host, the
// streams joined, and the groups updated.
PollResult poll(PtrDeviceScene& ds, std::vector<PoolGroup>& groups, const RenderParams& rp, uint32_t slots, uint64_t iterations, bool queueDry,
                bool tracePolls) {
    HIP_CHECK(hipGetLastError());   // a launch that failed (bad configuration, out of resources) must not pass for a slow frame
    const uint32_t ring = static_cast<uint32_t>((iterations - 1u) % kAliveRing);   // the live-slot counters of the last iteration
    bool headsCopied = false;
    for (uint32_t g = 0; g < groups.size(); ++g) {
        PoolGroup& gr = groups[g];
        if (gr.done) continue;
        if (queueDry) {
            HIP_CHECK(hipMemcpyAsync(ds.pinnedAlive + g, gr.scalars + kAliveBase + ring, sizeof(uint32_t), hipMemcpyDeviceToHost, gr.stream));
        } else if (!headsCopied) {
            HIP_CHECK(hipMemcpy2DAsync(ds.pinnedAlive + kPinnedHeadsOffset, sizeof(uint32_t), ds.itemHeads.ptr, sizeof(uint32_t) * kItemHeadStride,
                                       sizeof(uint32_t), kItemHeads, hipMemcpyDeviceToHost, gr.stream));
            headsCopied = true;
        }
    }
    PollResult r{true, false, queueDry, 0};
    uint64_t live = 0;
    for (uint32_t g = 0; g < groups.size(); ++g) {
        PoolGroup& gr = groups[g];
        if (gr.done) continue;
        HIP_CHECK(hipStreamSynchronize(gr.stream));
        if (queueDry) {
            if (tracePolls) {
                std::fprintf(stderr, "[poll] iteration %llu group %u live %u of %u chunk %u\n", static_cast<unsigned long long>(iterations), g,
                             ds.pinnedAlive[g], gr.pool.slots, gr.feederChunk);
            }
            gr.polledDry(ds.pinnedAlive[g], ds.feederChunk);
            if (!gr.done) live += ds.pinnedAlive[g];
        }
        r.allDone = r.allDone && gr.done;
    }
    if (queueDry && !r.allDone && ds.tailBelow > 0 && live <= ds.tailBelow) r.runTail = true;
    if (r.allDone || r.runTail) return r;
    r.nextCheck = iterations + (queueDry && ds.tailBelow > 0 ? kPollDry : kPollEvery);
    if (!queueDry) {
        uint64_t head = slots;   // items claimed so far = pre-assigned + what every range head has handed out
        const uint32_t* heads = ds.pinnedAlive + kPinnedHeadsOffset;
        for (uint32_t k = 0; k < kItemHeads; ++k) {
            const uint64_t lo = itemRangeStart(rp, k);
            const uint64_t hi = std::min<uint64_t>(lo + rp.itemsPerHead, rp.itemCount);
            head += std::min<uint64_t>(std::max<uint64_t>(heads[k], lo), hi) - lo;
        }
        if (head >= rp.itemCount) {
            r.queueDry = true;
        } else if (head > slots) {
            const double perIteration = static_cast<double>(head - slots) / static_cast<double>(iterations);
            const double left = static_cast<double>(rp.itemCount - head) / std::max(perIteration, 1.0);
            r.nextCheck = iterations + std::max<uint64_t>(kPollEvery, static_cast<uint64_t>(left * 0.75));
        }
    }
    return r;
}

enum class SpanKind : int { Extend = 0, Shade = 1, Connect = 2, Tail = 3, ResolveCov = 4, Background = 5 };   // the `kind` of a [launch] line

// Start and end events around the launches of a timed pass.
struct LaunchTimer {
    struct Span {
        hipEvent_t a, b;   // null until created
        SpanKind kind;
        const void* stream;
    };
    bool on = false;
    std::vector<Span> spans;
    ~LaunchTimer() {
        for (const Span& s : spans) {
            for (hipEvent_t e : {s.a, s.b}) if (e) (void)hipEventDestroy(e);
        }
    }
    template <typename F>
    void launch(SpanKind kind, hipStream_t st, F&& fn) {
        if (!on) {
            fn();
            return;
        }
        spans.push_back(Span{nullptr, nullptr, kind, st});
        Span& s = spans.back();
        HIP_CHECK(hipEventCreate(&s.a));
        HIP_CHECK(hipEventCreate(&s.b));
        HIP_CHECK(hipEventRecord(s.a, st));
        fn();
        HIP_CHECK(hipEventRecord(s.b, st));
    }
};

// The figures of a finished pass: wall time, kernel times from the launch spans, the counters of a counting pass, and the
// PTR_VERBOSE=launches / steps reports (tools/launch_timeline.py and tools/steps_probe.py parse them).
void passStats(const PtrDeviceScene& ds, const RenderParams& rp, const std::vector<LaunchTimer::Span>& spans, bool count, const ptr::Knobs& knobs,
               double seconds, PtrRenderStats& stats) {
    std::memset(&stats, 0, sizeof(stats));
    stats.totalSeconds = seconds;
    stats.avgMsPerSample = seconds * 1000.0 / rp.spp;
    stats.uploadSeconds = ds.uploadSeconds;
    stats.samples = static_cast<uint64_t>(rp.localPixels) * rp.spp;
    if (knobs.verboseLaunches && !spans.empty()) {   // debugging aid: when each launch ran (ms from the first)
        for (const LaunchTimer::Span& s : spans) {
            float t0 = 0.0f, t1 = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&t0, spans.front().a, s.a));
            HIP_CHECK(hipEventElapsedTime(&t1, spans.front().a, s.b));
            std::fprintf(stderr, "[launch] kind %d  start %.3f  end %.3f  (%.3f ms)  stream %p\n", static_cast<int>(s.kind), t0, t1, t1 - t0, s.stream);
        }
    }
    for (const LaunchTimer::Span& s : spans) {
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, s.a, s.b));
        switch (s.kind) {
            case SpanKind::Extend: stats.traceKernelMs += ms; ++stats.traceLaunches; break;
            case SpanKind::Shade: stats.shadeKernelMs += ms; break;
            case SpanKind::Connect: stats.shadowKernelMs += ms; break;
            case SpanKind::Tail: stats.tailKernelMs += ms; break;
            case SpanKind::ResolveCov: break;   // (PTR_VERBOSE=launches shows it: tools/cov_cost.py)
            case SpanKind::Background: break;   // (likewise: k_background runs beside the loop's first launches)
        }
    }
    if (!count) return;
    uint64_t c[kCounterSlots];
    HIP_CHECK(hipMemcpy(c, ds.counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    stats.primaryRays = c[kCntPrimaryRays];
    stats.extendRays = c[kCntExtendRays];
    stats.shadowRays = c[kCntShadowRays];
    stats.extendNodesVisited = c[kCntExtendNodes];
    stats.extendLeafPrimTests = c[kCntExtendPrims];
    stats.nodesVisited = c[kCntExtendNodes] + c[kCntShadowNodes];
    stats.leafPrimTests = c[kCntExtendPrims] + c[kCntShadowPrims];
    stats.shadedHits = c[kCntShadedHits];
    stats.triangleHits = c[kCntTriangleHits];
    stats.shadowEarlyExits = c[kCntShadowEarlyExit];
    if (!knobs.verboseSteps) return;
    // lane utilisation of k_extend's step loop (counting build)
    const double nodeLanes = static_cast<double>(c[kCntExtendNodes] - c[kCntExtendLeaves]), primLanes = static_cast<double>(c[kCntExtendPrims]);
    const double nodeSlots = static_cast<double>(c[kCntExtendWaveNodeSteps]), primSlots = static_cast<double>(c[kCntExtendWavePrimSteps]);
    std::fprintf(stderr, "[steps] k_extend: %.3g rays; node steps %.3g lane / %.3g slots = %.3f; prim steps %.3g lane / %.3g slots = %.3f; "
                         "refill passes %.3g (x64 lanes)\n",
                 static_cast<double>(c[kCntExtendRays]), nodeLanes, nodeSlots, nodeLanes / std::max(nodeSlots, 1.0), primLanes, primSlots,
                 primLanes / std::max(primSlots, 1.0), static_cast<double>(c[kCntExtendRefillPasses]));
    const double votes = static_cast<double>(c[kCntExtendVoteIterations]) / 64.0;
    std::fprintf(stderr, "[steps] k_extend: %.3g vote iterations; lanes holding a ray %.1f / 64 on average, of which at a leaf %.1f\n", votes,
                 static_cast<double>(c[kCntExtendActiveLanes]) / std::max(votes, 1.0), static_cast<double>(c[kCntExtendLeafLanes]) / std::max(votes, 1.0));
    const double shadeLanes = std::max(static_cast<double>(c[kCntShadeWaves]), 1.0);
    std::fprintf(stderr, "[steps] k_shade: %.3g wave visits; share of their lanes at each stage: ray traced %.3f, surface hit %.3f, of which a light "
                         "%.3f; light sample evaluated %.3f, tested against the light's own triangles %.3f, shadow ray queued %.3f; BSDF sampled "
                         "%.3f; new work item wanted %.3f\n",
                 shadeLanes / 64.0, c[kCntShadeAlive] / shadeLanes, c[kCntShadeSurface] / shadeLanes, c[kCntShadeEmitter] / shadeLanes,
                 c[kCntShadeLightEval] / shadeLanes, c[kCntShadeLightPretest] / shadeLanes, c[kCntShadeLightStored] / shadeLanes,
                 c[kCntShadeBsdfSample] / shadeLanes, c[kCntShadeNeedItem] / shadeLanes);
    static const char* names[kShadeParts] = {"loads + landing", "background", "surface reconstruction", "emitter", "light sample", "env sample",
                                             "BSDF sample + next ray", "work item + camera ray", "stores + lists", "subsurface walk"};
    double waveTotal = 0.0;
    for (uint32_t k = 0; k < kShadeParts; ++k) waveTotal += static_cast<double>(c[kCntShadeWaveTicks + k]);
    std::fprintf(stderr, "[steps] k_shade parts (clock ticks between the part's first and last instruction, waits included): share of the waves' time | lanes busy\n");
    for (uint32_t k = 0; k < kShadeParts; ++k) {
        const double wave = static_cast<double>(c[kCntShadeWaveTicks + k]), lane = static_cast<double>(c[kCntShadeLaneTicks + k]);
        if (wave <= 0.0) continue;
        std::fprintf(stderr, "[steps]   %-24s %5.1f %% | %.3f\n", names[k], 100.0 * wave / std::max(waveTotal, 1.0), lane / (64.0 * wave));
    }
    std::fprintf(stderr, "[steps] k_extend: refill passes take %.1f %% of the waves' time in the kernel\n",
                 100.0 * static_cast<double>(c[kCntExtendRefillTicks]) / std::max(static_cast<double>(c[kCntExtendWaveTicks]), 1.0));
}

// The pixels of a pass that k_background resolves beside the traced ones (none: count 0)
struct BackgroundPixels {
    const uint32_t* pixels = nullptr;
    uint32_t count = 0, parts = 1;
    float* out = nullptr;
};

template <typename Resolve>
void tracePass(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t sampleBase, uint32_t sppTotal, uint32_t passFlags,
               const uint32_t* dPixelOfLocal, uint32_t localPixels, hipStream_t stream, int mode, PtrRenderStats* stats, Resolve&& resolve,
               const BackgroundPixels& background = BackgroundPixels{}, const ptrhost::IterationHook* hook = nullptr);

// One pass over `spp` samples per pixel starting at sample `sampleBase` of a frame of `sppTotal`; passFlags bit 0 = first pass of
// the frame (output and counters start from zero), bit 1 = last pass (the running sum in dOut is divided by sppTotal).
// (renderBands has checked the size and the partition, and selected the device.)
// dCov (nullable; include/ptr_stats.h): six floats per pixel in the band layout of dOut, the covariance of the pixel mean.
void renderPass(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t sampleBase, uint32_t sppTotal, uint32_t passFlags,
                uint32_t part, uint32_t parts, float* dOut, float* dCov, hipStream_t stream, int mode, PtrRenderStats* stats) {
    // Pixels whose camera rays cannot reach the scene stay out of the pool: k_background resolves them (csrc/host/background_cull.h).
    // The rectangle is part of the cache key: camera and bounds may change between two calls on one scene handle.
    const ptr::CullRect cull = ptrhost::passCullRect(ds.worldBounds, settings, dCov != nullptr, mode);
    if (ds.cachedW != settings.width || ds.cachedH != settings.height || ds.cachedPart != part || ds.cachedParts != parts || !(ds.cachedCull == cull)) {
        std::vector<uint32_t> pixels, background;
        partitionPixels(settings.width, settings.height, part, parts, pixels);
        if (cull.cull) {   // split, order kept
            size_t kept = 0;
            for (const uint32_t pixel : pixels) {
                if (cull.inside(pixel % settings.width, pixel / settings.width)) pixels[kept++] = pixel;
                else background.push_back(pixel);
            }
            pixels.resize(kept);
        }
        ds.pixelOfLocal.upload(pixels.data(), pixels.size());
        ds.backgroundPixels.upload(background.data(), background.size());
        ds.cachedW = settings.width;
        ds.cachedH = settings.height;
        ds.cachedPart = part;
        ds.cachedParts = parts;
        ds.cachedCull = cull;
        ds.cachedLocalPixels = static_cast<uint32_t>(pixels.size());
        ds.cachedBackgroundPixels = static_cast<uint32_t>(background.size());
    }
    const uint32_t localPixels = ds.cachedLocalPixels;
    const BackgroundPixels background{ds.backgroundPixels.ptr, ds.cachedBackgroundPixels, parts, dOut};
    const uint32_t bandCount = ptr_part_band_count(settings.height, part, parts);
    const size_t outFloats = static_cast<size_t>(bandCount) * PTR_BAND_ROWS * settings.width * 3u;
    if (passFlags & 1u) HIP_CHECK(hipMemsetAsync(dOut, 0, outFloats * sizeof(float), stream));
    if (dCov && (passFlags & 1u)) HIP_CHECK(hipMemsetAsync(dCov, 0, outFloats * 2u * sizeof(float), stream));
    if (localPixels == 0) {
        const auto wall0 = std::chrono::steady_clock::now();
        if (background.count > 0u) {   // every pixel of the partition was culled: the background kernel is the whole pass
            RenderParams rp;
            fillRenderParams(settings, spp, rp);
            rp.sampleBase = sampleBase;
            rp.sppTotal = std::max(1u, sppTotal);
            rp.passFlags = passFlags;
            launchBackground(rp, ds.view, background.pixels, background.count, parts, dOut, stream);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        if (stats && background.count > 0u) {
            std::memset(stats, 0, sizeof(*stats));
            stats->totalSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
            stats->avgMsPerSample = stats->totalSeconds * 1000.0 / std::max(1u, spp);
            stats->uploadSeconds = ds.uploadSeconds;
            stats->samples = static_cast<uint64_t>(background.count) * std::max(1u, spp);
        }
        return;
    }
    tracePass(ds, settings, spp, sampleBase, sppTotal, passFlags, ds.pixelOfLocal.ptr, localPixels, stream, mode, stats,
              [&](const RenderParams& rp, const PathPool& pool, LaunchTimer& timer) {
                  launchResolve(rp, pool, parts, dOut, stream);
                  if (dCov) {
                      ds.covMean.ensure(localPixels);
                      timer.launch(SpanKind::ResolveCov, stream, [&] { launchResolveCov(rp, pool, parts, ds.covMean.ptr, dCov, stream); });
                  }
              },
              background);
    if (stats) stats->samples += static_cast<uint64_t>(background.count) * std::max(1u, spp);   // resolved like the traced ones
}

// The part of a pass that traces its work items: from the parameter set-up through the end-of-frame kernels, then `resolve` (what
// reads the per-sample accumulators: see renderPass), the stream joined and the figures of the pass.  dPixelOfLocal: the image pixel
// of each of the pass's `localPixels` (> 0) local pixels, on the device.
// `background`: pixels the pool never sees; k_background writes them on `stream` while the other groups' first launches run.
// `hook`: null in every render; the stepping probe's (ptr_debug_path_states), called after the launches of every iteration.
template <typename Resolve>
void tracePass(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t sampleBase, uint32_t sppTotal, uint32_t passFlags,
               const uint32_t* dPixelOfLocal, uint32_t localPixels, hipStream_t stream, int mode, PtrRenderStats* stats, Resolve&& resolve,
               const BackgroundPixels& background, const ptrhost::IterationHook* hook) {
    const bool count = (mode & 1) != 0;         // counting instantiation of the kernels
    const bool soloGroup = (mode & 2) != 0;     // one pool group: kernels run alone, for clean per-kernel timings

    RenderParams rp;
    fillRenderParams(settings, spp, rp);
    rp.sampleBase = sampleBase;
    rp.sppTotal = std::max(1u, sppTotal);
    rp.passFlags = passFlags;

    // Work items = single pixel samples: item w = sample * localPixels + localPixel.  Slots claim items from 64 range heads,
    // so the pool stays full until the last items regardless of how path length varies over the image.  (Items of C > 1
    // consecutive samples lengthen the end of the frame - once the queue is dry every slot still finishes its item, C = 4
    // cost 12 % on config 2 - so a frame whose per-sample accumulators do not fit is rendered in passes instead, see
    // renderBands.)
    rp.localPixels = localPixels;
    rp.byLocalPixels = makeDivU32(localPixels);
    const uint64_t itemCount64 = static_cast<uint64_t>(localPixels) * rp.spp;
    if (itemCount64 > 0xFFFF0000ull) throw HipError{"too many work items for one pass (reduce spp or resolution)"};
    rp.itemCount = static_cast<uint32_t>(itemCount64);
    // enough to keep every CU's wave slots full several times over - but never more than half the work items: a pool as
    // large as the frame is all ramp-up and drain (config 1, 16.8 M samples: 16 Mi slots 16.2 ms, 8 Mi slots 10.0 ms)
    // (32 Mi slots at most: a larger pool gives every launch more rays before its tail - config 2 +4.5 %, config 4 +2 %, config 5 +8 %
    // against 16 Mi - and since the lists made the end of the frame cheap it costs the partitions of a multi-GPU frame nothing:
    // one rank of eight 38.2 ms at 16 Mi, 38.4 ms at 32 Mi; profiles/r2_ab_grid_pool_knobs.txt)
    const uint64_t targetSlots = std::min<uint64_t>(ds.poolSlots, std::max<uint64_t>(1ull << 20, itemCount64 / 2u));
    uint32_t slots = static_cast<uint32_t>(std::min<uint64_t>(targetSlots, itemCount64));
    if (slots < itemCount64) slots &= ~255u;   // item ranges start right after the pre-assigned items: keep them 64-aligned
    // items [0, slots) are pre-assigned by k_generate; the rest is split into kItemHeads ranges with one head each
    rp.itemHeadFirst = slots;
    rp.itemsPerHead = static_cast<uint32_t>(((itemCount64 - slots + kItemHeads - 1u) / kItemHeads + 63u) & ~63ull);

    sizeSlots(ds, rp, count, slots);
    EnvLodView env;
    PathPool pool = slotRange(ds, rp, count, slots, 0u, slots, env);
    pool.pixelOfLocal = dPixelOfLocal;
    std::vector<PoolGroup> groups = makeGroups(ds, rp, count, soloGroup, slots, stream);
    for (PoolGroup& gr : groups) gr.pool.pixelOfLocal = dPixelOfLocal;
    LaunchTimer timer{stats != nullptr};

    if (count && (passFlags & 1u)) HIP_CHECK(hipMemsetAsync(ds.counters.ptr, 0, sizeof(uint64_t) * kCounterSlots, stream));   // counters add up over the passes
    HIP_CHECK(hipMemsetAsync(ds.scalars.ptr, 0, sizeof(uint32_t) * kScalarCount * kMaxPoolGroups, stream));
    HIP_CHECK(hipMemsetAsync(ds.connectCounts.ptr, 0, sizeof(uint32_t) * kConnectCountWords * 2u * kMaxPoolGroups, stream));
    HIP_CHECK(hipMemsetAsync(ds.busyCounts.ptr, 0, sizeof(uint32_t) * kConnectCountWords * 3u * kMaxPoolGroups, stream));
    uint32_t* heads = ds.pinnedAlive + kPinnedHeadsOffset;
    for (uint32_t k = 0; k < kItemHeads; ++k) heads[k] = static_cast<uint32_t>(itemRangeStart(rp, k));
    HIP_CHECK(hipMemsetAsync(pool.nextItem, 0, sizeof(uint32_t) * kItemHeadWords, stream));
    HIP_CHECK(hipMemcpy2DAsync(pool.nextItem, sizeof(uint32_t) * kItemHeadStride, heads, sizeof(uint32_t), sizeof(uint32_t), kItemHeads,
                               hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));   // the pinned staging area is reused by the polls
    HIP_CHECK(hipMemsetAsync(ds.itemReserve.ptr, 0, sizeof(uint2) * ((slots + 63u) / 64u), stream));
    if (rp.maxDepth == 0) HIP_CHECK(hipMemsetAsync(ds.itemAccum.ptr, 0, sizeof(float4) * rp.itemCount, stream));

    const auto wall0 = std::chrono::steady_clock::now();
    launchGenerate(rp, pool, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ds.groupEvents[0], stream));
    for (size_t g = 1; g < groups.size(); ++g) HIP_CHECK(hipStreamWaitEvent(groups[g].stream, ds.groupEvents[0], 0));
    if (background.count > 0u) {
        timer.launch(SpanKind::Background, stream,
                     [&] { launchBackground(rp, ds.view, background.pixels, background.count, background.parts, background.out, stream); });
    }
    uint64_t iterations = 0;
    // Worst case: every sample runs maxDepth bounces in sequence on its slot.
    // (a subsurface random walk adds up to sssMaxSteps iterations to a bounce)
    const uint64_t perBounce = ((rp.mediaMode & PTR_METAL_SSS) && rp.sssMode == 2u && ds.hasRandomWalkMaterial) ? 1ull + rp.sssMaxSteps : 1ull;
    const uint64_t maxIterations = static_cast<uint64_t>(rp.maxDepth) * perBounce * ((itemCount64 + slots - 1) / slots + 1) + 8;
    const ptr::Knobs knobs = ptr::readKnobs();
    PollResult last{false, false, false, kPollEvery};   // what the last poll found (none yet)
    while (rp.maxDepth > 0) {
        const uint32_t ring = static_cast<uint32_t>(iterations % kAliveRing);
        const bool queueDry = last.queueDry;
        for (PoolGroup& gr : groups) {
            if (gr.done) continue;
            uint32_t* aliveSlot = gr.scalars + kAliveBase + ring;
            gr.cfg.feederChunk = gr.feederChunk;
            // work heads and the next live-slot counter are cleared by k_shade (all zero at the start of the frame)
            const ShadeResets resets{gr.scalars + 1, gr.scalars + 2, gr.scalars + kAliveBase + (ring + 1u) % kAliveRing,
                                     (queueDry && gr.feederChunk > ds.feederChunk) ? 1u : 0u};
            gr.selectLists(iterations, queueDry);
            timer.launch(SpanKind::Extend, gr.stream, [&] { launchExtend(ds.view, gr.pool, gr.cfg, queueDry ? aliveSlot : nullptr, count, gr.stream); });
            // k_shade's list instantiation claims leftover work items lane by lane and is a fifth slower than the plain kernel while
            // it still walks the slots: it is launched once the last count of live slots says its list is about to pay
            PathPool shadePool = gr.pool;
            if (!gr.shadeListed) shadePool.busyIn = nullptr;
            if (gr.side && iterations > 0) HIP_CHECK(hipStreamWaitEvent(gr.stream, gr.connectDone, 0));
            timer.launch(SpanKind::Shade, gr.stream, [&] { launchShade(rp, ds.view, shadePool, resets, gr.env, count, gr.stream); });
            if (gr.side) {
                // k_connect of this iteration on the side stream, after this k_shade; the next k_shade waits for it (above)
                HIP_CHECK(hipEventRecord(gr.shadeDone, gr.stream));
                HIP_CHECK(hipStreamWaitEvent(gr.side, gr.shadeDone, 0));
                LaunchConfig ccfg = gr.cfg;
                ccfg.spill = gr.sideSpill;
                timer.launch(SpanKind::Connect, gr.side, [&] { launchConnect(rp, ds.view, gr.pool, ccfg, count, gr.side); });
                HIP_CHECK(hipEventRecord(gr.connectDone, gr.side));
            } else {
                timer.launch(SpanKind::Connect, gr.stream, [&] { launchConnect(rp, ds.view, gr.pool, gr.cfg, count, gr.stream); });
            }
        }
        ++iterations;
        if (hook) (*hook)(iterations - 1u, pool);
        if (iterations >= last.nextCheck || iterations >= maxIterations) {
            last = poll(ds, groups, rp, slots, iterations, last.queueDry, knobs.verbosePolls);
            if (last.allDone || last.runTail) break;
            if (iterations >= maxIterations) throw HipError{"wavefront loop did not terminate"};
        }
    }
    for (const PoolGroup& gr : groups) if (gr.side) HIP_CHECK(hipStreamWaitEvent(gr.stream, gr.connectDone, 0));
    for (size_t g = 1; g < groups.size(); ++g) {
        HIP_CHECK(hipEventRecord(ds.groupEvents[g], groups[g].stream));
        HIP_CHECK(hipStreamWaitEvent(stream, ds.groupEvents[g], 0));
    }
    if (last.runTail) {
        HIP_CHECK(hipMemsetAsync(ds.tailWords.ptr, 0, 4 * sizeof(uint32_t), stream));
        timer.launch(SpanKind::Tail, stream,
                     [&] { launchTail(rp, ds.view, pool, env, groups[0].cfg, ds.tailList.ptr, ds.tailWords.ptr, ds.tailWords.ptr + 1, count, stream); });
    }
    resolve(rp, pool, timer);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
    if (stats) passStats(ds, rp, timer.spans, count, knobs, seconds, *stats);
}

}  // namespace

namespace ptrhost {

// A frame.  One accumulator per sample has to fit in a quarter of the free device memory (at most 16 GiB); a frame with
// more samples than that is rendered in several passes of equal sample counts whose per-pixel sums add up in the output
// buffer.  (Folding C samples into one work item instead keeps one pass but lengthens the end-of-frame drain: 4096 spp of
// config 2 as items of 9 samples ran at 1116 Msamples/s.)  The sample streams do not depend on the split.
uint64_t maxPassItems(const PtrDeviceScene* ds) {
    uint64_t maxItems = 0xFFFFFFF0ull;
    if (ds) maxItems = std::min<uint64_t>(itemBudgetBytes(*ds) / sizeof(float4), maxItems);
    if (const uint64_t forced = ptr::readKnobs().maxItems) maxItems = forced;   // test knob
    return maxItems;
}

uint32_t framePasses(const PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp) {
    const uint64_t maxItems = maxPassItems(&ds);
    // counted on the whole frame, not on this partition: every partition then splits the samples the same way and the image
    // stays bit-identical whatever the number of partitions
    const uint64_t pixels = static_cast<uint64_t>(settings.width) * settings.height;
    const uint64_t perPixel = std::max<uint64_t>(1u, maxItems / std::max<uint64_t>(pixels, 1u));   // samples per pixel that fit in one pass
    return static_cast<uint32_t>((std::max(1u, spp) + perPixel - 1u) / perPixel);
}

void renderBands(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t part, uint32_t parts, float* dOut,
                 hipStream_t stream, int mode, PtrRenderStats* stats, float* dCov) {
    if (settings.width == 0 || settings.height == 0) throw HipError{"render size must be non-zero"};
    if (parts == 0 || part >= parts) throw HipError{"bad partition"};
    HIP_CHECK(hipSetDevice(ds.device));
    spp = std::max(1u, spp);
    const uint32_t passes = framePasses(ds, settings, spp);
    if (passes <= 1u) {
        renderPass(ds, settings, spp, 0u, spp, 3u, part, parts, dOut, dCov, stream, mode, stats);
        return;
    }
    const uint32_t perPass = (spp + passes - 1u) / passes;
    PtrRenderStats sum{};
    uint32_t done = 0u;
    for (uint32_t p = 0; done < spp; ++p) {
        const uint32_t n = std::min(perPass, spp - done);
        const uint32_t flags = (p == 0u ? 1u : 0u) | (done + n >= spp ? 2u : 0u);
        PtrRenderStats one{};
        renderPass(ds, settings, n, done, spp, flags, part, parts, dOut, dCov, stream, mode, stats ? &one : nullptr);
        if (stats) {   // counters are cumulative on the device: the last pass reports the totals; times, launches and samples add up
            addLaunchStats(one, sum);
            one.totalSeconds += sum.totalSeconds;
            sum = one;
        }
        done += n;
    }
    if (stats) {
        sum.avgMsPerSample = sum.totalSeconds * 1000.0 / spp;
        *stats = sum;
    }
}

void traceItems(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t sampleBase, const uint32_t* dPixelOfLocal,
                uint32_t localPixels, hipStream_t stream, PtrRenderStats* stats, const std::function<void(const float4*)>& consume,
                int mode, const IterationHook* hook) {
    // (pass flags 1: k_resolve, which launchResolve runs behind the flush of the outstanding connections, overwrites dScratch)
    const size_t scratchFloats = static_cast<size_t>(ptr_part_band_count(settings.height, 0u, 1u)) * PTR_BAND_ROWS * settings.width * 3u;
    ds.outBands.ensure(scratchFloats);
    tracePass(ds, settings, spp, sampleBase, spp, 1u, dPixelOfLocal, localPixels, stream, mode, stats,
              [&](const RenderParams& rp, const PathPool& pool, LaunchTimer&) {
                  launchResolve(rp, pool, 1u, ds.outBands.ptr, stream);
                  consume(pool.itemAccum);
              },
              BackgroundPixels{}, hook);
}

void imagePixelOrder(uint32_t width, uint32_t height, std::vector<uint32_t>& out) { partitionPixels(width, height, 0u, 1u, out); }

void addPassStats(const PtrRenderStats& one, PtrRenderStats& sum) {
    addLaunchStats(sum, one);
    sum.totalSeconds += one.totalSeconds;
    sum.uploadSeconds = one.uploadSeconds;
}

}  // namespace ptrhost

extern "C" {

int ptr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

uint32_t ptr_part_band_count(uint32_t height, uint32_t part_index, uint32_t part_count) {
    if (part_count == 0 || part_index >= part_count) return 0;
    const uint32_t bands = (height + PTR_BAND_ROWS - 1u) / PTR_BAND_ROWS;
    return bands > part_index ? (bands - part_index + part_count - 1u) / part_count : 0u;
}

int ptr_scene_upload(const PtrSceneDesc* scene, int device, PtrDeviceScene** out_scene, char* err, size_t err_cap) {
    return uploadTo("ptr_scene_upload", scene, nullptr, device, out_scene, err, err_cap);
}

int ptr_scene_upload_dynamic(const PtrSceneDesc* scene, int device, PtrDeviceScene** out_scene, char* err, size_t err_cap) {
    return uploadDynamic("ptr_scene_upload_dynamic", 0u, scene, device, 0u, out_scene, err, err_cap);
}

int ptr_scene_upload_dynamic_ex(const PtrSceneDesc* scene, int device, uint32_t flags, PtrDeviceScene** out_scene, char* err, size_t err_cap) {
    return uploadDynamic("ptr_scene_upload_dynamic_ex", PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES, scene, device, flags, out_scene, err, err_cap);
}

int ptr_scene_upload_deformable(const PtrSceneDesc* scene, int device, uint32_t flags, PtrDeviceScene** out_scene, char* err, size_t err_cap) {
    return uploadDynamic("ptr_scene_upload_deformable", PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS, scene, device, flags,
                         out_scene, err, err_cap);
}

void ptr_scene_release(PtrDeviceScene* scene) {
    if (!scene) return;
    (void)hipSetDevice(scene->device);
    delete scene;
}

int ptr_scene_info(const PtrDeviceScene* scene, uint64_t out[8]) {
    if (!scene || !out) return 1;
    std::memcpy(out, scene->info, sizeof(scene->info));
    return 0;
}

int ptr_scene_timings(const PtrDeviceScene* scene, double out[4]) {
    if (!scene || !out) return 1;
    std::memcpy(out, scene->timings, sizeof(scene->timings));
    return 0;
}

int ptr_scene_prepare_geometry(const PtrSceneDesc* scene, const char* cache_path, double* seconds, char* err, size_t err_cap) {
    if (!scene || !cache_path || !*cache_path) {
        setErr(err, err_cap, "ptr_scene_prepare_geometry: null argument");
        return 1;
    }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        ptr::PreparedGeometry pg;
        prepareGeometry(*scene, pg);
        std::string error;
        if (!ptr::WriteGeometryCache(cache_path, pg, ptr::SceneFingerprint(*scene), error)) throw HipError{error};
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_scene_upload_prepared(const PtrSceneDesc* scene, const char* cache_path, int device, PtrDeviceScene** out_scene, char* err, size_t err_cap) {
    if (!cache_path || !*cache_path) return nullArgument("ptr_scene_upload_prepared", err, err_cap);
    return uploadTo("ptr_scene_upload_prepared", scene, cache_path, device, out_scene, err, err_cap);
}

int ptr_render_bands_device(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index,
                            uint32_t part_count, void* d_out_rgb, void* stream, int count_traversal,
                            PtrRenderStats* stats, char* err, size_t err_cap) {
    if (!scene || !settings || !d_out_rgb) {
        setErr(err, err_cap, "ptr_render_bands_device: null argument");
        return 1;
    }
    try {
        renderBands(*scene, *settings, spp, part_index, part_count, static_cast<float*>(d_out_rgb),
                    static_cast<hipStream_t>(stream), count_traversal, stats);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_render_bands(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index,
                     uint32_t part_count, float* out_rgb_bands, int count_traversal, PtrRenderStats* stats,
                     char* err, size_t err_cap) {
    if (!scene || !settings || !out_rgb_bands) {
        setErr(err, err_cap, "ptr_render_bands: null argument");
        return 1;
    }
    try {
        const size_t floats = static_cast<size_t>(ptr_part_band_count(settings->height, part_index, part_count)) * PTR_BAND_ROWS * settings->width * 3u;
        HIP_CHECK(hipSetDevice(scene->device));
        scene->outBands.ensure(floats);
        renderBands(*scene, *settings, spp, part_index, part_count, scene->outBands.ptr, nullptr, count_traversal, stats);
        HIP_CHECK(hipMemcpy(out_rgb_bands, scene->outBands.ptr, floats * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_render(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, int verbose, float* out_rgb,
               PtrRenderStats* stats, char* err, size_t err_cap) {
    if (!scene || !settings || !out_rgb) {
        setErr(err, err_cap, "ptr_render: null argument");
        return 1;
    }
    PtrDeviceScene* ds = nullptr;
    int rc = ptr_scene_upload(scene, 0, &ds, err, err_cap);
    if (rc != 0) return rc;
    const uint32_t bands = (settings->height + PTR_BAND_ROWS - 1u) / PTR_BAND_ROWS;
    std::vector<float> banded;
    try {
        banded.resize(static_cast<size_t>(bands) * PTR_BAND_ROWS * settings->width * 3u);
    } catch (const std::exception& e) {
        ptr_scene_release(ds);
        setErr(err, err_cap, std::string("exception: ") + e.what());
        return 1;
    }
    PtrRenderStats local{};
    rc = ptr_render_bands(ds, settings, spp, 0, 1, banded.data(), 0, &local, err, err_cap);
    if (rc == 0) {
        // with a single partition the band layout is the image itself (plus padding rows)
        std::memcpy(out_rgb, banded.data(), static_cast<size_t>(settings->width) * settings->height * 3u * sizeof(float));
        if (stats) *stats = local;
        if (verbose) {
            std::fprintf(stderr, "[ptr] BVH %llu nodes, %llu tris, %llu spheres; upload %.3f s; render %.3f s (trace %.1f ms, shade %.1f ms, connect %.1f ms)\n",
                         static_cast<unsigned long long>(ds->info[0]), static_cast<unsigned long long>(ds->info[2]),
                         static_cast<unsigned long long>(ds->info[3]), ds->uploadSeconds, local.totalSeconds,
                         local.traceKernelMs, local.shadeKernelMs, local.shadowKernelMs);
        }
    }
    ptr_scene_release(ds);
    return rc;
}

int ptr_trace_rays(PtrDeviceScene* scene, const float* rays, uint64_t n, int any_hit, PtrHit* out, PtrRenderStats* stats,
                   char* err, size_t err_cap) {
    return deviceCall("ptr_trace_rays", scene, scene && (rays || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        scene->rayBatch.upload(reinterpret_cast<const float4*>(rays), n * 2);
        scene->hitBatch.ensure(n);
        HIP_CHECK(hipMemset(scene->counters.ptr, 0, sizeof(uint64_t) * kCounterSlots));
        launchTraceRays(scene->view, scene->rayBatch.ptr, n, any_hit != 0, scene->hitBatch.ptr, coldLaunchConfig(*scene), scene->counters.ptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        scene->hitBatch.download(out, n);
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            uint64_t c[kCounterSlots];
            scene->counters.download(c, kCounterSlots);
            stats->nodesVisited = c[kCntExtendNodes] + c[kCntShadowNodes];
            stats->leafPrimTests = c[kCntExtendPrims] + c[kCntShadowPrims];
            stats->extendRays = any_hit ? 0 : n;
            stats->shadowRays = any_hit ? n : 0;
        }
    });
}

int ptr_render_aovs(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t sample_index, float* out_albedo, float* out_normal,
                    char* err, size_t err_cap) {
    return deviceCall("ptr_render_aovs", scene, scene && settings, err, err_cap, [&] {
        if (settings->width == 0 || settings->height == 0) throw HipError{"render size must be non-zero"};
        DeviceBuffer<float4> albedo, normal;
        downloadFirstHit(*scene, *settings, sample_index, albedo, normal, out_albedo, out_normal);
    });
}

}  // extern "C"
