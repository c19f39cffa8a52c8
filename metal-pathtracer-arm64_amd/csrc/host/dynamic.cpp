// Dynamic scenes (include/ptr_dynamic.h): the upload of the extra device data, ptr_scene_set_mesh_transforms, and that header's two
// test-only probes, which look at a scene's arrays.  Compiled with hipcc (host code only), like hip_backend.cpp; the kernels are in
// kernels/dynamic.hip.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "../kernels/bvh_grid.h"
#include "../kernels/dynamic.h"
#include "device_scene.h"
#include "ptr_dynamic.h"

using namespace ptrk;
using namespace ptrhost;

namespace ptrhost {

void uploadDynamicTables(const PreparedScene& ps, PtrDeviceScene& ds) {
    const ptr::DynamicTables& t = ps.dyn;
    const ptr::FlatBvh& bvh = ps.pg.geo.bvh;
    auto dyn = std::make_unique<DynamicScene>();
    dyn->objPos.upload(reinterpret_cast<const float4*>(t.objPos.data()), t.objPos.size() / 4);
    dyn->objNrm.upload(reinterpret_cast<const float4*>(t.objNrm.data()), t.objNrm.size() / 4);
    dyn->textured = ds.view.triUv != nullptr;
    if (dyn->textured) dyn->objTan.upload(reinterpret_cast<const float4*>(t.objTan.data()), t.objTan.size() / 4);
    dyn->triBounds.upload(reinterpret_cast<const float4*>(t.triBounds.data()), t.triBounds.size() / 4);
    dyn->sphereBounds.upload(reinterpret_cast<const float4*>(t.sphereBounds.data()), t.sphereBounds.size() / 4);
    // a scene that renders from float nodes refits those; a quantised one keeps the float nodes beside the ones it renders from
    if (ps.pg.useQuantized) dyn->boxes.upload(reinterpret_cast<const float4*>(bvh.nodes.data()), bvh.nodes.size() / 4);
    dyn->meshTris.upload(t.meshTris.data(), t.meshTris.size());
    dyn->schedule.upload(t.schedule.data(), t.schedule.size());
    if (ps.pg.wideCount > 0u) dyn->wideSource.upload(t.wideSource.data(), t.wideSource.size());
    dyn->meshTriOffsets = t.meshTriOffsets;
    dyn->levelOffsets = t.levelOffsets;
    dyn->meshHasTangents = t.meshHasTangents;
    dyn->nodeCount = bvh.nodeCount;
    dyn->wideCount = ps.pg.wideCount;
    dyn->triCount = ps.pg.geo.triCount;
    dyn->sphereCount = ps.pg.geo.sphereCount;
    dyn->meanPrimExtent = bvh.meanPrimExtent;
    for (hipEvent_t& e : dyn->events) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&dyn->rootBox), 4 * sizeof(float4), hipHostMallocDefault));
    ds.dynamic = std::move(dyn);
}

}  // namespace ptrhost

namespace {

float4* floatBoxes(PtrDeviceScene& ds) { return ds.view.useQuantized ? ds.dynamic->boxes.ptr : ds.nodes.ptr; }

// the root box of the tree from node 0: the union of its children that exist
bool rootBoxOf(const float4 row[4], float lo[3], float hi[3]) {
    bool any = false;
    for (int c = 0; c < 2; ++c) {
        uint32_t ref;
        std::memcpy(&ref, &row[c].w, 4);
        if (ref == kRefEmpty) continue;
        const float4 l = row[c * 2], h = row[c * 2 + 1];
        const float cl[3] = {l.x, l.y, l.z}, ch[3] = {h.x, h.y, h.z};
        for (int a = 0; a < 3; ++a) {
            lo[a] = any ? std::min(lo[a], cl[a]) : cl[a];
            hi[a] = any ? std::max(hi[a], ch[a]) : ch[a];
        }
        any = true;
    }
    return any;
}

std::string matrixProblem(const float m[16], const ptr::MeshBake& bake) {
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(m[i])) return "has a non-finite entry";
    }
    if (bake.det3 == 0.0f || !std::isfinite(bake.det3)) return "has a zero 3x3 determinant";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(bake.nc0[a]) || !std::isfinite(bake.nc1[a]) || !std::isfinite(bake.nc2[a])) return "has a cofactor inverse that is not finite";
    }
    return "";
}

}  // namespace

extern "C" {

int ptr_scene_is_dynamic(const PtrDeviceScene* scene) { return scene && scene->dynamic ? 1 : 0; }

int ptr_scene_set_mesh_transforms(PtrDeviceScene* scene, const PtrMeshTransform* transforms, uint32_t count, void* stream, PtrUpdateInfo* info,
                                  char* err, size_t err_cap) {
    const char* who = "ptr_scene_set_mesh_transforms";
    if (!scene) return nullArgument(who, err, err_cap);
    if (!scene->dynamic) return refuse(err, err_cap, std::string(who) + ": the scene is not dynamic (upload it with ptr_scene_upload_dynamic)");
    if (!transforms) return refuse(err, err_cap, std::string(who) + ": null transform list");
    if (count == 0u) return refuse(err, err_cap, std::string(who) + ": count is 0");
    DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    std::vector<DynMeshRow> rows(count);
    try {
        std::vector<uint8_t> named(meshCount, 0);
        for (uint32_t i = 0; i < count; ++i) {
            const PtrMeshTransform& t = transforms[i];
            if (t.meshIndex >= meshCount) {
                return refuse(err, err_cap, std::string(who) + ": mesh index " + std::to_string(t.meshIndex) + " out of range (the scene has " +
                                                std::to_string(meshCount) + " meshes)");
            }
            if (named[t.meshIndex]++) return refuse(err, err_cap, std::string(who) + ": mesh index " + std::to_string(t.meshIndex) + " named twice");
            ptr::MeshBake bake;
            ptr::ComputeMeshBake(t.localToWorld, bake);
            const std::string problem = matrixProblem(t.localToWorld, bake);
            if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": the matrix of mesh " + std::to_string(t.meshIndex) + " " + problem);
            DynMeshRow& r = rows[i];
            std::memset(&r, 0, sizeof(r));
            std::memcpy(r.l2w, bake.localToWorld, sizeof(r.l2w));
            std::memcpy(r.nc0, bake.nc0, 12);
            std::memcpy(r.nc1, bake.nc1, 12);
            std::memcpy(r.nc2, bake.nc2, 12);
            r.detSign = bake.detSign;
            r.hasTangents = dyn.meshHasTangents[t.meshIndex] ? 1.0f : 0.0f;
        }
    }
    PTR_CATCH_ALL(err, err_cap)

    return deviceCall(who, scene, true, err, err_cap, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = static_cast<hipStream_t>(stream);
        PtrDeviceScene& ds = *scene;
        SceneView& v = ds.view;
        dyn.meshTable.ensure(static_cast<size_t>(count) * kDynMeshVec4);
        HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, rows.data(), rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(dyn.events[0], st));
        DynBakeArrays arrays{dyn.objPos.ptr, dyn.objNrm.ptr, dyn.textured ? dyn.objTan.ptr : nullptr, ds.tris.ptr, ds.triNormals.ptr, dyn.triBounds.ptr,
                             dyn.textured ? ds.triUv.ptr : nullptr, dyn.textured ? ds.triTangent.ptr : nullptr};
        uint64_t moved = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t m = transforms[i].meshIndex;
            const uint32_t first = dyn.meshTriOffsets[m], n = dyn.meshTriOffsets[m + 1u] - first;
            launchDynBake(arrays, dyn.meshTable.ptr, i, dyn.meshTris.ptr + first, n, st);
            moved += n;
        }
        HIP_CHECK(hipEventRecord(dyn.events[1], st));
        float4* boxes = floatBoxes(ds);
        const uint32_t levels = static_cast<uint32_t>(dyn.levelOffsets.size()) - 1u;
        for (uint32_t l = 0; l < levels; ++l) {
            launchDynRefitLevel(boxes, dyn.schedule.ptr + dyn.levelOffsets[l], dyn.levelOffsets[l + 1u] - dyn.levelOffsets[l], dyn.triBounds.ptr,
                                dyn.sphereBounds.ptr, st);
        }
        HIP_CHECK(hipEventRecord(dyn.events[2], st));
        float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        if (dyn.nodeCount > 0u) {
            // the grid travels to the kernels as arguments: the host needs the root box before it can launch the quantiser
            HIP_CHECK(hipMemcpyAsync(dyn.rootBox, boxes, 4 * sizeof(float4), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (rootBoxOf(dyn.rootBox, lo, hi)) {
                for (int a = 0; a < 3; ++a) {
                    gridAxis(lo[a], hi[a], v.gridOrigin[a], v.gridCell[a]);
                    v.gridInvCell[a] = 1.0f / v.gridCell[a];
                }
            }
        }
        // What a ray can hit now (csrc/host/background_cull.h): the refitted root box holds every primitive of the tree.  Triangles kept
        // out of the tree moved on the device only, and a scene without nodes has no root box: nothing is culled there.
        ds.worldBounds = ptr::WorldBounds{};
        if (dyn.nodeCount > 0u && v.oversizeRef == kRefEmpty && rootBoxOf(dyn.rootBox, lo, hi)) {
            for (int a = 0; a < 3; ++a) ds.worldBounds.lo[a] = lo[a], ds.worldBounds.hi[a] = hi[a];
            ds.worldBounds.valid = true;
        }
        if (v.useQuantized) launchDynQuantise(boxes, ds.qnodes.ptr, dyn.nodeCount, v.gridOrigin, v.gridCell, st);
        HIP_CHECK(hipEventRecord(dyn.events[3], st));
        if (v.useWide) launchDynWide(ds.qnodes.ptr, ds.wnodes.ptr, dyn.wideSource.ptr, dyn.wideCount * 4u, st);
        HIP_CHECK(hipEventRecord(dyn.events[4], st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (info) {
            std::memset(info, 0, sizeof(*info));
            float ms[4] = {0, 0, 0, 0};
            for (int g = 0; g < 4; ++g) HIP_CHECK(hipEventElapsedTime(&ms[g], dyn.events[g], dyn.events[g + 1]));
            info->bakeMs = ms[0], info->refitMs = ms[1], info->quantiseMs = ms[2], info->wideMs = ms[3];
            info->trianglesMoved = moved;
            info->nodes = dyn.nodeCount;
            info->levels = levels;
            info->wideNodes = dyn.wideCount;
            for (int a = 0; a < 3; ++a) {
                info->sceneLo[a] = lo[a], info->sceneHi[a] = hi[a];
                info->gridOrigin[a] = v.gridOrigin[a], info->gridCell[a] = v.gridCell[a];
            }
            const float maxCell = std::max(std::max(v.gridCell[0], v.gridCell[1]), v.gridCell[2]);
            info->cellOverExtent = dyn.meanPrimExtent > 0.0f ? maxCell / dyn.meanPrimExtent : 0.0f;
            info->totalSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
    });
}

int ptr_debug_scene_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out) {
    if (!scene || !size_out) return 1;
    const PtrDeviceScene& ds = *scene;
    const DynamicScene* dyn = ds.dynamic.get();
    const uint64_t tris = ds.info[2], spheres = ds.info[3], nodes = ds.info[0];
    const void* src = nullptr;
    uint64_t bytes = 0;
    switch (which) {
        case PTR_SCENE_ARRAY_TRIS: src = ds.tris.ptr, bytes = tris * 48u; break;
        case PTR_SCENE_ARRAY_TRI_NORMALS: src = ds.triNormals.ptr, bytes = tris * 48u; break;
        case PTR_SCENE_ARRAY_TRI_UV: src = ds.triUv.ptr, bytes = ds.view.triUv ? tris * 64u : 0u; break;
        case PTR_SCENE_ARRAY_TRI_TANGENT: src = ds.triTangent.ptr, bytes = ds.view.triTangent ? tris * 48u : 0u; break;
        case PTR_SCENE_ARRAY_TRI_BOUNDS: src = dyn ? dyn->triBounds.ptr : nullptr, bytes = dyn ? tris * 32u : 0u; break;
        case PTR_SCENE_ARRAY_SPHERE_BOUNDS: src = dyn ? dyn->sphereBounds.ptr : nullptr, bytes = dyn ? spheres * 32u : 0u; break;
        case PTR_SCENE_ARRAY_BOXES:
            src = ds.view.useQuantized ? (dyn ? dyn->boxes.ptr : nullptr) : ds.nodes.ptr;
            bytes = src ? nodes * 64u : 0u;
            break;
        case PTR_SCENE_ARRAY_QNODES: src = ds.qnodes.ptr, bytes = ds.view.useQuantized ? nodes * 32u : 0u; break;
        case PTR_SCENE_ARRAY_WNODES: src = ds.wnodes.ptr, bytes = ds.view.useWide ? ds.view.wideBytes : 0u; break;
        case PTR_SCENE_ARRAY_GRID: bytes = 24u; break;
        default: return 1;
    }
    *size_out = bytes;
    if (!out) return 0;
    if (cap_bytes < bytes) return 2;
    if (bytes == 0u) return 0;
    if (which == PTR_SCENE_ARRAY_GRID) {
        std::memcpy(out, ds.view.gridOrigin, 12);
        std::memcpy(static_cast<char*>(out) + 12, ds.view.gridCell, 12);
        return 0;
    }
    if (hipSetDevice(ds.device) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}

int ptr_debug_dynamic_tables(const PtrSceneDesc* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err, size_t err_cap) {
    if (!scene || !size_out) return nullArgument("ptr_debug_dynamic_tables", err, err_cap);
    try {
        ptr::PreparedGeometry pg;
        ptr::DynamicTables t;
        prepareGeometry(*scene, pg, &t);
        const ptr::FlatBvh& bvh = pg.geo.bvh;
        std::vector<uint32_t> words;
        const void* src = nullptr;
        uint64_t bytes = 0;
        auto take = [&](const void* p, size_t n) { src = p, bytes = n; };
        switch (which) {
            case PTR_DYNAMIC_TABLE_NODES: take(bvh.nodes.data(), bvh.nodes.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_QNODES: take(bvh.qnodes.data(), bvh.qnodes.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_WNODES: take(pg.wide.get(), static_cast<size_t>(pg.wideCount) * 64u); break;
            case PTR_DYNAMIC_TABLE_TRI_BOUNDS: take(t.triBounds.data(), t.triBounds.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_SPHERE_BOUNDS: take(t.sphereBounds.data(), t.sphereBounds.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_SCHEDULE: take(t.schedule.data(), t.schedule.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_LEVEL_OFFSETS: take(t.levelOffsets.data(), t.levelOffsets.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_WIDE_SOURCE: take(t.wideSource.data(), pg.wideCount > 0u ? t.wideSource.size() * 4u : 0u); break;
            case PTR_DYNAMIC_TABLE_GRID:
                words.resize(6);
                std::memcpy(words.data(), bvh.gridOrigin, 12);
                std::memcpy(words.data() + 3, bvh.gridCell, 12);
                take(words.data(), 24u);
                break;
            case PTR_DYNAMIC_TABLE_REQUANTISED:
                // the shared quantiser (kernels/bvh_grid.h) on the float nodes, with the grid the shared rule derives from node 0
                words.assign(static_cast<size_t>(bvh.nodeCount) * 8u, 0u);
                if (bvh.nodeCount > 0u) {
                    float lo[3], hi[3], origin[3], cell[3];
                    float4 row[4];
                    std::memcpy(row, bvh.nodes.data(), sizeof(row));
                    rootBoxOf(row, lo, hi);
                    for (int a = 0; a < 3; ++a) gridAxis(lo[a], hi[a], origin[a], cell[a]);
                    for (uint32_t i = 0; i < bvh.nodeCount; ++i) ptr::QuantiseNode(&bvh.nodes[static_cast<size_t>(i) * 16u], origin, cell, &words[static_cast<size_t>(i) * 8u]);
                }
                take(words.data(), words.size() * 4u);
                break;
            case PTR_DYNAMIC_TABLE_MESH_TRI_OFFSETS: take(t.meshTriOffsets.data(), t.meshTriOffsets.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_MESH_TRIS: take(t.meshTris.data(), t.meshTris.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_INFO:
                words = {bvh.nodeCount, static_cast<uint32_t>(t.levelOffsets.size()) - 1u, pg.wideCount, pg.useQuantized ? 1u : 0u, pg.geo.triCount,
                         pg.geo.sphereCount, bvh.maxDepth, bvh.rootRef, bvh.oversizeRef, pg.wideDepth};
                take(words.data(), words.size() * 4u);
                break;
            default: return refuse(err, err_cap, "ptr_debug_dynamic_tables: no such table");
        }
        *size_out = bytes;
        if (!out) return 0;
        if (cap_bytes < bytes) return refuse(err, err_cap, "ptr_debug_dynamic_tables: the buffer is too small");
        if (bytes) std::memcpy(out, src, bytes);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
