// Dynamic scenes (include/ptr_dynamic.h, include/ptr_deform.h, include/ptr_deform_device.h): the upload of the extra device data,
// ptr_scene_set_mesh_transforms, ptr_scene_set_mesh_vertices and its device-pointer form, ptr_scene_set_spheres and ptr_scene_set_rects,
// which all end in the same refit (finishUpdate), and the headers' test-only probes, which look at a scene's arrays.  Compiled with
// hipcc (host code only), like hip_backend.cpp; the kernels are in kernels/dynamic.hip.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "../kernels/bvh_grid.h"
#include "../kernels/dynamic.h"
#include "device_scene.h"
#include "ptr_deform_device.h"
#include "ptr_dynamic.h"
#include "rebuild_host.h"
#include "vecmath.h"

using namespace ptrk;
using namespace ptrhost;

namespace ptrhost {

ptrk::DynMeshRow meshRowOf(const ptr::MeshBake& bake, bool hasTangents) {
    DynMeshRow r;
    std::memset(&r, 0, sizeof(r));
    std::memcpy(r.l2w, bake.localToWorld, sizeof(r.l2w));
    std::memcpy(r.nc0, bake.nc0, 12);
    std::memcpy(r.nc1, bake.nc1, 12);
    std::memcpy(r.nc2, bake.nc2, 12);
    r.detSign = bake.detSign;
    r.hasTangents = hasTangents ? 1.0f : 0.0f;
    return r;
}

void fillPrimitiveRecords(const PtrSceneDesc& desc, const ptr::SceneGeometry& geo, const ptr::DynamicTables& t, const std::vector<int32_t>& lightIndexByRect,
                          PrimitiveRecords& out) {
    out = PrimitiveRecords{};
    out.rectTriLeaf = geo.rectTriLeaf;
    out.sphereLeaf = t.sphereLeaf;
    out.rectShadeKey = t.rectShadeKey;
    out.lightIndexByRect = lightIndexByRect;
    out.rectEmission.assign(static_cast<size_t>(desc.rectCount) * 3u, 0.0f);
    for (uint32_t i = 0; i < desc.rectCount; ++i) {
        if (lightIndexByRect[i] < 0) continue;
        const PtrMaterial& m = desc.materials[std::min(desc.rects[i].materialTwoSided[0], desc.materialCount - 1u)];
        std::memcpy(&out.rectEmission[static_cast<size_t>(i) * 3u], m.emission, 12);
    }
    out.rects.assign(desc.rects, desc.rects + desc.rectCount);
    out.spheres.assign(desc.spheres, desc.spheres + desc.sphereCount);
    out.triCount = geo.triCount;
}

void uploadDynamicTables(const PtrSceneDesc& desc, const PreparedScene& ps, PtrDeviceScene& ds) {
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
    dyn->meshRows.resize(t.meshBakes.size());
    for (size_t m = 0; m < t.meshBakes.size(); ++m) dyn->meshRows[m] = meshRowOf(t.meshBakes[m], t.meshHasTangents[m] != 0);
    dyn->flags = t.flags;
    if (t.flags & PTR_DYNAMIC_DEFORMABLE) {
        dyn->meshCorners.upload(t.meshCorners.data(), t.meshCorners.size());
        dyn->meshVertexCount = t.meshVertexCount;
        dyn->meshTangentsGiven = t.meshTangentsGiven;
    }
    if (t.flags & PTR_DYNAMIC_VERTEX_NORMALS) {
        dyn->adjOffsets.upload(t.adjOffsets.data(), t.adjOffsets.size());
        dyn->adjEntries.upload(t.adjEntries.data(), t.adjEntries.size());
        dyn->adjBase = t.adjBase;
    }
    if (t.flags & PTR_DYNAMIC_PRIMITIVES) {
        fillPrimitiveRecords(desc, ps.pg.geo, t, ps.lightIndexByRect, dyn->prims);
    }
    for (hipEvent_t& e : dyn->events) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&dyn->rootBox), 4 * sizeof(float4), hipHostMallocDefault));
    ptr::BuildLeafTable(bvh.nodes.data(), bvh.nodeCount, dyn->leafTable);   // include/ptr_rebuild.h, step 1
    ds.dynamic = std::move(dyn);
}

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

}  // namespace ptrhost

namespace {

float4* floatBoxes(PtrDeviceScene& ds) { return ds.view.useQuantized ? ds.dynamic->boxes.ptr : ds.nodes.ptr; }

DynBakeArrays bakeArrays(PtrDeviceScene& ds) {
    DynamicScene& dyn = *ds.dynamic;
    return DynBakeArrays{dyn.objPos.ptr, dyn.objNrm.ptr, dyn.textured ? dyn.objTan.ptr : nullptr, ds.tris.ptr, ds.triNormals.ptr, dyn.triBounds.ptr,
                         dyn.textured ? ds.triUv.ptr : nullptr, dyn.textured ? ds.triTangent.ptr : nullptr};
}

// The staging buffer of ptr_scene_set_spheres / ptr_scene_set_rects: 16 B rows and where each goes, (PTR_SCATTER_* << 28) | row
struct ScatterRows {
    std::vector<float> rows;
    std::vector<uint32_t> dest;
};

// (defined below the entry points)
void finishUpdate(PtrDeviceScene& ds, hipStream_t st, std::chrono::steady_clock::time_point t0, uint64_t moved, PtrUpdateInfo* info);
// The host half of a sphere's / a rectangle's move: the new record into `prims`, its rows appended to `out`.  "" or what is wrong with it.
std::string sphereRows(PrimitiveRecords& prims, const PtrSphereUpdate& u, ScatterRows& out);
std::string rectRows(PrimitiveRecords& prims, const PtrRectUpdate& u, ScatterRows& out);
int setPrimitives(const char* who, uint32_t kind, PtrDeviceScene* scene, const void* list, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                  size_t err_cap);

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

// One named mesh of ptr_scene_set_mesh_vertices / ptr_scene_set_mesh_vertices_device once the call is accepted
struct MeshSource {
    bool used = false;   // false: a mesh without triangles, which changes nothing
    DynVertexArrays v{nullptr, nullptr, nullptr};   // where the gather reads its arrays, on the device
};

// What both calls refuse about entry `mv` of their list (PtrMeshVertices and PtrMeshVerticesDevice have the same members): "" or the
// cause.  named: per mesh of the scene, how often the list has named it so far.  used: the mesh has triangles.
template <typename V>
std::string namedMeshProblem(const DynamicScene& dyn, const V& mv, std::vector<uint8_t>& named, bool normalsMayBeNull, const char* nullNormalsHint, bool& used) {
    used = false;
    const uint32_t meshCount = static_cast<uint32_t>(named.size());
    if (mv.meshIndex >= meshCount) {
        return "mesh index " + std::to_string(mv.meshIndex) + " out of range (the scene has " + std::to_string(meshCount) + " meshes)";
    }
    if (named[mv.meshIndex]++) return "mesh index " + std::to_string(mv.meshIndex) + " named twice";
    if (dyn.meshTriOffsets[mv.meshIndex + 1u] == dyn.meshTriOffsets[mv.meshIndex]) return "";   // no triangles: nothing to change
    const std::string mesh = "mesh " + std::to_string(mv.meshIndex);
    if (mv.vertexCount != dyn.meshVertexCount[mv.meshIndex]) {
        return mesh + " was uploaded with " + std::to_string(dyn.meshVertexCount[mv.meshIndex]) + " vertices, not vertexCount " + std::to_string(mv.vertexCount);
    }
    if (!mv.positions) return mesh + " has null positions";
    if (!mv.normals && !normalsMayBeNull) return mesh + " has null normals" + nullNormalsHint;
    if (mv.tangents && !dyn.meshTangentsGiven[mv.meshIndex]) return mesh + " was uploaded without tangents and is given some";
    if (!mv.tangents && dyn.meshTangentsGiven[mv.meshIndex]) return mesh + " was uploaded with tangents and is given none";
    used = true;
    return "";
}

// What both calls run once the mesh table is on the device and event 0 is recorded: per named mesh with triangles the gather of its
// arrays into the object-space corner rows and the bake under the matrix the mesh has (row i of the table), then the shared tail.
template <typename V>
void gatherBakeFinish(PtrDeviceScene& ds, const V* meshes, const std::vector<MeshSource>& src, hipStream_t st, std::chrono::steady_clock::time_point t0,
                      PtrUpdateInfo* info) {
    DynamicScene& dyn = *ds.dynamic;
    const DynBakeArrays arrays = bakeArrays(ds);
    uint64_t moved = 0;
    for (uint32_t i = 0; i < src.size(); ++i) {
        if (!src[i].used) continue;
        const uint32_t m = meshes[i].meshIndex;
        const uint32_t first = dyn.meshTriOffsets[m], n = dyn.meshTriOffsets[m + 1u] - first;
        launchDynGatherCorners(dyn.objPos.ptr, dyn.objNrm.ptr, dyn.textured ? dyn.objTan.ptr : nullptr, src[i].v, dyn.meshTris.ptr + first,
                               dyn.meshCorners.ptr + static_cast<size_t>(first) * 3u, n, st);
        launchDynBake(arrays, dyn.meshTable.ptr, i, dyn.meshTris.ptr + first, n, st);
        moved += n;
    }
    finishUpdate(ds, st, t0, moved, info);
}

// What is wrong with `bytes` of a caller's array at `p` for a kernel on `device` to read, or "": the host half of
// ptr_scene_set_mesh_vertices_device looks at the pointer alone, never at what it points to.
std::string devicePointerProblem(const void* p, size_t bytes, int device) {
    if (reinterpret_cast<uintptr_t>(p) & 3u) return "is not 4 B aligned";
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // (a pointer the runtime has never seen)
        return "is host memory, not device memory";
    }
    if (attr.isManaged || attr.type == hipMemoryTypeManaged) return "is managed memory, not plain device memory";
    if (attr.type == hipMemoryTypeHost) return "is registered or pinned host memory, not device memory";
    if (attr.type == hipMemoryTypeUnregistered) return "is host memory, not device memory";
    if (attr.type != hipMemoryTypeDevice) return "is not plain device memory";
    if (attr.device != device) return "is memory of device " + std::to_string(attr.device) + ", not of the scene's device " + std::to_string(device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();   // (no range on record: the kind and the device are what is known)
        return "";
    }
    const uintptr_t end = reinterpret_cast<uintptr_t>(base) + size, at = reinterpret_cast<uintptr_t>(p);
    if (at > end || end - at < bytes) return "has " + std::to_string(end - std::min(at, end)) + " B left in its allocation, fewer than the " + std::to_string(bytes) + " B of the array";
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
            rows[i] = meshRowOf(bake, dyn.meshHasTangents[t.meshIndex] != 0);
        }
    }
    PTR_CATCH_ALL(err, err_cap)

    return deviceCall(who, scene, true, err, err_cap, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = static_cast<hipStream_t>(stream);
        PtrDeviceScene& ds = *scene;
        dyn.meshTable.ensure(static_cast<size_t>(count) * kDynMeshVec4);
        HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, rows.data(), rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(dyn.events[0], st));
        const DynBakeArrays arrays = bakeArrays(ds);
        uint64_t moved = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t m = transforms[i].meshIndex;
            const uint32_t first = dyn.meshTriOffsets[m], n = dyn.meshTriOffsets[m + 1u] - first;
            launchDynBake(arrays, dyn.meshTable.ptr, i, dyn.meshTris.ptr + first, n, st);
            dyn.meshRows[m] = rows[i];   // the matrix a later ptr_scene_set_mesh_vertices bakes under
            moved += n;
        }
        finishUpdate(ds, st, t0, moved, info);
    });
}

int ptr_scene_set_mesh_vertices(PtrDeviceScene* scene, const PtrMeshVertices* meshes, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                                size_t err_cap) {
    const char* who = "ptr_scene_set_mesh_vertices";
    if (!scene) return nullArgument(who, err, err_cap);
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_DEFORMABLE)) {
        return refuse(err, err_cap, std::string(who) + ": the scene is not deformable (upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_DEFORMABLE)");
    }
    if (!meshes) return refuse(err, err_cap, std::string(who) + ": null mesh list");
    if (count == 0u) return refuse(err, err_cap, std::string(who) + ": count is 0");
    DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    // where the arrays of every named mesh go in the staging buffer, in floats (a mesh without triangles stages nothing)
    struct Staged {
        size_t positions = 0, normals = 0, tangents = 0;
        bool used = false, hasTangents = false;
    };
    std::vector<Staged> staged(count);
    std::vector<DynMeshRow> rows(count);
    size_t floats = 0;
    try {
        std::vector<uint8_t> named(meshCount, 0);
        for (uint32_t i = 0; i < count; ++i) {
            const PtrMeshVertices& mv = meshes[i];
            Staged& s = staged[i];
            const std::string problem = namedMeshProblem(dyn, mv, named, false, "", s.used);
            if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
            rows[i] = dyn.meshRows[mv.meshIndex];
            if (!s.used) continue;
            s.hasTangents = dyn.meshHasTangents[mv.meshIndex] != 0;   // (an untextured scene keeps no tangents: they are checked and dropped)
            s.positions = floats, floats += static_cast<size_t>(mv.vertexCount) * 3u;
            s.normals = floats, floats += static_cast<size_t>(mv.vertexCount) * 3u;
            if (s.hasTangents) s.tangents = floats, floats += static_cast<size_t>(mv.vertexCount) * 4u;
        }
        // staging: every array into the scene's pinned buffer, each component looked at on the way
        HIP_CHECK(hipSetDevice(scene->device));
        float* pinned = static_cast<float*>(dyn.pinnedFor(std::max<size_t>(floats, 4u) * sizeof(float)));
        auto stage = [&](const float* src, size_t n, float* dst) {
            bool finite = true;
            for (size_t k = 0; k < n; ++k) {
                finite = finite && std::isfinite(src[k]);
                dst[k] = src[k];
            }
            return finite;
        };
        for (uint32_t i = 0; i < count; ++i) {
            const PtrMeshVertices& mv = meshes[i];
            const Staged& s = staged[i];
            if (!s.used) continue;
            const size_t n = mv.vertexCount;
            const char* bad = nullptr;
            if (!stage(mv.positions, n * 3u, pinned + s.positions)) bad = "position";
            else if (!stage(mv.normals, n * 3u, pinned + s.normals)) bad = "normal";
            else if (mv.tangents) {
                std::vector<float> dropped;
                if (!s.hasTangents) dropped.resize(n * 4u);
                if (!stage(mv.tangents, n * 4u, s.hasTangents ? pinned + s.tangents : dropped.data())) bad = "tangent";
            }
            if (bad) return refuse(err, err_cap, std::string(who) + ": mesh " + std::to_string(mv.meshIndex) + " has a non-finite " + bad + " component");
        }
    }
    PTR_CATCH_ALL(err, err_cap)

    return deviceCall(who, scene, true, err, err_cap, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = static_cast<hipStream_t>(stream);
        dyn.staging.ensure((floats + 3u) / 4u);
        const float* dStaged = reinterpret_cast<const float*>(dyn.staging.ptr);
        if (floats) HIP_CHECK(hipMemcpyAsync(dyn.staging.ptr, dyn.pinned, floats * sizeof(float), hipMemcpyHostToDevice, st));
        dyn.meshTable.ensure(static_cast<size_t>(count) * kDynMeshVec4);
        HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, rows.data(), rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(dyn.events[0], st));
        std::vector<MeshSource> src(count);
        for (uint32_t i = 0; i < count; ++i) {
            const Staged& s = staged[i];
            src[i].used = s.used;
            if (s.used) src[i].v = DynVertexArrays{dStaged + s.positions, dStaged + s.normals, s.hasTangents ? dStaged + s.tangents : nullptr};
        }
        gatherBakeFinish(*scene, meshes, src, st, t0, info);
    });
}

int ptr_scene_set_mesh_vertices_device(PtrDeviceScene* scene, const PtrMeshVerticesDevice* meshes, uint32_t count, void* stream, PtrUpdateInfo* info,
                                       char* err, size_t err_cap) {
    const char* who = "ptr_scene_set_mesh_vertices_device";
    if (!scene) return nullArgument(who, err, err_cap);
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_DEFORMABLE)) {
        return refuse(err, err_cap, std::string(who) + ": the scene is not deformable (upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_DEFORMABLE)");
    }
    if (!meshes) return refuse(err, err_cap, std::string(who) + ": null mesh list");
    if (count == 0u) return refuse(err, err_cap, std::string(who) + ": count is 0");
    DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    const bool computes = (dyn.flags & PTR_DYNAMIC_VERTEX_NORMALS) != 0u;
    std::vector<MeshSource> src(count);
    std::vector<DynMeshRow> rows(count);
    // the arrays k_dyn_check_finite looks at, in the order a refusal names them: per named mesh positions, normals, tangents
    struct Checked {
        uint32_t entry;      // of the list
        const char* what;
        bool computed;       // normals this call computes: the row's pointer is set once the scratch is there
    };
    std::vector<DynCheckRow> checks;
    std::vector<Checked> checked;
    std::vector<size_t> computedAt(count, 0);   // per entry whose normals are computed: where, in floats of the scratch
    size_t computedFloats = 0;
    uint64_t largest = 0;
    try {
        std::vector<uint8_t> named(meshCount, 0);
        for (uint32_t i = 0; i < count; ++i) {
            const PtrMeshVerticesDevice& mv = meshes[i];
            const std::string problem = namedMeshProblem(dyn, mv, named, computes, " (computing them needs a scene uploaded with PTR_DYNAMIC_VERTEX_NORMALS)", src[i].used);
            if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
            rows[i] = dyn.meshRows[mv.meshIndex];
            if (!src[i].used) continue;
            const size_t n = mv.vertexCount;
            const struct {
                const float* data;
                size_t floats;
                const char* what;
                bool computedIfNull;
            } given[3] = {{mv.positions, n * 3u, "position", false}, {mv.normals, n * 3u, "normal", true}, {mv.tangents, n * 4u, "tangent", false}};
            for (const auto& g : given) {
                if (!g.data && !g.computedIfNull) continue;   // (no tangents: the mesh carries none)
                if (g.data) {
                    const std::string bad = devicePointerProblem(g.data, g.floats * sizeof(float), scene->device);
                    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": the " + g.what + " array of mesh " + std::to_string(mv.meshIndex) + " " + bad);
                }
                checks.push_back(DynCheckRow{g.data, g.floats});
                checked.push_back(Checked{i, g.what, !g.data});
                largest = std::max<uint64_t>(largest, g.floats);
            }
            if (!mv.normals) computedAt[i] = computedFloats, computedFloats += n * 3u;
            // (an untextured scene keeps no tangents: they are checked and dropped)
            src[i].v = DynVertexArrays{mv.positions, mv.normals, dyn.meshHasTangents[mv.meshIndex] ? mv.tangents : nullptr};
        }
        if (pastIndexLimit(checks.size())) return refuse(err, err_cap, std::string(who) + ": too many meshes in one call");
    }
    PTR_CATCH_ALL(err, err_cap)

    return deviceCall(who, scene, true, err, err_cap, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (computedFloats) dyn.computedNormals.ensure(computedFloats);
        for (size_t r = 0; r < checks.size(); ++r) {
            if (!checked[r].computed) continue;
            const uint32_t i = checked[r].entry;
            src[i].v.normals = checks[r].data = dyn.computedNormals.ptr + computedAt[i];
        }
        // the check rows ride behind the mesh rows of the table (both are 16 B units)
        dyn.meshTable.ensure(static_cast<size_t>(count) * kDynMeshVec4 + checks.size());
        HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, rows.data(), rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
        const DynCheckRow* dChecks = reinterpret_cast<const DynCheckRow*>(dyn.meshTable.ptr + static_cast<size_t>(count) * kDynMeshVec4);
        const size_t words = (checks.size() + 31u) / 32u;
        if (!checks.empty()) {
            HIP_CHECK(hipMemcpyAsync(const_cast<DynCheckRow*>(dChecks), checks.data(), checks.size() * sizeof(DynCheckRow), hipMemcpyHostToDevice, st));
            dyn.checkFlags.ensure(words);
            HIP_CHECK(hipMemsetAsync(dyn.checkFlags.ptr, 0, words * sizeof(uint32_t), st));
        }
        HIP_CHECK(hipEventRecord(dyn.events[0], st));
        for (uint32_t i = 0; i < count; ++i) {
            if (!src[i].used || meshes[i].normals) continue;
            const uint32_t m = meshes[i].meshIndex;
            const size_t first = dyn.meshTriOffsets[m];
            launchDynVertexNormals(meshes[i].positions, dyn.adjOffsets.ptr + dyn.adjBase[m], dyn.adjEntries.ptr + first * 3u, dyn.meshCorners.ptr + first * 3u,
                                   dyn.computedNormals.ptr + computedAt[i], meshes[i].vertexCount, st);
        }
        if (!checks.empty()) {
            // nothing the renderer reads has been written yet: the flag words come back first, and a set bit ends the call here
            launchDynCheckFinite(dChecks, static_cast<uint32_t>(checks.size()), largest, dyn.checkFlags.ptr, st);
            const uint32_t* flags = static_cast<const uint32_t*>(dyn.pinnedFor(words * sizeof(uint32_t)));
            HIP_CHECK(hipMemcpyAsync(dyn.pinned, dyn.checkFlags.ptr, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            for (size_t r = 0; r < checks.size(); ++r) {
                if (flags[r >> 5] >> (r & 31u) & 1u) {
                    throw HipError{std::string(who) + ": mesh " + std::to_string(meshes[checked[r].entry].meshIndex) + " has a non-finite " + checked[r].what +
                                   " component"};
                }
            }
        }
        gatherBakeFinish(*scene, meshes, src, st, t0, info);
    });
}

int ptr_scene_set_spheres(PtrDeviceScene* scene, const PtrSphereUpdate* spheres, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                          size_t err_cap) {
    return setPrimitives("ptr_scene_set_spheres", 0u, scene, spheres, count, stream, info, err, err_cap);
}

int ptr_scene_set_rects(PtrDeviceScene* scene, const PtrRectUpdate* rects, uint32_t count, void* stream, PtrUpdateInfo* info, char* err, size_t err_cap) {
    return setPrimitives("ptr_scene_set_rects", 1u, scene, rects, count, stream, info, err, err_cap);
}

uint32_t ptr_scene_dynamic_flags(const PtrDeviceScene* scene) { return scene && scene->dynamic ? scene->dynamic->flags : 0u; }

int ptr_debug_dynamic_update_rows(const PtrSceneDesc* scene, uint32_t kind, const void* update, void* out, uint64_t cap_bytes, uint64_t* rows_out,
                                  char* err, size_t err_cap) {
    const char* who = "ptr_debug_dynamic_update_rows";
    if (!scene || !update || !rows_out) return nullArgument(who, err, err_cap);
    if (kind > 1u) return refuse(err, err_cap, std::string(who) + ": no such kind");
    try {
        ptr::PreparedGeometry pg;
        ptr::DynamicTables t;
        t.flags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES;
        prepareGeometry(*scene, pg, &t);
        std::vector<float> lights;
        std::vector<int32_t> lightIndexByRect;
        uint32_t lightCount = 0;
        bool haveTriangles = true;
        buildRectLights(*scene, pg.geo, lights, lightIndexByRect, lightCount, haveTriangles);
        PrimitiveRecords prims;
        fillPrimitiveRecords(*scene, pg.geo, t, lightIndexByRect, prims);
        ScatterRows rows;
        const std::string problem = kind == 0u ? sphereRows(prims, *static_cast<const PtrSphereUpdate*>(update), rows)
                                               : rectRows(prims, *static_cast<const PtrRectUpdate*>(update), rows);
        if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
        const uint64_t n = rows.dest.size();
        *rows_out = n;
        if (!out) return 0;
        if (cap_bytes < n * 20u) return refuse(err, err_cap, std::string(who) + ": the buffer is too small");
        std::memcpy(out, rows.rows.data(), n * 16u);
        std::memcpy(static_cast<char*>(out) + n * 16u, rows.dest.data(), n * 4u);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"

namespace {

// What every update call ends with, after its own kernels (which ran between events 0 and 1 once this has recorded event 1): the refit of
// the float boxes level by level, the grid from the refitted root box, the requantisation and the wide copy; the world bounds the
// background cull reads; the figures of PtrUpdateInfo.
void finishUpdate(PtrDeviceScene& ds, hipStream_t st, std::chrono::steady_clock::time_point t0, uint64_t moved, PtrUpdateInfo* info) {
    DynamicScene& dyn = *ds.dynamic;
    SceneView& v = ds.view;
    {
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
    }
}

bool allFinite(const float* p, int n) {
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(p[i])) return false;
    }
    return true;
}

void putRow(ScatterRows& out, uint32_t array, size_t row, const float* src) {
    out.rows.insert(out.rows.end(), src, src + 4);
    out.dest.push_back((array << kScatterArrayShift) | static_cast<uint32_t>(row));
}

void putBounds(ScatterRows& out, uint32_t array, size_t slot, const ptr::BuildPrim& p) {
    const float lo[4] = {p.lo[0], p.lo[1], p.lo[2], 0.0f}, hi[4] = {p.hi[0], p.hi[1], p.hi[2], 0.0f};
    putRow(out, array, slot * 2u, lo);
    putRow(out, array, slot * 2u + 1u, hi);
}

std::string sphereRows(PrimitiveRecords& prims, const PtrSphereUpdate& u, ScatterRows& out) {
    const std::string name = "sphere " + std::to_string(u.sphereIndex);
    if (u.sphereIndex >= prims.spheres.size()) {
        return "sphere index " + std::to_string(u.sphereIndex) + " out of range (the scene has " + std::to_string(prims.spheres.size()) + " spheres)";
    }
    if (!allFinite(u.centerRadius, 4)) return name + " has a non-finite entry";
    PtrSphere s = prims.spheres[u.sphereIndex];
    std::memcpy(s.centerRadius, u.centerRadius, 16);
    float row[4];
    ptr::BuildPrim prim{};
    ptr::WriteSphere(s, row, prim);
    const size_t slot = prims.sphereLeaf[u.sphereIndex];
    putRow(out, PTR_SCATTER_SPHERES, slot, row);
    putBounds(out, PTR_SCATTER_SPHERE_BOUNDS, slot, prim);
    prims.spheres[u.sphereIndex] = s;
    return "";
}

std::string rectRows(PrimitiveRecords& prims, const PtrRectUpdate& u, ScatterRows& out) {
    const std::string name = "rectangle " + std::to_string(u.rectIndex);
    if (u.rectIndex >= prims.rects.size()) {
        return "rectangle index " + std::to_string(u.rectIndex) + " out of range (the scene has " + std::to_string(prims.rects.size()) + " rectangles)";
    }
    if (!allFinite(u.corner, 4) || !allFinite(u.edgeU, 4) || !allFinite(u.edgeV, 4) || !allFinite(u.normalAndPlane, 4)) return name + " has a non-finite entry";
    const ptr::float3 eu{u.edgeU[0], u.edgeU[1], u.edgeU[2]}, ev{u.edgeV[0], u.edgeV[1], u.edgeV[2]};
    const ptr::float3 n{u.normalAndPlane[0], u.normalAndPlane[1], u.normalAndPlane[2]};
    if (!(ptr::length(ptr::cross(eu, ev)) > 0.0f)) return name + " has cross(edgeU, edgeV) of length zero";
    if (!(ptr::length(n) > 0.0f)) return name + " has a normal of length zero";
    const uint32_t i = u.rectIndex;
    PtrRect r = prims.rects[i];
    std::memcpy(r.corner, u.corner, 16);
    std::memcpy(r.edgeU, u.edgeU, 16);
    std::memcpy(r.edgeV, u.edgeV, 16);
    std::memcpy(r.normalAndPlane, u.normalAndPlane, 16);
    float tri[2][12], nrm[2][12];
    ptr::BuildPrim half[2];
    ptr::WriteRectTriangles(r, i, prims.rectShadeKey[i], tri, nrm, half);
    const uint32_t slots[2] = {prims.rectTriLeaf[static_cast<size_t>(i) * 2u], prims.rectTriLeaf[static_cast<size_t>(i) * 2u + 1u]};
    for (int h = 0; h < 2; ++h) {
        if (slots[h] == 0xFFFFFFFFu) continue;   // (a half the geometry does not hold has no rows)
        for (size_t c = 0; c < 3; ++c) {
            putRow(out, PTR_SCATTER_TRIS, static_cast<size_t>(slots[h]) * 3u + c, &tri[h][c * 4]);
            putRow(out, PTR_SCATTER_TRI_NORMALS, static_cast<size_t>(slots[h]) * 3u + c, &nrm[h][c * 4]);
        }
        putBounds(out, PTR_SCATTER_TRI_BOUNDS, slots[h], half[h]);
    }
    float row[20];
    ptr::WriteRectRow(r, row);
    for (size_t q = 0; q < 5; ++q) putRow(out, PTR_SCATTER_RECTS, static_cast<size_t>(i) * 5u + q, &row[q * 4]);
    const int32_t light = prims.lightIndexByRect[i];
    if (light >= 0) {
        const bool haveTris = slots[0] != 0xFFFFFFFFu && slots[1] != 0xFFFFFFFFu;
        float lrow[ptr::kRectLightFloats];
        ptr::WriteRectLightRow(r, i, &prims.rectEmission[static_cast<size_t>(i) * 3u], haveTris ? tri[0] : nullptr, haveTris ? tri[1] : nullptr, lrow);
        for (size_t q = 0; q < kRectLightVec4; ++q) putRow(out, PTR_SCATTER_RECT_LIGHTS, static_cast<size_t>(light) * kRectLightVec4 + q, &lrow[q * 4]);
    }
    prims.rects[i] = r;
    return "";
}

// ptr_scene_set_spheres (kind 0) and ptr_scene_set_rects (kind 1): the rows on the host, one copy, one scatter, the refit
int setPrimitives(const char* who, uint32_t kind, PtrDeviceScene* scene, const void* list, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                  size_t err_cap) {
    if (!scene) return nullArgument(who, err, err_cap);
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_PRIMITIVES)) {
        return refuse(err, err_cap, std::string(who) + ": the scene does not keep its primitives (upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_PRIMITIVES)");
    }
    if (!list) return refuse(err, err_cap, std::string(who) + ": null list");
    if (count == 0u) return refuse(err, err_cap, std::string(who) + ": count is 0");
    DynamicScene& dyn = *scene->dynamic;
    ScatterRows rows;
    PrimitiveRecords next;
    try {
        next = dyn.prims;   // the records change only when the whole call is accepted
        std::vector<uint8_t> named(kind == 0u ? next.spheres.size() : next.rects.size(), 0);
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t index = kind == 0u ? static_cast<const PtrSphereUpdate*>(list)[i].sphereIndex : static_cast<const PtrRectUpdate*>(list)[i].rectIndex;
            if (index < named.size() && named[index]++) {
                return refuse(err, err_cap, std::string(who) + ": " + (kind == 0u ? "sphere" : "rectangle") + " index " + std::to_string(index) + " named twice");
            }
            const std::string problem = kind == 0u ? sphereRows(next, static_cast<const PtrSphereUpdate*>(list)[i], rows)
                                                   : rectRows(next, static_cast<const PtrRectUpdate*>(list)[i], rows);
            if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
        }
    }
    PTR_CATCH_ALL(err, err_cap)

    return deviceCall(who, scene, true, err, err_cap, [&] {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = static_cast<hipStream_t>(stream);
        PtrDeviceScene& ds = *scene;
        const size_t n = rows.dest.size();
        char* pinned = static_cast<char*>(dyn.pinnedFor(std::max<size_t>(n, 1u) * 20u));
        std::memcpy(pinned, rows.rows.data(), n * 16u);
        std::memcpy(pinned + n * 16u, rows.dest.data(), n * 4u);
        dyn.staging.ensure(n + (n + 3u) / 4u);
        HIP_CHECK(hipMemcpyAsync(dyn.staging.ptr, pinned, n * 20u, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(dyn.events[0], st));
        const size_t tris = dyn.triCount, spheres = dyn.sphereCount;
        DynScatterTargets t{};
        auto target = [&](uint32_t array, float4* base, size_t rowCount) { t.base[array] = base, t.rows[array] = static_cast<uint32_t>(rowCount); };
        target(PTR_SCATTER_TRIS, ds.tris.ptr, tris * 3u);
        target(PTR_SCATTER_TRI_NORMALS, ds.triNormals.ptr, tris * 3u);
        target(PTR_SCATTER_TRI_BOUNDS, dyn.triBounds.ptr, tris * 2u);
        target(PTR_SCATTER_SPHERES, ds.spheres.ptr, spheres);
        target(PTR_SCATTER_SPHERE_BOUNDS, dyn.sphereBounds.ptr, spheres * 2u);
        target(PTR_SCATTER_RECTS, ds.rects.ptr, dyn.prims.rects.size() * 5u);
        target(PTR_SCATTER_RECT_LIGHTS, ds.rectLights.ptr, static_cast<size_t>(ds.view.rectLightCount) * kRectLightVec4);
        launchDynScatterRows(t, dyn.staging.ptr, reinterpret_cast<const uint32_t*>(dyn.staging.ptr + n), static_cast<uint32_t>(n), st);
        dyn.prims = std::move(next);
        finishUpdate(ds, st, t0, kind == 1u ? static_cast<uint64_t>(count) * 2u : 0u, info);
    });
}

}  // namespace

extern "C" {

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
        case PTR_SCENE_ARRAY_RECTS: src = ds.rects.ptr, bytes = static_cast<uint64_t>(ds.view.rectCount) * 80u; break;
        case PTR_SCENE_ARRAY_RECT_LIGHTS: src = ds.rectLights.ptr, bytes = static_cast<uint64_t>(ds.view.rectLightCount) * kRectLightVec4 * 16u; break;
        case PTR_SCENE_ARRAY_SPHERES: src = ds.spheres.ptr, bytes = spheres * 16u; break;
        case PTR_SCENE_ARRAY_OBJ_POS: src = dyn ? dyn->objPos.ptr : nullptr, bytes = dyn ? tris * 48u : 0u; break;
        case PTR_SCENE_ARRAY_OBJ_NRM: src = dyn ? dyn->objNrm.ptr : nullptr, bytes = dyn ? tris * 48u : 0u; break;
        case PTR_SCENE_ARRAY_OBJ_TAN: src = dyn ? dyn->objTan.ptr : nullptr, bytes = dyn && dyn->textured ? tris * 48u : 0u; break;
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

int ptr_debug_vertex_adjacency(const PtrSceneDesc* scene, uint32_t mesh, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err, size_t err_cap) {
    const char* who = "ptr_debug_vertex_adjacency";
    if (!scene || !size_out) return nullArgument(who, err, err_cap);
    if (mesh >= scene->meshCount) return refuse(err, err_cap, std::string(who) + ": mesh index out of range");
    try {
        ptr::PreparedGeometry pg;
        ptr::DynamicTables t;
        t.flags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS;
        prepareGeometry(*scene, pg, &t);
        const size_t offsets = static_cast<size_t>(t.adjBase[mesh + 1u] - t.adjBase[mesh]);
        const size_t entries = static_cast<size_t>(t.meshTriOffsets[mesh + 1u] - t.meshTriOffsets[mesh]) * 3u;
        *size_out = (offsets + entries) * 4u;
        if (!out) return 0;
        if (cap_bytes < *size_out) return refuse(err, err_cap, std::string(who) + ": the buffer is too small");
        std::memcpy(out, t.adjOffsets.data() + t.adjBase[mesh], offsets * 4u);
        if (entries) std::memcpy(static_cast<char*>(out) + offsets * 4u, t.adjEntries.data() + static_cast<size_t>(t.meshTriOffsets[mesh]) * 3u, entries * 4u);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_debug_dynamic_tables(const PtrSceneDesc* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err, size_t err_cap) {
    if (!scene || !size_out) return nullArgument("ptr_debug_dynamic_tables", err, err_cap);
    try {
        ptr::PreparedGeometry pg;
        ptr::DynamicTables t;
        t.flags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES;
        prepareGeometry(*scene, pg, &t);
        const ptr::FlatBvh& bvh = pg.geo.bvh;
        std::vector<uint32_t> words;
        std::vector<float> lights;
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
            case PTR_DYNAMIC_TABLE_MESH_CORNERS: take(t.meshCorners.data(), t.meshCorners.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_RECT_TRI_LEAF: take(pg.geo.rectTriLeaf.data(), pg.geo.rectTriLeaf.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_SPHERE_LEAF: take(t.sphereLeaf.data(), t.sphereLeaf.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_TRIS: take(pg.geo.triData.data(), pg.geo.triData.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_TRI_NORMALS: take(pg.geo.triNormals.data(), pg.geo.triNormals.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_SPHERES: take(pg.geo.sphereData.data(), pg.geo.sphereData.size() * 4u); break;
            case PTR_DYNAMIC_TABLE_RECTS: take(scene->rects, static_cast<size_t>(scene->rectCount) * sizeof(PtrRect)); break;
            case PTR_DYNAMIC_TABLE_RECT_LIGHTS: {
                std::vector<int32_t> lightIndexByRect;
                uint32_t lightCount = 0;
                bool haveTriangles = true;
                buildRectLights(*scene, pg.geo, lights, lightIndexByRect, lightCount, haveTriangles);
                take(lights.data(), lights.size() * 4u);
                break;
            }
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
