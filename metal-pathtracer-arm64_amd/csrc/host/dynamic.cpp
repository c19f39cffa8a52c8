// Dynamic scenes (include/ptr_dynamic.h, include/ptr_deform.h, include/ptr_deform_device.h): the upload of the extra device data,
// ptr_scene_set_mesh_transforms, ptr_scene_set_mesh_vertices and its device-pointer form, ptr_scene_set_spheres and ptr_scene_set_rects,
// which all end in the same refit (finishUpdate), and the headers' test-only probes, which look at a scene's arrays.  Every update call
// is a check half (the rules, on the host) and a run half (the device work on one scene and one stream), declared in dynamic_host.h: the
// frame on several devices (multi_dynamic.cpp) checks once and runs on every partition.  Compiled with hipcc (host code only), like
// hip_backend.cpp; the kernels are in kernels/dynamic.hip.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "../kernels/bvh_grid.h"
#include "../kernels/dynamic.h"
#include "device_scene.h"
#include "dynamic_host.h"
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

void fillPrimitiveRecords(const PtrSceneDesc& desc, const ptr::SceneGeometry& geo, const ptr::DynamicTables& t, const ptr::RectLightTable& lights,
                          PrimitiveRecords& out) {
    out = PrimitiveRecords{};
    out.rectTriLeaf = geo.rectTriLeaf;
    out.sphereLeaf = t.sphereLeaf;
    out.rectShadeKey = t.rectShadeKey;
    out.lightIndexByRect = lights.lightIndexByRect;
    out.rectEmission = lights.rectEmission;
    out.rects.assign(desc.rects, desc.rects + desc.rectCount);
    out.spheres.assign(desc.spheres, desc.spheres + desc.sphereCount);
    out.triCount = geo.triCount;
}

void fillDynamicRecords(const PtrSceneDesc& desc, const ptr::PreparedGeometry& pg, const ptr::DynamicTables& t, const ptr::RectLightTable& lights,
                        DynamicScene& dyn) {
    const ptr::FlatBvh& bvh = pg.geo.bvh;
    dyn.meshTriOffsets = t.meshTriOffsets;
    dyn.levelOffsets = t.levelOffsets;
    dyn.meshHasTangents = t.meshHasTangents;
    dyn.nodeCount = bvh.nodeCount;
    dyn.wideCount = pg.wideCount;
    dyn.triCount = pg.geo.triCount;
    dyn.sphereCount = pg.geo.sphereCount;
    dyn.meanPrimExtent = bvh.meanPrimExtent;
    dyn.meshRows.resize(t.meshBakes.size());
    for (size_t m = 0; m < t.meshBakes.size(); ++m) dyn.meshRows[m] = meshRowOf(t.meshBakes[m], t.meshHasTangents[m] != 0);
    dyn.flags = t.flags;
    if (t.flags & PTR_DYNAMIC_DEFORMABLE) {
        dyn.meshVertexCount = t.meshVertexCount;
        dyn.meshTangentsGiven = t.meshTangentsGiven;
    }
    if (t.flags & PTR_DYNAMIC_VERTEX_NORMALS) dyn.adjBase = t.adjBase;
    if (t.flags & PTR_DYNAMIC_PRIMITIVES) fillPrimitiveRecords(desc, pg.geo, t, lights, dyn.prims);
    ptr::BuildLeafTable(bvh.nodes.data(), bvh.nodeCount, dyn.leafTable);   // include/ptr_rebuild.h, step 1
}

void uploadDynamicTables(const PtrSceneDesc& desc, const PreparedScene& ps, PtrDeviceScene& ds) {
    const ptr::DynamicTables& t = ps.dyn;
    const ptr::FlatBvh& bvh = ps.pg.geo.bvh;
    auto dyn = std::make_unique<DynamicScene>();
    fillDynamicRecords(desc, ps.pg, t, ps.rectLights, *dyn);
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
    if (t.flags & PTR_DYNAMIC_DEFORMABLE) dyn->meshCorners.upload(t.meshCorners.data(), t.meshCorners.size());
    if (t.flags & PTR_DYNAMIC_VERTEX_NORMALS) {
        dyn->adjOffsets.upload(t.adjOffsets.data(), t.adjOffsets.size());
        dyn->adjEntries.upload(t.adjEntries.data(), t.adjEntries.size());
    }
    for (hipEvent_t& e : dyn->events) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&dyn->rootBox), 4 * sizeof(float4), hipHostMallocDefault));
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

// (defined below the entry points)
void finishUpdate(PtrDeviceScene& ds, hipStream_t st, std::chrono::steady_clock::time_point t0, uint64_t moved, PtrUpdateInfo* info);
// The host half of a sphere's / a rectangle's move: the new record into `prims`, its rows appended to `out`.  "" or what is wrong with it.
// named: per sphere / rectangle of the scene, whether the list has named it so far.
std::string sphereRows(PrimitiveRecords& prims, const PtrSphereUpdate& u, std::vector<uint8_t>& named, ScatterRows& out);
std::string rectRows(PrimitiveRecords& prims, const PtrRectUpdate& u, std::vector<uint8_t>& named, ScatterRows& out);

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

// What both vertex calls refuse about entry `mv` of their list (PtrMeshVertices and PtrMeshVerticesDevice have the same members): "" or the
// cause.  named: per mesh of the scene, whether the list has named it so far.  used: the mesh has triangles.
template <typename V>
std::string namedMeshProblem(const DynamicScene& dyn, const V& mv, std::vector<uint8_t>& named, bool normalsMayBeNull, const char* nullNormalsHint, bool& used) {
    used = false;
    const std::string bad = ptr::NamedIndexProblem("mesh", "meshes", mv.meshIndex, named);
    if (!bad.empty()) return bad;
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

// What both vertex calls run once the mesh table is on the device and event 0 is recorded: per named mesh with triangles (entry i: used,
// mesh, and through arraysOf where the gather reads its arrays) the gather into the object-space corner rows and the bake under the matrix
// the mesh has (row i of the table), then the shared tail.
template <typename E, typename ArraysOf>
void gatherBakeFinish(PtrDeviceScene& ds, const std::vector<E>& entry, ArraysOf&& arraysOf, hipStream_t st, std::chrono::steady_clock::time_point t0,
                      PtrUpdateInfo* info) {
    DynamicScene& dyn = *ds.dynamic;
    const DynBakeArrays arrays = bakeArrays(ds);
    uint64_t moved = 0;
    for (uint32_t i = 0; i < entry.size(); ++i) {
        if (!entry[i].used) continue;
        const uint32_t m = entry[i].mesh;
        const uint32_t first = dyn.meshTriOffsets[m], n = dyn.meshTriOffsets[m + 1u] - first;
        launchDynGatherCorners(dyn.objPos.ptr, dyn.objNrm.ptr, dyn.textured ? dyn.objTan.ptr : nullptr, arraysOf(entry[i]), dyn.meshTris.ptr + first,
                               dyn.meshCorners.ptr + static_cast<size_t>(first) * 3u, n, st);
        launchDynBake(arrays, dyn.meshTable.ptr, i, dyn.meshTris.ptr + first, n, st);
        moved += n;
    }
    finishUpdate(ds, st, t0, moved, info);
}

const char* const kNotDynamic = "the scene is not dynamic (upload it with ptr_scene_upload_dynamic)";
const char* const kNotDeformable = "the scene is not deformable (upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_DEFORMABLE)";

// firstNonFinite over `rows`, whose row r is u.checked[index[r]]: a flagged row ends the call - nothing the renderer reads has been written yet
void finiteCheck(const char* who, const DeviceVerticesUpdate& u, const std::vector<DynCheckRow>& rows, const std::vector<size_t>& index, DynCheckRow* dRows,
                 uint32_t* dFlags, uint32_t* pinnedFlags, hipStream_t st) {
    const int bad = firstNonFinite(rows.data(), rows.size(), dRows, dFlags, pinnedFlags, st);
    if (bad < 0) return;
    const DeviceVerticesUpdate::Checked& c = u.checked[index[static_cast<size_t>(bad)]];
    throw Refused{std::string(who) + ": mesh " + std::to_string(u.entry[c.entry].mesh) + " has a non-finite " + c.what + " component"};
}

}  // namespace

namespace ptrhost {

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

int firstNonFinite(const DynCheckRow* rows, size_t n, DynCheckRow* dRows, uint32_t* dFlags, uint32_t* pinnedFlags, hipStream_t st) {
    const size_t words = (n + 31u) / 32u;
    uint64_t largest = 0;
    for (size_t r = 0; r < n; ++r) largest = std::max<uint64_t>(largest, rows[r].count);
    HIP_CHECK(hipMemcpyAsync(dRows, rows, n * sizeof(DynCheckRow), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(dFlags, 0, words * sizeof(uint32_t), st));
    launchDynCheckFinite(dRows, static_cast<uint32_t>(n), largest, dFlags, st);
    HIP_CHECK(hipMemcpyAsync(pinnedFlags, dFlags, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t r = 0; r < n; ++r) {
        if (pinnedFlags[r >> 5] >> (r & 31u) & 1u) return static_cast<int>(r);
    }
    return -1;
}

std::string listProblem(const void* list, uint32_t count, const char* nullWords) {
    if (!list) return nullWords;
    if (count == 0u) return "count is 0";
    return "";
}

std::string checkMeshTransforms(const PtrDeviceScene* scene, const PtrMeshTransform* transforms, uint32_t count, TransformUpdate& out) {
    if (!scene->dynamic) return kNotDynamic;
    const std::string bad = listProblem(transforms, count, "null transform list");
    if (!bad.empty()) return bad;
    const DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    out.mesh.resize(count), out.rows.resize(count);
    std::vector<uint8_t> named(meshCount, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const PtrMeshTransform& t = transforms[i];
        const std::string bad = ptr::NamedIndexProblem("mesh", "meshes", t.meshIndex, named);
        if (!bad.empty()) return bad;
        ptr::MeshBake bake;
        ptr::ComputeMeshBake(t.localToWorld, bake);
        const std::string problem = matrixProblem(t.localToWorld, bake);
        if (!problem.empty()) return "the matrix of mesh " + std::to_string(t.meshIndex) + " " + problem;
        out.mesh[i] = t.meshIndex;
        out.rows[i] = meshRowOf(bake, dyn.meshHasTangents[t.meshIndex] != 0);
    }
    return "";
}

void runMeshTransforms(PtrDeviceScene& ds, const TransformUpdate& u, hipStream_t st, PtrUpdateInfo* info, const InputsEnqueued& enqueued) {
    const auto t0 = std::chrono::steady_clock::now();
    DynamicScene& dyn = *ds.dynamic;
    const uint32_t count = static_cast<uint32_t>(u.rows.size());
    dyn.meshTable.ensure(static_cast<size_t>(count) * kDynMeshVec4);
    HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, u.rows.data(), u.rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(dyn.events[0], st));
    if (enqueued) enqueued();
    const DynBakeArrays arrays = bakeArrays(ds);
    uint64_t moved = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t m = u.mesh[i];
        const uint32_t first = dyn.meshTriOffsets[m], n = dyn.meshTriOffsets[m + 1u] - first;
        launchDynBake(arrays, dyn.meshTable.ptr, i, dyn.meshTris.ptr + first, n, st);
        dyn.meshRows[m] = u.rows[i];   // the matrix a later ptr_scene_set_mesh_vertices bakes under
        moved += n;
    }
    finishUpdate(ds, st, t0, moved, info);
}

std::string checkMeshVertices(const PtrDeviceScene* scene, const PtrMeshVertices* meshes, uint32_t count, VerticesUpdate& out) {
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_DEFORMABLE)) return kNotDeformable;
    const std::string bad = listProblem(meshes, count, "null mesh list");
    if (!bad.empty()) return bad;
    const DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    out.entry.assign(count, VerticesUpdate::Entry{});
    out.rows.resize(count);
    // where the arrays of every named mesh go in the staging buffer, in floats (a mesh without triangles stages nothing)
    size_t floats = 0;
    std::vector<uint8_t> named(meshCount, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const PtrMeshVertices& mv = meshes[i];
        VerticesUpdate::Entry& s = out.entry[i];
        const std::string problem = namedMeshProblem(dyn, mv, named, false, "", s.used);
        if (!problem.empty()) return problem;
        s.mesh = mv.meshIndex;
        out.rows[i] = dyn.meshRows[mv.meshIndex];
        if (!s.used) continue;
        s.hasTangents = dyn.meshHasTangents[mv.meshIndex] != 0;   // (an untextured scene keeps no tangents: they are checked and dropped)
        s.positions = floats, floats += static_cast<size_t>(mv.vertexCount) * 3u;
        s.normals = floats, floats += static_cast<size_t>(mv.vertexCount) * 3u;
        if (s.hasTangents) s.tangents = floats, floats += static_cast<size_t>(mv.vertexCount) * 4u;
    }
    out.floats = floats;
    return "";
}

std::string stageMeshVertices(const PtrMeshVertices* meshes, const VerticesUpdate& u, float* pinned) {
    for (uint32_t i = 0; i < u.entry.size(); ++i) {
        const PtrMeshVertices& mv = meshes[i];
        const VerticesUpdate::Entry& s = u.entry[i];
        if (!s.used) continue;
        const size_t n = mv.vertexCount;
        const char* bad = nullptr;
        if (!stageFinite(mv.positions, n * 3u, pinned + s.positions)) bad = "position";
        else if (!stageFinite(mv.normals, n * 3u, pinned + s.normals)) bad = "normal";
        else if (mv.tangents) {
            std::vector<float> dropped;
            if (!s.hasTangents) dropped.resize(n * 4u);
            if (!stageFinite(mv.tangents, n * 4u, s.hasTangents ? pinned + s.tangents : dropped.data())) bad = "tangent";
        }
        if (bad) return "mesh " + std::to_string(mv.meshIndex) + " has a non-finite " + bad + " component";
    }
    return "";
}

void runMeshVertices(PtrDeviceScene& ds, const VerticesUpdate& u, const float* pinned, hipStream_t st, PtrUpdateInfo* info, const InputsEnqueued& enqueued) {
    const auto t0 = std::chrono::steady_clock::now();
    DynamicScene& dyn = *ds.dynamic;
    dyn.staging.ensure((u.floats + 3u) / 4u);
    const float* dStaged = reinterpret_cast<const float*>(dyn.staging.ptr);
    if (u.floats) HIP_CHECK(hipMemcpyAsync(dyn.staging.ptr, pinned, u.floats * sizeof(float), hipMemcpyHostToDevice, st));
    dyn.meshTable.ensure(u.rows.size() * kDynMeshVec4);
    HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, u.rows.data(), u.rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(dyn.events[0], st));
    if (enqueued) enqueued();
    gatherBakeFinish(ds, u.entry,
                     [&](const VerticesUpdate::Entry& s) {
                         return DynVertexArrays{dStaged + s.positions, dStaged + s.normals, s.hasTangents ? dStaged + s.tangents : nullptr};
                     },
                     st, t0, info);
}

std::string checkMeshVerticesDevice(const PtrDeviceScene* scene, const PtrMeshVerticesDevice* meshes, uint32_t count, int arraysDevice,
                                    DeviceVerticesUpdate& out) {
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_DEFORMABLE)) return kNotDeformable;
    const std::string badList = listProblem(meshes, count, "null mesh list");
    if (!badList.empty()) return badList;
    const DynamicScene& dyn = *scene->dynamic;
    const uint32_t meshCount = static_cast<uint32_t>(dyn.meshTriOffsets.size()) - 1u;
    const bool computes = (dyn.flags & PTR_DYNAMIC_VERTEX_NORMALS) != 0u;
    out.entry.assign(count, DeviceVerticesUpdate::Entry{});
    out.rows.resize(count);
    std::vector<uint8_t> named(meshCount, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const PtrMeshVerticesDevice& mv = meshes[i];
        DeviceVerticesUpdate::Entry& e = out.entry[i];
        const std::string problem = namedMeshProblem(dyn, mv, named, computes, " (computing them needs a scene uploaded with PTR_DYNAMIC_VERTEX_NORMALS)", e.used);
        if (!problem.empty()) return problem;
        e.mesh = mv.meshIndex, e.vertexCount = mv.vertexCount;
        out.rows[i] = dyn.meshRows[mv.meshIndex];
        if (!e.used) continue;
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
                const std::string bad = devicePointerProblem(g.data, g.floats * sizeof(float), arraysDevice);
                if (!bad.empty()) return std::string("the ") + g.what + " array of mesh " + std::to_string(mv.meshIndex) + " " + bad;
            }
            out.checked.push_back(DeviceVerticesUpdate::Checked{i, g.what, !g.data, g.data, g.floats});
        }
        e.computes = !mv.normals;
        if (e.computes) e.computedAt = out.computedFloats, out.computedFloats += n * 3u;
        // (an untextured scene keeps no tangents: they are checked and dropped)
        e.v = DynVertexArrays{mv.positions, mv.normals, dyn.meshHasTangents[mv.meshIndex] ? mv.tangents : nullptr};
    }
    if (pastIndexLimit(out.checked.size())) return "too many meshes in one call";
    return "";
}

void checkGivenArrays(const char* who, const DeviceVerticesUpdate& u, DeviceBuffer<float4>& dRows, DeviceBuffer<uint32_t>& dFlags, uint32_t* pinnedFlags,
                      hipStream_t st) {
    std::vector<DynCheckRow> rows;
    std::vector<size_t> index;
    for (size_t r = 0; r < u.checked.size(); ++r) {
        if (u.checked[r].computed) continue;
        rows.push_back(DynCheckRow{u.checked[r].data, u.checked[r].floats});
        index.push_back(r);
    }
    if (rows.empty()) return;
    dRows.ensure(rows.size());
    dFlags.ensure((rows.size() + 31u) / 32u);
    finiteCheck(who, u, rows, index, reinterpret_cast<DynCheckRow*>(dRows.ptr), dFlags.ptr, pinnedFlags, st);
}

void runMeshVerticesDevice(const char* who, PtrDeviceScene& ds, const DeviceVerticesUpdate& u, bool checkGiven, hipStream_t st, PtrUpdateInfo* info) {
    const auto t0 = std::chrono::steady_clock::now();
    DynamicScene& dyn = *ds.dynamic;
    const size_t count = u.entry.size();
    if (u.computedFloats) dyn.computedNormals.ensure(u.computedFloats);
    std::vector<DynCheckRow> checks;
    std::vector<size_t> index;
    for (size_t r = 0; r < u.checked.size(); ++r) {
        const DeviceVerticesUpdate::Checked& c = u.checked[r];
        if (!c.computed && !checkGiven) continue;
        checks.push_back(DynCheckRow{c.computed ? dyn.computedNormals.ptr + u.entry[c.entry].computedAt : c.data, c.floats});
        index.push_back(r);
    }
    // the check rows ride behind the mesh rows of the table (both are 16 B units)
    dyn.meshTable.ensure(count * kDynMeshVec4 + checks.size());
    HIP_CHECK(hipMemcpyAsync(dyn.meshTable.ptr, u.rows.data(), u.rows.size() * sizeof(DynMeshRow), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(dyn.events[0], st));
    for (size_t i = 0; i < count; ++i) {
        const DeviceVerticesUpdate::Entry& e = u.entry[i];
        if (!e.used || !e.computes) continue;
        const size_t first = dyn.meshTriOffsets[e.mesh];
        launchDynVertexNormals(e.v.positions, dyn.adjOffsets.ptr + dyn.adjBase[e.mesh], dyn.adjEntries.ptr + first * 3u, dyn.meshCorners.ptr + first * 3u,
                               dyn.computedNormals.ptr + e.computedAt, e.vertexCount, st);
    }
    if (!checks.empty()) {
        const size_t words = (checks.size() + 31u) / 32u;
        dyn.checkFlags.ensure(words);
        finiteCheck(who, u, checks, index, reinterpret_cast<DynCheckRow*>(dyn.meshTable.ptr + count * kDynMeshVec4), dyn.checkFlags.ptr,
                    static_cast<uint32_t*>(dyn.pinned.pinnedFor(words * sizeof(uint32_t))), st);
    }
    gatherBakeFinish(ds, u.entry,
                     [&](const DeviceVerticesUpdate::Entry& e) {
                         return DynVertexArrays{e.v.positions, e.computes ? dyn.computedNormals.ptr + e.computedAt : e.v.normals, e.v.tangents};
                     },
                     st, t0, info);
}

}  // namespace ptrhost

extern "C" {

int ptr_scene_is_dynamic(const PtrDeviceScene* scene) { return scene && scene->dynamic ? 1 : 0; }

int ptr_scene_set_mesh_transforms(PtrDeviceScene* scene, const PtrMeshTransform* transforms, uint32_t count, void* stream, PtrUpdateInfo* info,
                                  char* err, size_t err_cap) {
    TransformUpdate u;
    return updateCall("ptr_scene_set_mesh_transforms", scene, err, err_cap, [&] { return checkMeshTransforms(scene, transforms, count, u); },
                      [&] { runMeshTransforms(*scene, u, static_cast<hipStream_t>(stream), info); });
}

int ptr_scene_set_mesh_vertices(PtrDeviceScene* scene, const PtrMeshVertices* meshes, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                                size_t err_cap) {
    VerticesUpdate u;
    const float* pinned = nullptr;
    return updateCall("ptr_scene_set_mesh_vertices", scene, err, err_cap,
                      [&] {
                          const std::string problem = checkMeshVertices(scene, meshes, count, u);
                          if (!problem.empty()) return problem;
                          // staging: every array into the scene's pinned buffer, each component looked at on the way
                          HIP_CHECK(hipSetDevice(scene->device));
                          float* staged = static_cast<float*>(scene->dynamic->pinned.pinnedFor(std::max<size_t>(u.floats, 4u) * sizeof(float)));
                          pinned = staged;
                          return stageMeshVertices(meshes, u, staged);
                      },
                      [&] { runMeshVertices(*scene, u, pinned, static_cast<hipStream_t>(stream), info); });
}

int ptr_scene_set_mesh_vertices_device(PtrDeviceScene* scene, const PtrMeshVerticesDevice* meshes, uint32_t count, void* stream, PtrUpdateInfo* info,
                                       char* err, size_t err_cap) {
    static const char* const who = "ptr_scene_set_mesh_vertices_device";
    DeviceVerticesUpdate u;
    return updateCall(who, scene, err, err_cap, [&] { return checkMeshVerticesDevice(scene, meshes, count, scene->device, u); },
                      [&] { runMeshVerticesDevice(who, *scene, u, true, static_cast<hipStream_t>(stream), info); });
}

int ptr_scene_set_spheres(PtrDeviceScene* scene, const PtrSphereUpdate* spheres, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                          size_t err_cap) {
    PrimitivesUpdate u;
    return updateCall("ptr_scene_set_spheres", scene, err, err_cap, [&] { return checkPrimitives(0u, scene, spheres, count, u); },
                      [&] { runPrimitives(*scene, u, static_cast<hipStream_t>(stream), info); });
}

int ptr_scene_set_rects(PtrDeviceScene* scene, const PtrRectUpdate* rects, uint32_t count, void* stream, PtrUpdateInfo* info, char* err, size_t err_cap) {
    PrimitivesUpdate u;
    return updateCall("ptr_scene_set_rects", scene, err, err_cap, [&] { return checkPrimitives(1u, scene, rects, count, u); },
                      [&] { runPrimitives(*scene, u, static_cast<hipStream_t>(stream), info); });
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
        PrimitiveRecords prims;
        fillPrimitiveRecords(*scene, pg.geo, t, rectLightsOf(*scene, pg.geo), prims);
        ScatterRows rows;
        std::vector<uint8_t> named(kind == 0u ? prims.spheres.size() : prims.rects.size(), 0);
        const std::string problem = kind == 0u ? sphereRows(prims, *static_cast<const PtrSphereUpdate*>(update), named, rows)
                                               : rectRows(prims, *static_cast<const PtrRectUpdate*>(update), named, rows);
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

std::string sphereRows(PrimitiveRecords& prims, const PtrSphereUpdate& u, std::vector<uint8_t>& named, ScatterRows& out) {
    const std::string name = "sphere " + std::to_string(u.sphereIndex);
    const std::string bad = ptr::NamedIndexProblem("sphere", "spheres", u.sphereIndex, named);
    if (!bad.empty()) return bad;
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

std::string rectRows(PrimitiveRecords& prims, const PtrRectUpdate& u, std::vector<uint8_t>& named, ScatterRows& out) {
    const std::string name = "rectangle " + std::to_string(u.rectIndex);
    const std::string bad = ptr::NamedIndexProblem("rectangle", "rectangles", u.rectIndex, named);
    if (!bad.empty()) return bad;
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

}  // namespace

namespace ptrhost {

// ptr_scene_set_spheres (kind 0) and ptr_scene_set_rects (kind 1): the rows on the host ...
std::string checkPrimitives(uint32_t kind, const PtrDeviceScene* scene, const void* list, uint32_t count, PrimitivesUpdate& out) {
    if (!scene->dynamic || !(scene->dynamic->flags & PTR_DYNAMIC_PRIMITIVES)) {
        return "the scene does not keep its primitives (upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_PRIMITIVES)";
    }
    const std::string bad = listProblem(list, count, "null list");
    if (!bad.empty()) return bad;
    out.kind = kind, out.count = count;
    PrimitiveRecords& next = out.next;
    next = scene->dynamic->prims;   // the records change only when the whole call is accepted
    std::vector<uint8_t> named(kind == 0u ? next.spheres.size() : next.rects.size(), 0);
    for (uint32_t i = 0; i < count; ++i) {
        const std::string problem = kind == 0u ? sphereRows(next, static_cast<const PtrSphereUpdate*>(list)[i], named, out.rows)
                                               : rectRows(next, static_cast<const PtrRectUpdate*>(list)[i], named, out.rows);
        if (!problem.empty()) return problem;
    }
    return "";
}

// ... one copy, one scatter, the refit
void runPrimitives(PtrDeviceScene& ds, const PrimitivesUpdate& u, hipStream_t st, PtrUpdateInfo* info, const InputsEnqueued& enqueued) {
    const auto t0 = std::chrono::steady_clock::now();
    DynamicScene& dyn = *ds.dynamic;
    const ScatterRows& rows = u.rows;
    const size_t n = rows.dest.size();
    char* pinned = static_cast<char*>(dyn.pinned.pinnedFor(std::max<size_t>(n, 1u) * 20u));
    std::memcpy(pinned, rows.rows.data(), n * 16u);
    std::memcpy(pinned + n * 16u, rows.dest.data(), n * 4u);
    dyn.staging.ensure(n + (n + 3u) / 4u);
    HIP_CHECK(hipMemcpyAsync(dyn.staging.ptr, pinned, n * 20u, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(dyn.events[0], st));
    if (enqueued) enqueued();
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
    dyn.prims = u.next;
    finishUpdate(ds, st, t0, u.kind == 1u ? static_cast<uint64_t>(u.count) * 2u : 0u, info);
}

}  // namespace ptrhost

extern "C" {

int ptr_debug_scene_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out) {
    if (!scene || !size_out) return 1;
    const PtrDeviceScene& ds = *scene;
    const DynamicScene* dyn = ds.dynamic.get();
    const uint64_t tris = ds.info[2], spheres = ds.info[3], nodes = ds.info[0];
    float grid[6];
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
        case PTR_SCENE_ARRAY_GRID:
            std::memcpy(grid, ds.view.gridOrigin, 12), std::memcpy(grid + 3, ds.view.gridCell, 12);
            src = grid, bytes = sizeof(grid);
            break;
        case PTR_SCENE_ARRAY_RECTS: src = ds.rects.ptr, bytes = static_cast<uint64_t>(ds.view.rectCount) * 80u; break;
        case PTR_SCENE_ARRAY_RECT_LIGHTS: src = ds.rectLights.ptr, bytes = static_cast<uint64_t>(ds.view.rectLightCount) * kRectLightVec4 * 16u; break;
        case PTR_SCENE_ARRAY_SPHERES: src = ds.spheres.ptr, bytes = spheres * 16u; break;
        case PTR_SCENE_ARRAY_OBJ_POS: src = dyn ? dyn->objPos.ptr : nullptr, bytes = dyn ? tris * 48u : 0u; break;
        case PTR_SCENE_ARRAY_OBJ_NRM: src = dyn ? dyn->objNrm.ptr : nullptr, bytes = dyn ? tris * 48u : 0u; break;
        case PTR_SCENE_ARRAY_OBJ_TAN: src = dyn ? dyn->objTan.ptr : nullptr, bytes = dyn && dyn->textured ? tris * 48u : 0u; break;
        default: return 1;
    }
    return probeArrayTail(ds.device, src, which == PTR_SCENE_ARRAY_GRID, bytes, out, cap_bytes, size_out);
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
            case PTR_DYNAMIC_TABLE_RECT_LIGHTS:
                lights = rectLightsOf(*scene, pg.geo).lights;
                take(lights.data(), lights.size() * 4u);
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
