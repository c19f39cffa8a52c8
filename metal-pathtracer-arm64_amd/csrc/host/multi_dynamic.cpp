// Host side of include/ptr_multi_dynamic.h: a frame on several devices whose scenes are dynamic and are updated in place.  Nothing here
// states a rule or launches a kernel of its own: every call is the check half of the single-device call (dynamic_host.h) against partition
// 0's records, the fan-out of what the kernels read, and the run half on every partition's scene and stream under the partition driver of
// multi_frame_host.h; the steps it shares with multi_appearance.cpp are in multi_update_host.h.  Compiled with hipcc (host code only),
// like multi_frame.cpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "multi_update_host.h"
#include "ptr_multi_dynamic.h"

using namespace ptrhost;
using namespace ptrk;

namespace {

constexpr uint32_t kAllDynamicFlags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS;

// the arrays of a device update that travel (multi_update_host.h); which: 0 positions, 1 normals, 2 tangents
Travel travelOf(const DeviceVerticesUpdate& u) {
    Travel t;
    for (uint32_t i = 0; i < u.entry.size(); ++i) {
        const DeviceVerticesUpdate::Entry& e = u.entry[i];
        if (!e.used) continue;
        const size_t n = e.vertexCount;
        const float* const given[3] = {e.v.positions, e.v.normals, e.v.tangents};
        const size_t width[3] = {3u, 3u, 4u};
        for (int k = 0; k < 3; ++k) {
            if (given[k]) t.add(given[k], n * width[k], i, k);   // (not: computed normals, a mesh or a scene without tangents)
        }
    }
    return t;
}

// the update as a partition sees it whose copy of the travelling arrays starts at `base`
DeviceVerticesUpdate movedTo(const DeviceVerticesUpdate& u, const Travel& t, const float* base) {
    DeviceVerticesUpdate mine = u;
    for (const Travel::Array& a : t.arrays) {
        DynVertexArrays& v = mine.entry[a.entry].v;
        (a.which == 0 ? v.positions : a.which == 1 ? v.normals : v.tangents) = base + a.at;
    }
    return mine;
}

}  // namespace

extern "C" {

int ptr_multi_frame_create_dynamic(const PtrSceneDesc* scene, const PtrSettings* settings, int n_devices, uint32_t dynamic_flags,
                                   PtrMultiFrame** out_frame, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_create_dynamic";
    const std::string problem = dynamicFlagsProblem(dynamic_flags, kAllDynamicFlags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    return createMultiFrame(who, scene, settings, nullptr, 0u, false, nullptr, n_devices, false, true, dynamic_flags, out_frame, err, err_cap);
}

int ptr_multi_frame_debug_create_dynamic_on(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t dynamic_flags, const int* device_ids,
                                            int n, PtrMultiFrame** out_frame, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_debug_create_dynamic_on";
    const std::string problem = dynamicFlagsProblem(dynamic_flags, kAllDynamicFlags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    return createMultiFrame(who, scene, settings, nullptr, 0u, false, device_ids, n, true, true, dynamic_flags, out_frame, err, err_cap);
}

int ptr_multi_frame_is_dynamic(const PtrMultiFrame* frame) { return frame && frame->dynamic ? 1 : 0; }

uint32_t ptr_multi_frame_dynamic_flags(const PtrMultiFrame* frame) { return frame && frame->dynamic ? frame->dynamic->flags : 0u; }

PtrDeviceScene* ptr_multi_frame_part_scene(PtrMultiFrame* frame, uint32_t p) {
    return frame && p < frame->parts ? frame->part[p]->scene.get() : nullptr;
}

int ptr_multi_frame_set_mesh_transforms(PtrMultiFrame* frame, const PtrMeshTransform* transforms, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                        size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_mesh_transforms";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(transforms, count, "null transform list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    TransformUpdate u;
    std::string problem;
    try {
        problem = checkMeshTransforms(frame->part[0]->scene.get(), transforms, count, u);
    }
    PTR_CATCH_ALL(err, err_cap)
    return hostUpdate(who, *frame, t0, problem, info, err, err_cap,
                      [&](PtrDeviceScene& ds, hipStream_t st, PtrUpdateInfo* one, const InputsEnqueued& sent) { runMeshTransforms(ds, u, st, one, sent); });
}

int ptr_multi_frame_set_mesh_vertices(PtrMultiFrame* frame, const PtrMeshVertices* meshes, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                      size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_mesh_vertices";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(meshes, count, "null mesh list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    VerticesUpdate u;
    const float* pinned = nullptr;
    std::string problem;
    try {
        problem = checkMeshVertices(frame->part[0]->scene.get(), meshes, count, u);
        if (problem.empty()) {   // staged once, for every partition
            HIP_CHECK(hipSetDevice(frame->rootDevice));
            float* staged = static_cast<float*>(distributionOf(*frame).pinned.pinnedFor(std::max<size_t>(u.floats, 4u) * sizeof(float)));
            pinned = staged;
            problem = stageMeshVertices(meshes, u, staged);
        }
    }
    PTR_CATCH_ALL(err, err_cap)
    return hostUpdate(who, *frame, t0, problem, info, err, err_cap,
                      [&](PtrDeviceScene& ds, hipStream_t st, PtrUpdateInfo* one, const InputsEnqueued& sent) { runMeshVertices(ds, u, pinned, st, one, sent); });
}

int ptr_multi_frame_set_spheres(PtrMultiFrame* frame, const PtrSphereUpdate* spheres, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_spheres";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(spheres, count, "null list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    PrimitivesUpdate u;
    std::string problem;
    try {
        problem = checkPrimitives(0u, frame->part[0]->scene.get(), spheres, count, u);
    }
    PTR_CATCH_ALL(err, err_cap)
    return hostUpdate(who, *frame, t0, problem, info, err, err_cap, [&](PtrDeviceScene& ds, hipStream_t st, PtrUpdateInfo* one, const InputsEnqueued& sent) { runPrimitives(ds, u, st, one, sent); });
}

int ptr_multi_frame_set_rects(PtrMultiFrame* frame, const PtrRectUpdate* rects, uint32_t count, PtrMultiUpdateInfo* info, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_rects";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(rects, count, "null list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    PrimitivesUpdate u;
    std::string problem;
    try {
        problem = checkPrimitives(1u, frame->part[0]->scene.get(), rects, count, u);
    }
    PTR_CATCH_ALL(err, err_cap)
    return hostUpdate(who, *frame, t0, problem, info, err, err_cap, [&](PtrDeviceScene& ds, hipStream_t st, PtrUpdateInfo* one, const InputsEnqueued& sent) { runPrimitives(ds, u, st, one, sent); });
}

int ptr_multi_frame_set_mesh_vertices_device(PtrMultiFrame* frame, const PtrMeshVerticesDevice* meshes, uint32_t count, int src_device, void* stream,
                                             PtrMultiUpdateInfo* info, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_mesh_vertices_device";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(meshes, count, "null mesh list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (src_device < 0) return refuse(err, err_cap, std::string(who) + ": no such HIP device");
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    PtrMultiFrame& f = *frame;
    DeviceVerticesUpdate u;
    try {
        if (src_device >= ptr_device_count()) return refuse(err, err_cap, std::string(who) + ": no such HIP device");
        const std::string problem = checkMeshVerticesDevice(f.part[0]->scene.get(), meshes, count, src_device, u);
        if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    }
    PTR_CATCH_ALL(err, err_cap)

    try {
        hipStream_t callers = static_cast<hipStream_t>(stream);
        const Travel travel = travelOf(u);
        // the check, once, where the arrays are; a refusal leaves every partition as it was
        const DeviceRoute route = routeFromDevice(f, travel, src_device, callers, "vertex", [&](MultiDistribution& md, MultiDistribution::Source& source) {
            const size_t words = (u.checked.size() + 31u) / 32u;
            checkGivenArrays(who, u, source.rows, source.flags, static_cast<uint32_t*>(md.pinned.pinnedFor(std::max<size_t>(words, 1u) * sizeof(uint32_t))), callers);
        });
        PtrUpdateInfo first{};
        const std::string refused = runUpdate(who, f, t0, info, [&](Part& me, uint32_t p, const auto& arrived) {
            const float* base = bringArrays(route, travel, me, p);
            const DeviceVerticesUpdate mine = base ? movedTo(u, travel, base) : u;
            arrived();
            runMeshVerticesDevice(who, *me.scene, mine, false, me.stream, p == 0u ? &first : nullptr);
        });
        if (!refused.empty()) return refuse(err, err_cap, refused);
        if (info) {
            info->first = first;
            info->stagedParts = route.stagedParts;
        }
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_debug_check_update(const PtrSceneDesc* scene, uint32_t dynamic_flags, uint32_t kind, const void* list, uint32_t count, char* err,
                                       size_t err_cap) {
    static const char* const names[4] = {"ptr_multi_frame_set_mesh_transforms", "ptr_multi_frame_set_mesh_vertices", "ptr_multi_frame_set_spheres",
                                         "ptr_multi_frame_set_rects"};
    const char* who = "ptr_multi_frame_debug_check_update";
    if (!scene) return nullArgument(who, err, err_cap);
    if (kind > 3u) return refuse(err, err_cap, std::string(who) + ": no such kind");
    std::string problem = dynamicFlagsProblem(dynamic_flags, kAllDynamicFlags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    who = names[kind];
    try {
        // the records of an upload without the upload: the preparation of a dynamic scene and the light table, on the host
        ptr::PreparedGeometry pg;
        ptr::DynamicTables t;
        t.flags = dynamic_flags;
        prepareGeometry(*scene, pg, &t);
        PtrDeviceScene ds;
        ds.dynamic = std::make_unique<DynamicScene>();
        fillDynamicRecords(*scene, pg, t, rectLightsOf(*scene, pg.geo), *ds.dynamic);
        if (kind == 0u) {
            TransformUpdate u;
            problem = checkMeshTransforms(&ds, static_cast<const PtrMeshTransform*>(list), count, u);
        } else if (kind == 1u) {
            VerticesUpdate u;
            problem = checkMeshVertices(&ds, static_cast<const PtrMeshVertices*>(list), count, u);
            std::vector<float> staged(std::max<size_t>(u.floats, 4u));
            if (problem.empty()) problem = stageMeshVertices(static_cast<const PtrMeshVertices*>(list), u, staged.data());
        } else {
            PrimitivesUpdate u;
            problem = checkPrimitives(kind - 2u, &ds, list, count, u);
        }
        setErr(err, err_cap, "");
        return problem.empty() ? 0 : refuse(err, err_cap, std::string(who) + ": " + problem);
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_tree_cost(PtrMultiFrame* frame, double* cost, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_tree_cost";
    if (!frame || !cost) return nullArgument(who, err, err_cap);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    Part& first = *frame->part[0];
    const std::string problem = checkTreeCall(first.scene.get(), 0u);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    return deviceCall(who, first.scene.get(), true, err, err_cap, [&] { *cost = treeCost(*first.scene, first.stream); });
}

int ptr_multi_frame_rebuild_tree(PtrMultiFrame* frame, uint32_t flags, PtrRebuildInfo* info, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_rebuild_tree";
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string badFlags = rebuildFlagsProblem(flags);
    if (!badFlags.empty()) return refuse(err, err_cap, std::string(who) + ": " + badFlags);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    PtrMultiFrame& f = *frame;
    const std::string problem = checkTreeCall(f.part[0]->scene.get(), flags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    try {
        std::vector<PtrRebuildInfo> infos(f.parts);
        const std::string refused = runUpdate(who, f, Clock::now(), static_cast<PtrMultiUpdateInfo*>(nullptr), [&](Part& me, uint32_t p, const auto& arrived) {
            arrived();
            rebuildTree(who, *me.scene, flags, me.stream, infos[p]);
        });
        if (!refused.empty()) return refuse(err, err_cap, refused);
        // every partition reached the same tree: the bits of both costs, the decision, the counts
        for (uint32_t p = 1; p < f.parts; ++p) {
            const PtrRebuildInfo &a = infos[0], &b = infos[p];
            const bool same = std::memcmp(&a.costBefore, &b.costBefore, sizeof(double)) == 0 && std::memcmp(&a.costAfter, &b.costAfter, sizeof(double)) == 0 &&
                              a.installed == b.installed && a.nodes == b.nodes && a.levels == b.levels && a.wideNodes == b.wideNodes &&
                              a.wideDepth == b.wideDepth && a.leaves == b.leaves;
            if (same) continue;
            f.broken = true;
            char text[256];
            std::snprintf(text, sizeof(text), ": the partitions disagree: device %d (partition 0) cost %.17g -> %.17g, installed %u, %llu nodes; device %d (partition %u) cost %.17g -> %.17g, installed %u, %llu nodes",
                          f.part[0]->device, a.costBefore, a.costAfter, a.installed, static_cast<unsigned long long>(a.nodes), f.part[p]->device, p, b.costBefore,
                          b.costAfter, b.installed, static_cast<unsigned long long>(b.nodes));
            return refuse(err, err_cap, std::string(who) + text);
        }
        if (info) *info = infos[0];
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
