// The update calls of a resident scene - its geometry (dynamic.cpp, rebuild.cpp: include/ptr_dynamic.h, ptr_deform.h, ptr_deform_device.h,
// ptr_rebuild.h) and its appearance (appearance.cpp: include/ptr_appearance.h) - and what they share with the frame on several devices
// that fans them out (multi_dynamic.cpp: include/ptr_multi_dynamic.h; multi_appearance.cpp: include/ptr_multi_appearance.h).  Every
// call is two halves: check*, the rules of the call on the host against the scene's host-side records - no device work, no record changed, "" or the refusal without the caller's name
// in front - which leaves the accepted update in an ...Update struct, and run*, the device work of that update on one scene and one
// stream, joined before it returns and before the records follow.  The records come from the preparation at upload (fillDynamicRecords,
// fillAppearanceRecords), never from the device.  Scenes uploaded from one preparation with the same flags and given the same calls hold
// the same records, so an update checked against one of them runs on all of them.  Internal: not part of the C-ABI.
#pragma once

#include <chrono>
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "device_scene.h"
#include "index_rule.h"
#include "ptr_appearance.h"
#include "ptr_deform_device.h"
#include "ptr_rebuild.h"

namespace ptrhost {

// A call refused after device work began, the scene as it was (a non-finite component found on the device, the depth bounds of a
// rebuild): reported like any failure by the single-device calls, told apart from a device failure by multi_dynamic.cpp.
struct Refused : HipError {
    explicit Refused(std::string m) : HipError{std::move(m)} {}
};

// The host-side records of a dynamic scene, the ones the check halves read, from a description and its preparation: what
// uploadDynamicTables keeps beside the device arrays.  No device call.
void fillDynamicRecords(const PtrSceneDesc& desc, const ptr::PreparedGeometry& pg, const ptr::DynamicTables& t, const ptr::RectLightTable& lights,
                        DynamicScene& dyn);

// The host-side records of a scene's appearance from the description and its preparation (appearance.cpp): the compact material rows,
// every rectangle's material index, the texture records.  No device call.
void fillAppearanceRecords(const PtrSceneDesc& desc, const PreparedScene& ps, AppearanceRecords& rec);

// What every update entry point is: a null scene refused, the call's rules (check), the device work (run)
template <typename Check, typename Run>
int updateCall(const char* who, PtrDeviceScene* scene, char* err, size_t err_cap, Check&& check, Run&& run) {
    if (!scene) return nullArgument(who, err, err_cap);
    try {
        const std::string problem = check();
        if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    }
    PTR_CATCH_ALL(err, err_cap)
    return deviceCall(who, scene, true, err, err_cap, run);
}

// The host staging copy: `n` floats into `dst` (pinned memory, usually); false when one of them is not finite
inline bool stageFinite(const float* src, size_t n, float* dst) {
    bool finite = true;
    for (size_t k = 0; k < n; ++k) {
        finite = finite && std::isfinite(src[k]);
        dst[k] = src[k];
    }
    return finite;
}

// The device finiteness check: k_dyn_check_finite over `n` > 0 arrays of the current device (row r: its pointer and its floats).  The rows
// and zeroed flag words go to the device, the kernel runs, the words come back and `st` is joined: the first row with a non-finite float,
// or -1.  The scratch is the caller's: dRows (n rows) and dFlags ((n + 31) / 32 words) on the device, pinnedFlags (as many) for the way back.
int firstNonFinite(const ptrk::DynCheckRow* rows, size_t n, ptrk::DynCheckRow* dRows, uint32_t* dFlags, uint32_t* pinnedFlags, hipStream_t st);

// What a run half calls (when given) once the copies that bring the scene the call's inputs are enqueued on its stream
using InputsEnqueued = std::function<void()>;

// "" or what is wrong with a call's list before anyone looks into it
std::string listProblem(const void* list, uint32_t count, const char* nullWords);
// "" or what is wrong with `bytes` of a caller's array at `p` for a kernel on `device` to read (the pointer alone is looked at)
std::string devicePointerProblem(const void* p, size_t bytes, int device);
// "" or what the uploads of a dynamic scene refuse about `flags`; `known` is the mask of the PTR_DYNAMIC_* flags the entry point knows
std::string dynamicFlagsProblem(uint32_t flags, uint32_t known);

// ---- ptr_scene_set_mesh_transforms
struct TransformUpdate {
    std::vector<uint32_t> mesh;
    std::vector<ptrk::DynMeshRow> rows;
};
std::string checkMeshTransforms(const PtrDeviceScene* scene, const PtrMeshTransform* transforms, uint32_t count, TransformUpdate& out);
void runMeshTransforms(PtrDeviceScene& ds, const TransformUpdate& u, hipStream_t st, PtrUpdateInfo* info, const InputsEnqueued& enqueued = {});

// ---- ptr_scene_set_mesh_vertices: the layout of the staging buffer, the staging (each component looked at on the way), the device half
struct VerticesUpdate {
    struct Entry {
        uint32_t mesh = 0;
        size_t positions = 0, normals = 0, tangents = 0;   // where the arrays go in the staging buffer, in floats
        bool used = false, hasTangents = false;            // used false: a mesh without triangles stages nothing
    };
    std::vector<Entry> entry;
    std::vector<ptrk::DynMeshRow> rows;
    size_t floats = 0;
};
std::string checkMeshVertices(const PtrDeviceScene* scene, const PtrMeshVertices* meshes, uint32_t count, VerticesUpdate& out);
std::string stageMeshVertices(const PtrMeshVertices* meshes, const VerticesUpdate& u, float* pinned);
// pinned: u.floats staged floats in pinned host memory this device's copies may read
void runMeshVertices(PtrDeviceScene& ds, const VerticesUpdate& u, const float* pinned, hipStream_t st, PtrUpdateInfo* info,
                     const InputsEnqueued& enqueued = {});

// ---- ptr_scene_set_mesh_vertices_device
struct DeviceVerticesUpdate {
    struct Entry {
        uint32_t mesh = 0, vertexCount = 0;
        bool used = false, computes = false;                      // computes: null normals, k_dyn_vertex_normals fills them
        ptrk::DynVertexArrays v{nullptr, nullptr, nullptr};       // where the gather reads its arrays, on the device
        size_t computedAt = 0;                                    // computes: where in the scene's scratch, in floats
    };
    // the arrays k_dyn_check_finite looks at, in the order a refusal names them: per named mesh positions, normals, tangents
    struct Checked {
        uint32_t entry;      // of the list
        const char* what;
        bool computed;       // normals the call computes: the row's pointer is set once the scratch is there
        const float* data;   // given: the caller's array
        uint64_t floats;
    };
    std::vector<Entry> entry;
    std::vector<Checked> checked;
    std::vector<ptrk::DynMeshRow> rows;
    size_t computedFloats = 0;
};
// arraysDevice: the device the caller's arrays must live on
std::string checkMeshVerticesDevice(const PtrDeviceScene* scene, const PtrMeshVerticesDevice* meshes, uint32_t count, int arraysDevice,
                                    DeviceVerticesUpdate& out);
// k_dyn_check_finite over the given arrays of `u` alone, on the current device (the one they live on) and `st`, which is joined: throws
// Refused "<who>: mesh M has a non-finite ... component".  dRows / dFlags: scratch on that device; pinnedFlags: its pinned twin.
void checkGivenArrays(const char* who, const DeviceVerticesUpdate& u, DeviceBuffer<float4>& dRows, DeviceBuffer<uint32_t>& dFlags, uint32_t* pinnedFlags,
                      hipStream_t st);
// The arrays of u.entry are on ds.device.  checkGiven false: the given arrays were looked at already and only computed normals are.
void runMeshVerticesDevice(const char* who, PtrDeviceScene& ds, const DeviceVerticesUpdate& u, bool checkGiven, hipStream_t st, PtrUpdateInfo* info);

// ---- ptr_scene_set_spheres (kind 0) and ptr_scene_set_rects (kind 1)
// The staging buffer of the two calls: 16 B rows and where each goes, (PTR_SCATTER_* << 28) | row
struct ScatterRows {
    std::vector<float> rows;
    std::vector<uint32_t> dest;
};
struct PrimitivesUpdate {
    uint32_t kind = 0, count = 0;
    ScatterRows rows;
    PrimitiveRecords next;   // the records once the call is accepted
};
std::string checkPrimitives(uint32_t kind, const PtrDeviceScene* scene, const void* list, uint32_t count, PrimitivesUpdate& out);
void runPrimitives(PtrDeviceScene& ds, const PrimitivesUpdate& u, hipStream_t st, PtrUpdateInfo* info, const InputsEnqueued& enqueued = {});

// ---- ptr_scene_tree_cost and ptr_scene_rebuild_tree (rebuild.cpp)
std::string rebuildFlagsProblem(uint32_t flags);
std::string checkTreeCall(const PtrDeviceScene* scene, uint32_t flags);
double treeCost(PtrDeviceScene& ds, hipStream_t st);
// a depth refusal of step 8 is thrown as Refused "<who>: ...", the scene unchanged
void rebuildTree(const char* who, PtrDeviceScene& ds, uint32_t flags, hipStream_t st, PtrRebuildInfo& info);

// ---- ptr_scene_set_materials (appearance.cpp, like everything below)
using UpdateClock = std::chrono::steady_clock;
struct MaterialsUpdate {
    UpdateClock::time_point began;       // the call's entry: the info's clock includes the check
    std::vector<uint32_t> index;         // the named materials
    std::vector<float> rows, texRows;    // their compact rows; their texture rows (a scene with textures)
    uint32_t typeMask = 0;               // of the table with the rows in it, like everything below
    bool randomWalk = false;
    bool touchesRects = false;           // a rectangle uses a named material: `lights` is the scene's new table
    ptr::RectLightTable lights;
    bool keyChanged = false;             // a named material changed its shade key: `keys` is k_app_rekey's table
    std::vector<uint8_t> keys;
};
std::string checkMaterials(const PtrDeviceScene* scene, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, MaterialsUpdate& out);
void runMaterials(PtrDeviceScene& ds, const MaterialsUpdate& u, hipStream_t st, PtrAppearanceInfo* info);

// ---- ptr_scene_set_textures and its device form: the rules and the new records, the staging of host pixels (each component looked at
// on the way), the device half
struct TexturesUpdate {
    UpdateClock::time_point began;
    bool fromDevice = false;
    struct Entry {
        uint32_t texture = 0;
        const float* rgba = nullptr;     // the caller's level 0: host pixels to stage, or a device array read where it is
        size_t floats = 0;
    };
    std::vector<Entry> entry;
    std::vector<uint32_t> records;       // per entry the texture's record (kernels/texture.h) with the call's wrap / filter word
    size_t floats = 0;                   // of the host form: what stageTextures writes, entry after entry
};
// arraysDevice: the device the arrays of the device form must live on
std::string checkTextures(const PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, int arraysDevice,
                          TexturesUpdate& out);
std::string stageTextures(const TexturesUpdate& u, float* pinned);
// pinned: u.floats staged floats of the host form, in pinned memory this device's copies may read.  A non-finite component of the device
// form: Refused "<who>: texture T has ..."; checkGiven false: the arrays were looked at already (where they live) and are not again.
void runTextures(const char* who, PtrDeviceScene& ds, const TexturesUpdate& u, const float* pinned, bool checkGiven, hipStream_t st, PtrAppearanceInfo* info,
                 const InputsEnqueued& enqueued = {});

// ---- ptr_scene_set_environment and its device form
struct EnvironmentUpdate {
    UpdateClock::time_point began;
    bool fromDevice = false;
    const float* rgba = nullptr;
    uint32_t width = 0, height = 0;
    std::vector<float> cell;             // the per-row cell weights of a map of that size
};
std::string checkEnvironment(const PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, bool fromDevice, int arraysDevice,
                             EnvironmentUpdate& out);
// the host form's pixels into `pinned` (width * height * 4 floats), each component looked at on the way: "" or the refusal
std::string stageEnvironment(const EnvironmentUpdate& u, float* pinned);
// pinned: the staged pixels of the host form (null for the device form).  A non-finite component of the device form: Refused "<who>: the
// map has a non-finite component", the scene untouched; checkGiven as for runTextures.
void runEnvironment(const char* who, PtrDeviceScene& ds, const EnvironmentUpdate& u, const float* pinned, bool checkGiven, hipStream_t st,
                    PtrAppearanceInfo* info, const InputsEnqueued& enqueued = {});

}  // namespace ptrhost
