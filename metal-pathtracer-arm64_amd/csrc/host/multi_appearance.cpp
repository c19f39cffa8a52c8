// Host side of include/ptr_multi_appearance.h: the appearance calls of a resident scene on a frame on several devices.  Nothing here
// states a rule or launches a kernel of its own: every call is the check half of the single-device call (dynamic_host.h, appearance.cpp)
// against partition 0's records, the fan-out of what the kernels read, and the run half on every partition's scene and stream - the
// steps multi_update_host.h states for this file and multi_dynamic.cpp.  Compiled with hipcc (host code only), like multi_dynamic.cpp.
#include <algorithm>
#include <cstring>

#include "multi_update_host.h"
#include "ptr_deform_device.h"
#include "ptr_multi_appearance.h"

using namespace ptrhost;
using namespace ptrk;

namespace {

constexpr uint32_t kAllDynamicFlags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS;

// After the join: every partition reached the same light count and the same decision about environment sampling
void requireAgreement(const char* who, PtrMultiFrame& f, const std::vector<PtrAppearanceInfo>& every) {
    for (uint32_t p = 1; p < f.parts; ++p) {
        const PtrAppearanceInfo &a = every[0], &b = every[p];
        if (a.envSampling == b.envSampling && a.lightsAfter == b.lightsAfter) continue;
        f.broken = true;
        char text[256];
        std::snprintf(text, sizeof(text), ": the partitions disagree: device %d (partition 0) envSampling %u, %u lights; device %d (partition %u) envSampling %u, %u lights",
                      f.part[0]->device, a.envSampling, a.lightsAfter, f.part[p]->device, p, b.envSampling, b.lightsAfter);
        throw HipError{std::string(who) + text};
    }
}

// A host-form call (and materials): hostUpdate with every partition's info, compared after the join
template <typename Run>
int hostCall(const char* who, PtrMultiFrame& f, Clock::time_point t0, const std::string& problem, uint64_t stagedBytes, PtrMultiAppearanceInfo* info, char* err,
             size_t cap, Run&& run) {
    std::vector<PtrAppearanceInfo> every;
    if (const int rc = hostUpdate(who, f, t0, problem, info, err, cap, run, &every)) return rc;
    try {
        requireAgreement(who, f, every);
    }
    PTR_CATCH_ALL(err, cap)
    if (info) info->hostStagedBytes = stagedBytes;
    return 0;
}

// A device-form call once step 1 accepted it: the travelling arrays, each of them a row of the one check where they are; refusal(r),
// what a set bit of row r says; run(me, base, info, arrived), the run half on a partition whose copy of the arrays starts at base
// (null: it reads them in place).
template <typename Refusal, typename Run>
int deviceCallOnParts(const char* who, PtrMultiFrame& f, Clock::time_point t0, const Travel& travel, int src_device, void* stream, PtrMultiAppearanceInfo* info,
                      char* err, size_t cap, Refusal&& refusal, Run&& run) {
    try {
        hipStream_t callers = static_cast<hipStream_t>(stream);
        // the check, once, where the arrays are; a refusal leaves every partition as it was
        const DeviceRoute route = routeFromDevice(f, travel, src_device, callers, "pixel", [&](MultiDistribution& md, MultiDistribution::Source& source) {
            const size_t n = travel.arrays.size(), words = (n + 31u) / 32u;
            std::vector<DynCheckRow> rows(n);
            for (size_t r = 0; r < n; ++r) rows[r] = DynCheckRow{travel.arrays[r].src, travel.arrays[r].floats};
            source.rows.ensure(n);
            source.flags.ensure(words);
            const int bad = firstNonFinite(rows.data(), n, reinterpret_cast<DynCheckRow*>(source.rows.ptr), source.flags.ptr,
                                           static_cast<uint32_t*>(md.pinned.pinnedFor(words * sizeof(uint32_t))), callers);
            if (bad >= 0) throw Refused{std::string(who) + ": " + refusal(static_cast<size_t>(bad))};
        });
        std::vector<PtrAppearanceInfo> every(f.parts);
        const std::string refused = runUpdate(who, f, t0, info, [&](Part& me, uint32_t p, const auto& arrived) {
            const float* base = bringArrays(route, travel, me, p);
            run(me, base, &every[p], InputsEnqueued(arrived));
        });
        if (!refused.empty()) return refuse(err, cap, refused);
        requireAgreement(who, f, every);
        if (info) {
            info->first = every[0];
            info->stagedParts = route.stagedParts;
        }
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

// what the device forms refuse about src_device once the frame was found good; a partition's scene lives on another device than the
// arrays may, so the single-device pointer checks are made against src_device
int refuseSource(const char* who, int src_device, char* err, size_t cap) {
    try {
        if (src_device >= ptr_device_count()) return refuse(err, cap, std::string(who) + ": no such HIP device");
    }
    PTR_CATCH_ALL(err, cap)
    return 0;
}

int setTextures(const char* who, PtrMultiFrame* frame, const PtrTextureUpdate* textures, uint32_t count, bool fromDevice, int src_device, void* stream,
                PtrMultiAppearanceInfo* info, char* err, size_t err_cap) {
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(textures, count, "null texture list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (src_device < 0) return refuse(err, err_cap, std::string(who) + ": no such HIP device");
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    if (fromDevice) {
        if (const int rc = refuseSource(who, src_device, err, err_cap)) return rc;
    }
    PtrMultiFrame& f = *frame;
    TexturesUpdate u;
    const float* pinned = nullptr;
    std::string problem;
    try {
        problem = checkTextures(f.part[0]->scene.get(), textures, count, fromDevice, src_device, u);
        if (problem.empty() && !fromDevice) {   // staged once, for every partition
            HIP_CHECK(hipSetDevice(f.rootDevice));
            float* staged = static_cast<float*>(distributionOf(f).pinned.pinnedFor(std::max<size_t>(u.floats, 4u) * sizeof(float)));
            pinned = staged;
            problem = stageTextures(u, staged);
        }
    }
    PTR_CATCH_ALL(err, err_cap)
    if (!fromDevice) {
        return hostCall(who, f, t0, problem, u.floats * sizeof(float), info, err, err_cap,
                        [&](PtrDeviceScene& ds, hipStream_t st, PtrAppearanceInfo* one, const InputsEnqueued& sent) { runTextures(who, ds, u, pinned, false, st, one, sent); });
    }
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    Travel travel;
    for (uint32_t i = 0; i < count; ++i) travel.add(u.entry[i].rgba, u.entry[i].floats, i, 0);
    return deviceCallOnParts(
        who, f, t0, travel, src_device, stream, info, err, err_cap,
        [&](size_t row) { return "texture " + std::to_string(u.entry[travel.arrays[row].entry].texture) + " has a non-finite component"; },
        [&](Part& me, const float* base, PtrAppearanceInfo* one, const InputsEnqueued& sent) {
            TexturesUpdate mine = u;
            if (base) {
                for (const Travel::Array& a : travel.arrays) mine.entry[a.entry].rgba = base + a.at;
            }
            runTextures(who, *me.scene, mine, nullptr, false, me.stream, one, sent);
        });
}

int setEnvironment(const char* who, PtrMultiFrame* frame, const float* rgba, uint32_t width, uint32_t height, bool fromDevice, int src_device, void* stream,
                   PtrMultiAppearanceInfo* info, char* err, size_t err_cap) {
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    if (!rgba) return refuse(err, err_cap, std::string(who) + ": null pixels");
    if (src_device < 0) return refuse(err, err_cap, std::string(who) + ": no such HIP device");
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    if (fromDevice) {
        if (const int rc = refuseSource(who, src_device, err, err_cap)) return rc;
    }
    PtrMultiFrame& f = *frame;
    EnvironmentUpdate u;
    const float* pinned = nullptr;
    std::string problem;
    const size_t floats = static_cast<size_t>(width) * height * 4u;
    try {
        problem = checkEnvironment(f.part[0]->scene.get(), rgba, width, height, fromDevice, src_device, u);
        if (problem.empty() && !fromDevice) {   // staged once, for every partition
            HIP_CHECK(hipSetDevice(f.rootDevice));
            float* staged = static_cast<float*>(distributionOf(f).pinned.pinnedFor(floats * sizeof(float)));
            pinned = staged;
            problem = stageEnvironment(u, staged);
        }
    }
    PTR_CATCH_ALL(err, err_cap)
    if (!fromDevice) {
        return hostCall(who, f, t0, problem, floats * sizeof(float), info, err, err_cap,
                        [&](PtrDeviceScene& ds, hipStream_t st, PtrAppearanceInfo* one, const InputsEnqueued& sent) { runEnvironment(who, ds, u, pinned, false, st, one, sent); });
    }
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    Travel travel;
    travel.add(rgba, floats, 0u, 0);
    return deviceCallOnParts(
        who, f, t0, travel, src_device, stream, info, err, err_cap, [&](size_t) { return std::string("the map has a non-finite component"); },
        [&](Part& me, const float* base, PtrAppearanceInfo* one, const InputsEnqueued& sent) {
            EnvironmentUpdate mine = u;
            if (base) mine.rgba = base;
            runEnvironment(who, *me.scene, mine, nullptr, false, me.stream, one, sent);
        });
}

}  // namespace

extern "C" {

int ptr_multi_frame_set_materials(PtrMultiFrame* frame, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, PtrMultiAppearanceInfo* info,
                                  char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_set_materials";
    const auto t0 = Clock::now();
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = listProblem(indices && materials ? indices : nullptr, count, "null material list");
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    if (const int rc = refuseFrame(who, frame, err, err_cap)) return rc;
    MaterialsUpdate u;
    std::string problem;
    try {
        problem = checkMaterials(frame->part[0]->scene.get(), indices, materials, count, u);
    }
    PTR_CATCH_ALL(err, err_cap)
    return hostCall(who, *frame, t0, problem, 0u, info, err, err_cap, [&](PtrDeviceScene& ds, hipStream_t st, PtrAppearanceInfo* one, const InputsEnqueued& sent) {
        sent();   // (the run half brings the rows itself)
        runMaterials(ds, u, st, one);
    });
}

int ptr_multi_frame_set_textures(PtrMultiFrame* frame, const PtrTextureUpdate* textures, uint32_t count, PtrMultiAppearanceInfo* info, char* err,
                                 size_t err_cap) {
    return setTextures("ptr_multi_frame_set_textures", frame, textures, count, false, 0, nullptr, info, err, err_cap);
}

int ptr_multi_frame_set_textures_device(PtrMultiFrame* frame, const PtrTextureUpdate* textures, uint32_t count, int src_device, void* stream,
                                        PtrMultiAppearanceInfo* info, char* err, size_t err_cap) {
    return setTextures("ptr_multi_frame_set_textures_device", frame, textures, count, true, src_device, stream, info, err, err_cap);
}

int ptr_multi_frame_set_environment(PtrMultiFrame* frame, const float* rgba, uint32_t width, uint32_t height, PtrMultiAppearanceInfo* info, char* err,
                                    size_t err_cap) {
    return setEnvironment("ptr_multi_frame_set_environment", frame, rgba, width, height, false, 0, nullptr, info, err, err_cap);
}

int ptr_multi_frame_set_environment_device(PtrMultiFrame* frame, const float* rgba, uint32_t width, uint32_t height, int src_device, void* stream,
                                           PtrMultiAppearanceInfo* info, char* err, size_t err_cap) {
    return setEnvironment("ptr_multi_frame_set_environment_device", frame, rgba, width, height, true, src_device, stream, info, err, err_cap);
}

int ptr_multi_frame_debug_check_appearance(const PtrSceneDesc* scene, uint32_t dynamic_flags, uint32_t kind, const void* list, const PtrMaterial* materials,
                                           uint32_t count, uint32_t width, uint32_t height, char* err, size_t err_cap) {
    static const char* const names[3] = {"ptr_multi_frame_set_materials", "ptr_multi_frame_set_textures", "ptr_multi_frame_set_environment"};
    const char* who = "ptr_multi_frame_debug_check_appearance";
    if (!scene) return nullArgument(who, err, err_cap);
    if (kind > 2u) return refuse(err, err_cap, std::string(who) + ": no such kind");
    std::string problem = dynamicFlagsProblem(dynamic_flags, kAllDynamicFlags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    who = names[kind];
    try {
        // the records of an upload without the upload: the host preparation, the appearance records, those of a dynamic scene when flags
        // are given, and the few members of the view the checks read
        PreparedScene ps;
        prepareScene(*scene, ps, nullptr, dynamic_flags != 0u, dynamic_flags);
        PtrDeviceScene ds;
        fillAppearanceRecords(*scene, ps, ds.appearanceRecords);
        if (dynamic_flags != 0u) {
            ds.dynamic = std::make_unique<DynamicScene>();
            fillDynamicRecords(*scene, ps.pg, ps.dyn, ps.rectLights, *ds.dynamic);
        }
        SceneView& v = ds.view;
        v.materialCount = scene->materialCount;
        v.rectCount = scene->rectCount;
        v.textureCount = ps.texels.empty() ? 0u : scene->textureCount;
        if (scene->envRgba && scene->envWidth > 0 && scene->envHeight > 0) {
            v.envRgba = reinterpret_cast<const float4*>(scene->envRgba);   // (never read here: "the scene has a map")
            v.envWidth = scene->envWidth, v.envHeight = scene->envHeight;
        }
        if (kind == 0u) {
            MaterialsUpdate u;   // (its list rule comes first, as in the call)
            problem = checkMaterials(&ds, static_cast<const uint32_t*>(list), materials, count, u);
        } else if (kind == 1u) {
            problem = listProblem(list, count, "null texture list");
            if (problem.empty()) {
                TexturesUpdate u;
                problem = checkTextures(&ds, static_cast<const PtrTextureUpdate*>(list), count, false, 0, u);
                std::vector<float> staged(std::max<size_t>(u.floats, 4u));
                if (problem.empty()) problem = stageTextures(u, staged.data());
            }
        } else if (!list) {
            problem = "null pixels";
        } else {
            EnvironmentUpdate u;
            problem = checkEnvironment(&ds, static_cast<const float*>(list), width, height, false, 0, u);
            std::vector<float> staged(problem.empty() ? static_cast<size_t>(width) * height * 4u : 0u);
            if (problem.empty()) problem = stageEnvironment(u, staged.data());
        }
        setErr(err, err_cap, "");
        return problem.empty() ? 0 : refuse(err, err_cap, std::string(who) + ": " + problem);
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
