// What the host files of a frame on several devices share: multi_frame.cpp (include/ptr_multi_frame.h), which owns the frame, and
// multi_dynamic.cpp / multi_appearance.cpp (include/ptr_multi_dynamic.h, include/ptr_multi_appearance.h), which update its scenes in
// place (what those two share beyond this is in multi_update_host.h).  The frame object, what a partition keeps beside
// its FramePart (frame_rounds.h), runParts - the partition driver of multi_host.h on a frame - and the one create behind every entry
// point.  Internal: not part of the C-ABI.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "device_scene.h"
#include "frame_classes.h"
#include "frame_rounds.h"
#include "multi_host.h"
#include "ptr_multi_frame.h"

namespace ptrhost {

// what one partition keeps for the frame's life; everything of it lives on `device`
struct Part {
    int device = 0;
    bool forceStaged = false;
    FramePart fp;   // its pixels, the state, the lists, the test-only frame's samples; fp.scene is `scene` below, or null
    std::unique_ptr<PtrDeviceScene> scene;   // null: the test-only frame
    hipStream_t stream = nullptr;
    DeviceBuffer<float> edge, bandOut, packed;   // the exchange's edge rows; the outputs in band layout; the checkpoint buffer
    std::vector<float> hostPacked;   // the checkpoint buffer's host side
    // include/ptr_multi_dynamic.h, include/ptr_multi_appearance.h: the vertex or pixel arrays of another device, pulled here (allocated by
    // the first such call, kept)
    DeviceBuffer<float> pulled;
};

// What a frame created over dynamic scenes keeps beside its partitions (include/ptr_multi_dynamic.h); a static frame has none of it.
struct MultiDynamic {
    uint32_t flags = 0;   // PTR_DYNAMIC_*: what every partition's scene was uploaded with
};

// What the update calls of a frame distribute their inputs through (include/ptr_multi_dynamic.h, include/ptr_multi_appearance.h), made by
// the first call that needs it (distributionOf, multi_update_host.h): a frame that is never updated, static or dynamic, has none of it.
struct MultiDistribution {
    // portable pinned memory, grown on demand and kept: host vertex data and host pixels are staged here once for all partitions, and
    // device-resident data passes through here once for the partitions that cannot pull it from a peer
    PinnedBuffer pinned{hipHostMallocPortable};
    // per device the caller's arrays have lived on: the scratch of the finiteness check there, and the event the partitions wait on
    struct Source {
        DeviceBuffer<float4> rows;
        DeviceBuffer<uint32_t> flags;
        hipEvent_t ready = nullptr;
    };
    std::map<int, std::unique_ptr<Source>> source;
    ~MultiDistribution() {
        for (auto& s : source) {
            if (s.second->ready && hipSetDevice(s.first) == hipSuccess) (void)hipEventDestroy(s.second->ready);
        }
    }
};

}  // namespace ptrhost

struct PtrMultiFrame {
    PtrSettings settings{};
    uint32_t width = 0, height = 0, parts = 0, sampleCount = 0;
    size_t pixels = 0;
    bool sceneless = false;
    std::vector<std::unique_ptr<ptrhost::Part>> part;
    ptrhost::HaloExchange ex;
    // the first device: the gather of the partitions' band buffers, the image-order outputs of a host resolve, the feature buffers
    int rootDevice = 0;
    ptrhost::BandGather bands;
    DeviceBuffer<float> image;
    DeviceBuffer<float4> albedo, normal;
    // pixels per count, kept on the host as PtrFrame keeps them: the checks and ptr_multi_frame_info need no device call
    ptrhost::CountClasses classes;
    bool broken = false;   // a call failed on a device: only release is left
    PtrMultiInfo last{};
    std::unique_ptr<ptrhost::MultiDynamic> dynamic;   // ptr_multi_frame_create_dynamic only
    std::unique_ptr<ptrhost::MultiDistribution> distribution;   // null until an update call distributes something
};

namespace ptrhost {

// One call's partitions on threads (runPartitionThreads): body(me, p, meet) with me's device current; every worker joins its own
// stream.  The call's seconds per partition are the frame's last; a failure leaves the frame broken.
template <typename Body>
void runParts(PtrMultiFrame& f, Body&& body) {
    std::vector<int> devices;
    for (const auto& me : f.part) devices.push_back(me->device);
    try {
        runPartitionThreads(
            devices, f.last.partRenderSeconds, f.last.partWaitSeconds, [&](uint32_t p, const auto& meet) { body(*f.part[p], p, meet); },
            [&](uint32_t p) { return f.part[p]->stream; }, [](uint32_t) {});
    } catch (...) {
        f.broken = true;
        (void)hipSetDevice(f.rootDevice);
        throw;
    }
    (void)hipSetDevice(f.rootDevice);
}

// Create, for every entry point (multi_frame.cpp): a scene (or, for the test-only frame, samples), the size, the devices asked for.
// dynamic: the scene is prepared and uploaded as ptr_scene_upload_deformable would with dynamicFlags, and the frame keeps a MultiDynamic.
int createMultiFrame(const char* who, const PtrSceneDesc* scene, const PtrSettings* settings, const float* samples, uint32_t sampleCount, bool sceneless,
                     const int* ids, int n, bool listed, bool dynamic, uint32_t dynamicFlags, PtrMultiFrame** out, char* err, size_t cap);
// what every call on an existing frame refuses first
int refuseBroken(const char* who, const PtrMultiFrame* f, char* err, size_t cap);

}  // namespace ptrhost
