// What the two host files of a frame on several devices share: multi_frame.cpp (include/ptr_multi_frame.h), which owns the frame, and
// multi_dynamic.cpp (include/ptr_multi_dynamic.h), which updates its scenes in place.  The frame object, what a partition keeps, the
// driver that runs a call's partitions on threads, and the one create behind every entry point.  Internal: not part of the C-ABI.
#pragma once

#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "adaptive_state.h"
#include "device_scene.h"
#include "multi_host.h"
#include "parallel.h"
#include "ptr_multi_frame.h"
#include "round_barrier.h"

namespace ptrhost {

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// what one partition keeps for the frame's life; everything of it lives on `device`
struct Part {
    int device = 0;
    bool forceStaged = false;
    ptrk::MultiPart mp{};
    uint32_t local = 0;                      // its pixels
    std::unique_ptr<PtrDeviceScene> scene;   // null: the test-only frame
    hipStream_t stream = nullptr;
    AdaptiveStore store;   // the state, image order; L_p's two buffers; the compaction's scratch and the class-minimum word
    DeviceBuffer<uint32_t> order, listS;   // the first list; S_p
    DeviceBuffer<uint8_t> inS;
    DeviceBuffer<float> edge, bandOut, packed;   // the exchange's edge rows; the outputs in band layout; the checkpoint buffer
    DeviceBuffer<float4> probeSamples, probeItems;
    std::vector<float> hostPacked;   // the checkpoint buffer's host side
    // include/ptr_multi_dynamic.h: the vertex arrays of another device, pulled here (allocated by the first such call, kept)
    DeviceBuffer<float> pulled;
};

// What a frame created over dynamic scenes keeps beside its partitions (include/ptr_multi_dynamic.h); a static frame has none of it.
struct MultiDynamic {
    uint32_t flags = 0;   // PTR_DYNAMIC_*: what every partition's scene was uploaded with
    // portable pinned memory, grown on demand and kept: host vertex data is staged here once for all partitions, and device-resident
    // data passes through here once for the partitions that cannot pull it from a peer
    void* pinned = nullptr;
    size_t pinnedBytes = 0;
    void* pinnedFor(size_t bytes) {
        if (bytes > pinnedBytes) {
            if (pinned) (void)hipHostFree(pinned);
            pinned = nullptr, pinnedBytes = 0;
            HIP_CHECK(hipHostMalloc(&pinned, bytes, hipHostMallocPortable));
            pinnedBytes = bytes;
        }
        return pinned;
    }
    // per device the caller's arrays have lived on: the scratch of the finiteness check there, and the event the partitions wait on
    struct Source {
        DeviceBuffer<float4> rows;
        DeviceBuffer<uint32_t> flags;
        hipEvent_t ready = nullptr;
    };
    std::map<int, std::unique_ptr<Source>> source;
    ~MultiDynamic() {
        for (auto& s : source) {
            if (s.second->ready && hipSetDevice(s.first) == hipSuccess) (void)hipEventDestroy(s.second->ready);
        }
        if (pinned) (void)hipHostFree(pinned);
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
    // the first device: the partitions' band buffers one after the other, where each output of each partition starts
    // (k_multi_interleave's table: [output][partition]), the image-order outputs of a host resolve, the feature buffers
    int rootDevice = 0;
    std::vector<uint64_t> wordOffset;
    DeviceBuffer<float> gathered, image;
    DeviceBuffer<uint64_t> dWordOffset;
    DeviceBuffer<float4> albedo, normal;
    // pixels per count, kept on the host as PtrFrame keeps them: the checks and ptr_multi_frame_info need no device call
    std::map<uint32_t, uint64_t> classes;
    bool broken = false;   // a call failed on a device: only release is left
    PtrMultiInfo last{};
    std::unique_ptr<ptrhost::MultiDynamic> dynamic;   // ptr_multi_frame_create_dynamic only

    bool uniform() const { return classes.size() == 1u; }
    uint32_t minCount() const { return classes.begin()->first; }
    uint32_t maxCount() const { return classes.rbegin()->first; }
    bool empty() const { return uniform() && minCount() == 0u; }
};

namespace ptrhost {

// One call's partitions on threads: body(me, p, meet) with me's device current.  meet() is the round barrier - false once a partition
// has failed, and the body then returns at once.  Every way out of a worker but the regular one releases the partitions that wait for
// it; every worker joins its own stream.  A failure is reported with the device's id and leaves the frame broken.
template <typename Body>
void runParts(PtrMultiFrame& f, Body&& body) {
    const uint32_t parts = f.parts;
    std::vector<std::string> errors(parts);
    std::vector<double> seconds(parts, 0.0), waited(parts, 0.0);
    ptr::RoundBarrier barrier(parts);
    auto worker = [&](uint32_t p) {
        Part& me = *f.part[p];
        const auto t0 = Clock::now();
        auto meet = [&]() -> bool {
            const auto m0 = Clock::now();
            const bool all = barrier.arriveAndWait();
            waited[p] += since(m0);
            return all;
        };
        try {
            HIP_CHECK(hipSetDevice(me.device));
            body(me, p, meet);
            HIP_CHECK(hipGetLastError());
        } catch (const HipError& e) {
            barrier.fail();
            errors[p] = e.message;
        } catch (const std::exception& e) {
            barrier.fail();
            errors[p] = std::string("exception: ") + e.what();
        } catch (...) {
            barrier.fail();
            errors[p] = "unknown exception";
        }
        if (me.stream) (void)hipStreamSynchronize(me.stream);
        seconds[p] = since(t0);
    };
    try {
        ptr::runOnThreads(parts, worker, [&] { barrier.fail(); });   // (a thread that could not be started never arrives)
    } catch (...) {
        f.broken = true;
        (void)hipSetDevice(f.rootDevice);
        throw;
    }
    (void)hipSetDevice(f.rootDevice);
    for (uint32_t p = 0; p < parts; ++p) {
        if (errors[p].empty()) continue;
        f.broken = true;
        throw HipError{"device " + std::to_string(f.part[p]->device) + ": " + errors[p]};
    }
    if (barrier.failed()) {
        f.broken = true;
        throw HipError{"a partition left the frame early"};
    }
    for (uint32_t p = 0; p < parts; ++p) {
        f.last.partRenderSeconds[p] = seconds[p];
        f.last.partWaitSeconds[p] = waited[p];
    }
}

// Create, for every entry point (multi_frame.cpp): a scene (or, for the test-only frame, samples), the size, the devices asked for.
// dynamic: the scene is prepared and uploaded as ptr_scene_upload_deformable would with dynamicFlags, and the frame keeps a MultiDynamic.
int createMultiFrame(const char* who, const PtrSceneDesc* scene, const PtrSettings* settings, const float* samples, uint32_t sampleCount, bool sceneless,
                     const int* ids, int n, bool listed, bool dynamic, uint32_t dynamicFlags, PtrMultiFrame** out, char* err, size_t cap);
// what every call on an existing frame refuses first
int refuseBroken(const char* who, const PtrMultiFrame* f, char* err, size_t cap);

}  // namespace ptrhost
