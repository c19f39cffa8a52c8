// What the update calls of a frame on several devices share: multi_dynamic.cpp (include/ptr_multi_dynamic.h: geometry) and
// multi_appearance.cpp (include/ptr_multi_appearance.h: appearance).  The four steps of a call are stated once here: what a call on an
// existing frame refuses, the run and join of the run halves with their times (runUpdate, hostUpdate), and the way arrays that live on a
// device reach every partition (Travel, routeFromDevice, bringArrays).  Internal: not part of the C-ABI.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dynamic_host.h"
#include "multi_frame_host.h"

namespace ptrhost {

// What a call on an existing frame refuses once its own arguments were found good, before partition 0's records are looked at
inline int refuseFrame(const char* who, const PtrMultiFrame* f, char* err, size_t cap) {
    if (const int rc = refuseBroken(who, f, err, cap)) return rc;
    if (f->sceneless) return refuse(err, cap, std::string(who) + ": the frame has no scene");
    return 0;
}

// The frame's distribution state, made at the first call that needs it
inline MultiDistribution& distributionOf(PtrMultiFrame& f) {
    if (!f.distribution) f.distribution = std::make_unique<MultiDistribution>();
    return *f.distribution;
}

// (a calling thread that visits the partitions' devices and the arrays' device: whatever way the call ends, it leaves on the frame's first)
struct BackOnRoot {
    int device;
    ~BackOnRoot() { (void)hipSetDevice(device); }
};

// Steps 3 and 4 of an update: one(me, p, arrived) on every partition's thread - arrived() once the partition's inputs are on their way -
// with a Refused of a partition kept apart from a failure.  Returns "" or the refusal every partition reached; partitions that do not
// agree on it break the frame.  info (nullable; PtrMultiUpdateInfo or PtrMultiAppearanceInfo) is filled but for `first` and what the
// distribution counts (stagedParts, hostStagedBytes).
template <typename Info, typename One>
std::string runUpdate(const char* who, PtrMultiFrame& f, Clock::time_point t0, Info* info, One&& one) {
    std::vector<std::string> refusals(f.parts);
    std::vector<double> arrivedAt(f.parts, 0.0);
    const PtrMultiInfo kept = f.last;   // (the driver notes the partitions' times there: an update leaves the frame's own figures alone)
    runParts(f, [&](Part& me, uint32_t p, const auto&) {
        auto arrived = [&] { arrivedAt[p] = since(t0); };
        try {
            one(me, p, arrived);
        } catch (const Refused& r) {
            refusals[p] = r.message;
        }
    });
    const PtrMultiInfo timed = f.last;
    f.last = kept;
    for (uint32_t p = 1; p < f.parts; ++p) {
        if (refusals[p] == refusals[0]) continue;
        f.broken = true;
        auto said = [&](uint32_t q) { return refusals[q].empty() ? std::string("accepted the call") : "refused it (" + refusals[q] + ")"; };
        throw HipError{std::string(who) + ": the partitions disagree: device " + std::to_string(f.part[0]->device) + " (partition 0) " + said(0u) + ", device " +
                       std::to_string(f.part[p]->device) + " (partition " + std::to_string(p) + ") " + said(p)};
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->parts = f.parts;
        for (uint32_t p = 0; p < f.parts; ++p) {
            info->partSeconds[p] = timed.partRenderSeconds[p];
            info->distributeSeconds = std::max(info->distributeSeconds, arrivedAt[p]);
        }
        info->totalSeconds = since(t0);
    }
    return refusals[0];
}

// An update call whose inputs every partition copies from the host itself (or from the frame's pinned memory): t0 is the call's entry,
// `problem` what the check half (and the staging) said, run(scene, stream, info, enqueued) the run half, which calls `enqueued` once the
// partition's copies are on its stream.  every (nullable): the run half's info of every partition, for a call that compares them; without
// it only partition 0 is asked for one.
template <typename Info, typename Run>
int hostUpdate(const char* who, PtrMultiFrame& f, Clock::time_point t0, const std::string& problem, Info* info, char* err, size_t cap, Run&& run,
               std::vector<decltype(Info::first)>* every = nullptr) {
    if (!problem.empty()) return refuse(err, cap, std::string(who) + ": " + problem);
    try {
        decltype(Info::first) first{};
        if (every) every->assign(f.parts, first);
        const std::string refused = runUpdate(who, f, t0, info, [&](Part& me, uint32_t p, const auto& arrived) {
            run(*me.scene, me.stream, every ? &(*every)[p] : p == 0u ? &first : nullptr, InputsEnqueued(arrived));
        });
        if (!refused.empty()) return refuse(err, cap, refused);
        if (info) info->first = every ? (*every)[0] : first;
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

// Where the arrays of a device-form call that travel lie in a partition's buffer (and in the pinned memory), in floats.  entry / which
// are the caller's: which entry of its list an array belongs to and which of that entry's arrays it is.
struct Travel {
    struct Array {
        const float* src;
        size_t at, floats;
        uint32_t entry;
        int which;
    };
    std::vector<Array> arrays;
    size_t floats = 0;
    void add(const float* src, size_t n, uint32_t entry, int which) {
        arrays.push_back(Array{src, floats, n, entry, which});
        floats += n;
    }
};

// How the arrays of a device-form call reach every partition (include/ptr_multi_dynamic.h, Distribution)
struct DeviceRoute {
    int srcDevice = 0;
    std::vector<int> how;           // per partition: 0 in place, 1 pulled from its peer, 2 through the pinned memory
    uint32_t stagedParts = 0;
    const float* pinned = nullptr;  // the travelling arrays in the frame's pinned memory, when a partition needs them there
    hipEvent_t ready = nullptr;     // recorded on the caller's stream behind the check and the staging copies
};

// Step 2 of a device-form call, on the calling thread: who pulls and who cannot, then on src_device and the caller's stream the check -
// check(distribution, source), once, where the arrays are; it joins the stream and throws Refused, every partition as it was - the
// staging copies for the partitions that cannot pull, once for all of them, and the event.  arraysName: "vertex" or "pixel", for the
// line that goes to stderr per staged partition.  Leaves the frame's first device current.
template <typename Check>
DeviceRoute routeFromDevice(PtrMultiFrame& f, const Travel& travel, int src_device, hipStream_t callers, const char* arraysName, Check&& check) {
    BackOnRoot backOnRoot{f.rootDevice};
    MultiDistribution& md = distributionOf(f);
    DeviceRoute route;
    route.srcDevice = src_device;
    route.how.assign(f.parts, 0);
    for (uint32_t p = 0; p < f.parts; ++p) {
        const Part& me = *f.part[p];
        if (me.device == src_device && !me.forceStaged) continue;
        int direct = 0;
        if (me.device != src_device && !me.forceStaged) {
            HIP_CHECK(hipSetDevice(me.device));
            HIP_CHECK(hipDeviceCanAccessPeer(&direct, me.device, src_device));
            if (direct) {
                const hipError_t enabled = hipDeviceEnablePeerAccess(src_device, 0);
                if (enabled != hipSuccess && enabled != hipErrorPeerAccessAlreadyEnabled) direct = 0;
                (void)hipGetLastError();
            }
        }
        route.how[p] = direct ? 1 : 2;
        if (!direct) {
            ++route.stagedParts;
            std::fprintf(stderr, "[ptr] device %d does not read the %s arrays of device %d directly: they go through pinned host memory\n", me.device, arraysName,
                         src_device);
        }
    }
    HIP_CHECK(hipSetDevice(src_device));
    auto& source = md.source[src_device];
    if (!source) {
        source = std::make_unique<MultiDistribution::Source>();
        HIP_CHECK(hipEventCreateWithFlags(&source->ready, hipEventDisableTiming));
    }
    check(md, *source);
    if (route.stagedParts > 0u && travel.floats > 0u) {   // once, for every partition that cannot pull; the event below is behind these copies
        float* staged = static_cast<float*>(md.pinned.pinnedFor(travel.floats * sizeof(float)));
        for (const Travel::Array& a : travel.arrays) {
            HIP_CHECK(hipMemcpyAsync(staged + a.at, a.src, a.floats * sizeof(float), hipMemcpyDeviceToHost, callers));
        }
        route.pinned = staged;
    }
    HIP_CHECK(hipEventRecord(source->ready, callers));
    route.ready = source->ready;
    return route;
}

// On partition p's thread: its stream waits for the source, and the arrays it does not read in place are brought into me.pulled on
// that stream.  The base of its copy (array a at base + a.at), or null: it reads the caller's arrays where they are.
inline const float* bringArrays(const DeviceRoute& route, const Travel& travel, Part& me, uint32_t p) {
    HIP_CHECK(hipStreamWaitEvent(me.stream, route.ready, 0));
    if (route.how[p] == 0 || travel.floats == 0u) return nullptr;
    me.pulled.ensure(travel.floats);
    for (const Travel::Array& a : travel.arrays) {
        if (route.how[p] == 1) {
            HIP_CHECK(hipMemcpyPeerAsync(me.pulled.ptr + a.at, me.device, a.src, route.srcDevice, a.floats * sizeof(float), me.stream));
        } else {
            HIP_CHECK(hipMemcpyAsync(me.pulled.ptr + a.at, route.pinned + a.at, a.floats * sizeof(float), hipMemcpyHostToDevice, me.stream));
        }
    }
    return me.pulled.ptr;
}

}  // namespace ptrhost
