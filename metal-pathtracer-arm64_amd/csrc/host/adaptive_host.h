// What the three adaptive round loops share on the host - the frame of one device (adaptive.cpp, include/ptr_adaptive.h), the lock-step
// frame on several devices (multi.cpp, include/ptr_multi.h) and the resumable frame (frame_rounds.cpp, which frame.cpp,
// include/ptr_frame.h, calls for its one partition and multi_frame.cpp, include/ptr_multi_frame.h, for each of several in lock step):
// the parameter check, the rules by which a frame is cut into rounds and a round into sub-passes, the sample source of a pass, the
// sample step of a round, the device events of PTR_VERBOSE=launches, and the finish into staging with its downloads.  The owner of the
// per-pixel state is AdaptiveStore (adaptive_state.h, through device_scene.h); the refusals are beside deviceCall in device_scene.h.
// Each loop keeps what is its own: its barriers, its classes, its halo.  Implemented in adaptive.cpp.  Internal: not part of the C-ABI.
#pragma once

#include <algorithm>
#include <functional>
#include <string>

#include "../kernels/adaptive.h"
#include "device_scene.h"
#include "ptr_adaptive.h"

namespace ptrhost {

// "<who>: ..." for bad parameters, empty when all are good.  No device call.
std::string badAdaptiveParams(const char* who, const PtrAdaptiveParams& p);

// samples of the round that starts when the active pixels share the count n (< maxSpp)
inline uint32_t adaptiveRoundSpp(const PtrAdaptiveParams& p, uint32_t n) { return n == 0u ? p.minSpp : std::min(p.stepSpp, p.maxSpp - n); }

// A round whose accumulators do not fit one pass arrives in sub-passes; the update is sample-ordered, so the split changes nothing.
// body(done, spp, last): the sub-pass of samples done .. done + spp - 1 of the round; `last` on the one that completes it.
template <typename Body>
void forEachSubPass(uint64_t maxItems, uint32_t active, uint32_t roundSpp, Body&& body) {
    const uint32_t perPass = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(maxItems / active, roundSpp)));
    for (uint32_t done = 0u; done < roundSpp;) {
        const uint32_t spp = std::min(perPass, roundSpp - done);
        body(done, spp, done + spp == roundSpp);
        done += spp;
    }
}

// samples sampleBase .. sampleBase + spp - 1 of the `active` list entries: hands `consume` the accumulators and joins the stream
using PassSource = std::function<void(uint32_t spp, uint32_t sampleBase, const uint32_t* dList, uint32_t active, PtrRenderStats* one,
                                      const std::function<void(const float4*)>& consume)>;
// the renderer's: traceItems on the scene (`scene` and `settings` outlive the source)
PassSource tracedSource(PtrDeviceScene& scene, const PtrSettings& settings, hipStream_t stream);
// The test-only probes': gathered by k_multi_gather_items from given samples, sample s of image pixel p at dSamples[s * pixels + p],
// s < sampleCount (a sample past them is refused).  `items` grows on demand; a caller that sized it before frees nothing mid-frame.
PassSource gatheredSource(const float4* dSamples, size_t pixels, uint32_t sampleCount, DeviceBuffer<float4>& items, hipStream_t stream);

// What the sample steps of one call share.  `sum` (nullable) collects the passes' stats; the two events, where set, are recorded on
// the stream before and behind every update (the [adaptive] line).
struct SampleStep {
    PassSource source;
    uint64_t maxItems = 0;
    ptrk::AdaptiveState state{};
    hipStream_t stream = nullptr;
    PtrRenderStats* sum = nullptr;
    hipEvent_t beforeUpdate = nullptr, afterUpdate = nullptr;
};
// (done, spp, last) of a sub-pass, as forEachSubPass hands them out
using SubPassHook = std::function<void(uint32_t done, uint32_t spp, bool last)>;
// The `count` (> 0) entries of `list`, all at nBefore samples, get spp more: the sub-pass split, the source, the sample-ordered update
// (e on the last sub-pass) and the pass stats.  inPass runs inside the pass behind the update, before the source joins the stream;
// afterPass once it has joined.
void addSamples(const SampleStep& step, const uint32_t* list, uint32_t count, uint32_t nBefore, uint32_t spp, const SubPassHook& inPass = nullptr,
                const SubPassHook& afterPass = nullptr);

// Up to ten device events (the pairs frame_rounds.h names), created on demand (PTR_VERBOSE=launches) and destroyed with the set.
struct EventSet {
    hipEvent_t e[10] = {};
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() {
        for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev);
    }
    void create(uint32_t count) {
        for (uint32_t i = 0; i < count; ++i) HIP_CHECK(hipEventCreate(&e[i]));
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// An image on its way to the host: `staging` grows to ten words per pixel - rgb 3, cov 6, count 1 - finish(dRgb, dCov, dCount) writes
// them there on the device (dCov / dCount null where outCov / outCount are) and joins its stream, then the blocking downloads.
void finishAndDownload(DeviceBuffer<float>& staging, size_t pixels, float* outRgb, float* outCov, uint32_t* outCount,
                       const std::function<void(float* dRgb, float* dCov, uint32_t* dCount)>& finish);

}  // namespace ptrhost
