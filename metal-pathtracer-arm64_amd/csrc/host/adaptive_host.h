// What the adaptive frame of one device (adaptive.cpp, include/ptr_adaptive.h) and the one on several devices (multi.cpp,
// include/ptr_multi.h) share on the host: the parameter check, the device buffers of the per-pixel state, and the rules by which a frame
// is cut into rounds and a round into sub-passes.  Internal: not part of the C-ABI.
#pragma once

#include <algorithm>
#include <string>

#include "../kernels/adaptive.h"
#include "device_scene.h"
#include "ptr_adaptive.h"

namespace ptrhost {

constexpr uint32_t kAdaptiveBlock = 256u;   // threads per block of the compaction kernels (adaptive.hip)

// "<who>: ..." for bad parameters, empty when all are good.  No device call.
std::string badAdaptiveParams(const char* who, const PtrAdaptiveParams& p);

// The state of a `pixels`-pixel image, the two lists and the compaction's scratch, grown on demand.
struct AdaptiveBuffers {
    ptrk::AdaptiveState state;
    uint32_t* lists[2];
    ptrk::AdaptiveScratch scratch;
};
AdaptiveBuffers ensureAdaptiveBuffers(PtrDeviceScene& ds, size_t pixels);
// the state of every pixel set to zero (asynchronous on `stream`)
void zeroAdaptiveState(const AdaptiveBuffers& b, size_t pixels, hipStream_t stream);

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

}  // namespace ptrhost
