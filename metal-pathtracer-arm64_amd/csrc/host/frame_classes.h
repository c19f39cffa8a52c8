// The pixels of a resumable frame per sample count n_p, kept on the host by PtrFrame (frame.cpp) and PtrMultiFrame (multi_frame.cpp): a
// round moves |S| pixels from n_min to n_min + k, so the checks and the info calls need no device call.  Beside the table, what the
// accumulate, refine and reset entry points of both frames refuse once the frame may be looked at.  No HIP include: a CPU program drives
// the table (tools/frame_host_check.cpp).  Internal: not part of the C-ABI.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>

#include "ptr_frame.h"

namespace ptrhost {

class CountClasses {
public:
    void reset(uint64_t pixels) { at_ = {{0u, pixels}}; }   // every pixel at 0 samples
    // from the counts of a state that was imported
    void rebuild(const uint32_t* n, size_t pixels) {
        at_.clear();
        for (size_t p = 0; p < pixels; ++p) ++at_[n[p]];
    }
    void move(uint32_t from, uint32_t to, uint64_t pixels) {
        if (pixels == 0u) return;
        auto it = at_.find(from);
        if (it != at_.end()) {   // (always, unless an import brought counts that disagree with themselves)
            it->second -= std::min<uint64_t>(it->second, pixels);
            if (it->second == 0u) at_.erase(it);
        }
        at_[to] += pixels;
    }

    bool uniform() const { return at_.size() == 1u; }
    uint32_t minCount() const { return at_.begin()->first; }
    uint32_t maxCount() const { return at_.rbegin()->first; }
    bool empty() const { return uniform() && minCount() == 0u; }
    uint64_t pixelsAt(uint32_t count) const { return at_.count(count) ? at_.at(count) : 0u; }
    // everything of ptr_frame_info but the size, into a struct of zeros
    void fill(PtrFrameInfo& out) const {
        out.minCount = minCount();
        out.maxCount = maxCount();
        for (const auto& c : at_) out.totalSamples += static_cast<uint64_t>(c.first) * c.second;
        out.uniform = uniform() ? 1u : 0u;
    }

private:
    std::map<uint32_t, uint64_t> at_;
};

// "<who>: ..." or empty.  sampleLimit: the samples a test-only frame was given; 0 for a frame with a scene, which has no limit.
inline std::string pastGivenSamples(const std::string& w, uint64_t lastSample, uint32_t sampleLimit) {
    return sampleLimit && lastSample > sampleLimit ? w + ": a sample past the ones the frame was given" : std::string();
}

inline std::string badAccumulate(const char* who, const CountClasses& classes, uint32_t spp, uint32_t sampleLimit) {
    const std::string w(who);
    if (!classes.uniform()) {
        return w + ": the frame is not uniform (its pixels hold different sample counts); a refine with threshold 0 "
                   "brings every pixel with a non-zero error up to a common count";
    }
    const uint64_t after = static_cast<uint64_t>(classes.minCount()) + spp;
    if (after > 0xFFFFFFF0ull) return w + ": too many samples";
    return pastGivenSamples(w, after, sampleLimit);
}

inline std::string badRefine(const char* who, const CountClasses& classes, const PtrAdaptiveParams& params, uint32_t sampleLimit) {
    const std::string w(who);
    if (!classes.empty() && classes.minCount() < 2u) return w + ": every pixel of a frame that is not empty must hold at least 2 samples";
    return pastGivenSamples(w, params.maxSpp, sampleLimit);
}

// settings: null keeps the stored ones
inline std::string badReset(const char* who, uint32_t width, uint32_t height, const PtrSettings* settings) {
    const bool same = !settings || (settings->width == width && settings->height == height);
    return same ? std::string() : std::string(who) + ": a frame keeps its width and height for its life";
}

}  // namespace ptrhost
