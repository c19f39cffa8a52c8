// The round loop of a resumable frame, stated once for one partition: the frame of one device (frame.cpp, include/ptr_frame.h) is its
// one-partition case on the calling thread, the frame on several devices (multi_frame.cpp, include/ptr_multi_frame.h) runs it on every
// partition's thread in lock step.  Beside it, what a partition of either frame keeps and the sample step over that.  The sources and
// the state's owner are adaptive_host.h's, the class kernels frame.h's, the exchange multi_host.h's.  Internal: not part of the C-ABI.
#pragma once

#include <functional>
#include <vector>

#include "../kernels/frame.h"
#include "../kernels/multi.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "multi_host.h"

namespace ptrhost {

// What one partition of a resumable frame keeps for the frame's life, on its device.  A PtrFrame is one partition of one.
struct FramePart {
    ptrk::MultiPart mp{};
    uint32_t local = 0;                // its pixels
    PtrDeviceScene* scene = nullptr;   // not owned; null: the test-only frame
    AdaptiveStore store;   // the state, image order; L_p's two buffers; the compaction's scratch and the class-minimum word
    DeviceBuffer<uint32_t> order, listS;   // the first list; S_p
    DeviceBuffer<uint8_t> inS;             // the flag "in S_p" per entry of L_p
    // the test-only frame: the samples it was given (all of the image's), and the accumulators of a pass gathered from them
    DeviceBuffer<float4> probeSamples, probeItems;
};

// what the sample steps of one call on a partition share; sampleCount: of the test-only frame; `sum` (nullable) collects the stats
SampleStep sampleStep(FramePart& me, const PtrSettings& settings, uint32_t sampleCount, hipStream_t stream, PtrRenderStats* sum);

struct ClassMove {
    uint32_t from, to;
    uint64_t pixels;
};

// What the partitions of one refine share.  They tell each other |L_p|, the smallest n in L_p and |S_p| of the round between two
// meetings; every thread computes the same figures from them, and partition 0's writes the results.
struct RefineCall {
    const char* who = "";
    PtrAdaptiveParams params{};
    uint32_t parts = 1;
    bool empty = false;    // the frame holds no sample yet: the call begins with minSpp for every pixel
    const HaloExchange* ex = nullptr;   // parts > 1
    std::vector<uint32_t> pubActive, pubMin, pubInClass;
    // the results: the call's info but for pixelsAtMax, the pixels each step moved between counts, the most samples one pixel got
    PtrAdaptiveInfo info{};
    std::vector<ClassMove> moves;
    uint32_t deepest = 0;

    RefineCall(const char* who, const PtrAdaptiveParams& params, uint32_t parts, bool empty, const HaloExchange* ex)
        : who(who), params(params), parts(parts), empty(empty), ex(ex), pubActive(parts, 0u), pubMin(parts, ptrk::kFrameNoCount), pubInClass(parts, 0u) {}
};

// PTR_VERBOSE=launches: the events the loop records on the partition's stream where `marks` holds them, in pairs around the publish
// half of the exchange, its collect half, the class minimum, the split and the merge of a round ...
enum RoundMark { kMarkPublish = 0, kMarkCollect = 2, kMarkMinimum = 4, kMarkSplit = 6, kMarkMerge = 8, kRoundMarks = 10 };
// ... and what it tells the caller once per round in which the partition's S_p is not empty, with the stream joined behind the merge
struct RoundReport {
    uint32_t round, nMin, inClass, activeBefore, spp;
};
using RoundReporter = std::function<void(const RoundReport&)>;

// The rounds of one refine on partition p: class minimum -> split -> an ordinary pass over S_p -> update -> select on S_p merged into
// L_p, with the edge rows of e exchanged through dEdge (parts > 1) and a meeting before and behind every merge.  meet() is false once
// a partition has failed, and the loop then returns at once.  Returns the samples the partition took.
uint64_t refinePartition(RefineCall& call, uint32_t p, FramePart& me, float* dEdge, const SampleStep& step, const std::function<bool()>& meet,
                         const EventSet& marks, const RoundReporter& report);

}  // namespace ptrhost
