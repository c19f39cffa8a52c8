// The round loop of a resumable frame for one partition, and the sample step over what a partition keeps (frame_rounds.h).  Compiled
// with hipcc (host code only).
#include <algorithm>

#include "frame_rounds.h"

using namespace ptrk;

namespace ptrhost {

SampleStep sampleStep(FramePart& me, const PtrSettings& settings, uint32_t sampleCount, hipStream_t stream, PtrRenderStats* sum) {
    const size_t pixels = static_cast<size_t>(me.mp.width) * me.mp.height;
    return SampleStep{me.scene ? tracedSource(*me.scene, settings, stream) : gatheredSource(me.probeSamples.ptr, pixels, sampleCount, me.probeItems, stream),
                      maxPassItems(me.scene), me.store.state(), stream, sum};
}

uint64_t refinePartition(RefineCall& call, uint32_t p, FramePart& me, float* dEdge, const SampleStep& step, const std::function<bool()>& meet,
                         const EventSet& marks, const RoundReporter& report) {
    const PtrAdaptiveParams& params = call.params;
    const uint32_t parts = call.parts, width = me.mp.width, height = me.mp.height;
    hipStream_t stream = step.stream;
    const AdaptiveState& st = step.state;
    const AdaptiveScratch scratch = me.store.scratch();
    uint64_t samples = 0u;
    auto mark = [&](int i) { if (marks[i]) HIP_CHECK(hipEventRecord(marks[i], stream)); };
    // the publish half of the exchange behind the last sub-pass of an update (addSamples' hook: inside the pass, before the source
    // joins the stream, so the outbox is written when addSamples returns)
    const SubPassHook publish = [&](uint32_t, uint32_t, bool last) {
        if (last && parts > 1u) haloPublish(me.mp, st.e, dEdge, *call.ex, stream, marks[kMarkPublish], marks[kMarkPublish + 1]);
    };
    auto addTo = [&](const uint32_t* list, uint32_t count, uint32_t nBefore, uint32_t spp) {
        addSamples(step, list, count, nBefore, spp, publish);
        HIP_CHECK(hipGetLastError());
        if (parts > 1u) HIP_CHECK(hipStreamSynchronize(stream));   // (the source joined the stream already: the outbox is written)
        samples += static_cast<uint64_t>(count) * spp;
    };
    // the length of the list a select, a split or a merge just wrote, and (with `min`) the class minimum beside it
    auto readWords = [&](uint32_t* total, uint32_t* min) {
        uint32_t words[2] = {0u, 0u};
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(words, scratch.total, (min ? 2u : 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        *total = words[0];
        if (min) *min = words[1];
    };
    // The smallest n in a list.  It reads n only, so it may run behind the merge that wrote the list: it must be published before the
    // meeting that precedes the round it is for.
    auto classMin = [&](const uint32_t* list, uint32_t count) {
        uint32_t ignored = 0u, min = kFrameNoCount;
        mark(kMarkMinimum);
        HIP_CHECK(hipMemsetAsync(me.store.minWord(), 0xFF, sizeof(uint32_t), stream));   // kFrameNoCount
        launchFrameClassMin(list, count, st.n, me.store.minWord(), stream);
        mark(kMarkMinimum + 1);
        readWords(&ignored, &min);
        return min;
    };
    // after a meeting: the sum of |L_p|, the smallest n over all lists, the sum of |S_p|
    uint64_t total = 0u, inClassTotal = 0u;
    uint32_t nMin = kFrameNoCount;
    auto sumUp = [&] {
        total = inClassTotal = 0u;
        nMin = kFrameNoCount;
        for (uint32_t q = 0; q < parts; ++q) {
            total += call.pubActive[q];
            inClassTotal += call.pubInClass[q];
            nMin = std::min(nMin, call.pubMin[q]);
        }
    };
    // partition 0 keeps the call's books
    auto note = [&](uint32_t from, uint32_t spp, uint64_t pixels) {
        if (p != 0u) return;
        call.moves.push_back(ClassMove{from, from + spp, pixels});
        call.info.totalSamples += pixels * spp;
        call.deepest = std::max(call.deepest, spp);
        if (call.info.rounds < PTR_ADAPTIVE_INFO_ROUNDS) call.info.activeAfter[call.info.rounds] = static_cast<uint32_t>(total);
        ++call.info.rounds;
    };

    if (call.empty) {
        if (me.local) addTo(me.order.ptr, me.local, 0u, params.minSpp);
        if (!meet()) return samples;   // every partition has published
    }
    // the start list, and with it this partition's share of the first round's class minimum
    uint32_t turn = 0u, active = 0u, myMin = kFrameNoCount;
    if (me.local) {
        if (parts > 1u) haloCollect(me.mp, dEdge, st.e, *call.ex, stream);
        launchAdaptiveSelect(me.order.ptr, me.local, width, height, st, params.maxSpp, params.threshold, scratch, me.store.list(0u), stream);
        readWords(&active, nullptr);
        if (active) myMin = classMin(me.store.list(0u), active);
    }
    call.pubActive[p] = active, call.pubMin[p] = myMin;
    if (!meet()) return samples;   // every start list is known; the outboxes may be overwritten again
    sumUp();
    if (call.empty) note(0u, params.minSpp, static_cast<uint64_t>(width) * height);
    for (uint32_t round = 0u; total > 0u; ++round) {
        if (nMin >= params.maxSpp) throw HipError{std::string(call.who) + ": an active list holds a pixel at maxSpp"};   // (select never keeps one)
        const uint32_t k = std::min(params.stepSpp, params.maxSpp - nMin);
        const uint32_t* list = me.store.list(turn);
        // 1. S_p and its samples; behind the last update the edge rows of e go to the outbox
        uint32_t inClass = 0u;
        if (active > 0u && myMin == nMin) {
            mark(kMarkSplit);
            launchFrameSplit(list, active, st.n, nMin, me.inS.ptr, scratch, me.listS.ptr, stream);
            mark(kMarkSplit + 1);
            readWords(&inClass, nullptr);
            if (inClass == 0u || inClass > active) throw HipError{std::string(call.who) + ": the class of the round is empty"};
            addTo(me.listS.ptr, inClass, nMin, k);
        }
        // 2. every partition has published
        if (!meet()) return samples;
        // 3. the neighbours' rows, select on S_p merged into L_p, the next list's length and minimum
        if (inClass > 0u) {
            const uint32_t before = active;
            if (parts > 1u) haloCollect(me.mp, dEdge, st.e, *call.ex, stream, marks[kMarkCollect], marks[kMarkCollect + 1]);
            mark(kMarkMerge);
            launchFrameMerge(list, active, me.inS.ptr, width, height, st, params.maxSpp, params.threshold, scratch, me.store.list(turn ^ 1u), stream);
            mark(kMarkMerge + 1);
            readWords(&active, nullptr);
            turn ^= 1u;
            if (report) report(RoundReport{round, nMin, inClass, before, k});   // (before the next minimum records its events again)
            myMin = active ? classMin(me.store.list(turn), active) : kFrameNoCount;
        }
        call.pubActive[p] = active, call.pubMin[p] = myMin, call.pubInClass[p] = inClass;
        // 4. every list is known; the outboxes may be overwritten again
        if (!meet()) return samples;
        // 5. the same totals on every thread: all leave or all go on
        const uint32_t from = nMin;
        sumUp();
        note(from, k, inClassTotal);
    }
    return samples;
}

}  // namespace ptrhost
