// Host side of include/ptr_multi_frame.h: the resumable frame on several devices.  The frame object - per partition a resident scene, a
// stream, the state's owner, the first list, S and the buffers of the exchange and the checkpoint; on the first device the gather
// buffers; on the host the count classes - the argument checks, and one driver that runs a call's partitions on threads which meet at
// a round barrier (round_barrier.h) and end together when one of them fails.  The only loop of its own is ptr_frame.h's refine run in
// lock step over the partitions; the sample step, the sources and the state's owner are adaptive_host.h's, the class kernels frame.h's,
// the exchange, the device list and the hand-over to the first device multi_host.h's, finish and interleave multi.h's.  The frame
// object, what a partition keeps and the partition driver are declared in multi_frame_host.h, which multi_dynamic.cpp shares.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/frame.h"
#include "../kernels/multi.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "knobs.h"
#include "multi_frame_host.h"
#include "multi_host.h"
#include "parallel.h"
#include "ptr_multi_frame.h"
#include "round_barrier.h"

using namespace ptrhost;
using namespace ptrk;

namespace {

constexpr uint32_t kOutWords = 10u;   // a partition's outputs in band layout: rgb 3, cov 6, count 1 words per pixel, one after the other

void destroy(PtrMultiFrame* f) {
    if (!f) return;
    for (auto& me : f->part) {
        if (!me) continue;
        (void)hipSetDevice(me->device);
        if (me->stream) {
            (void)hipStreamSynchronize(me->stream);
            (void)hipStreamDestroy(me->stream);
        }
        me.reset();
    }
    (void)hipSetDevice(f->rootDevice);
    delete f;
}
struct Destroy {
    void operator()(PtrMultiFrame* f) const { destroy(f); }
};

void beginCall(PtrMultiFrame& f) {
    std::memset(&f.last, 0, sizeof(f.last));
    f.last.parts = f.parts;
}

// what the sample steps of one call on a partition share; `sum` (nullable) collects the stats
SampleStep sampleStep(PtrMultiFrame& f, Part& me, PtrRenderStats* sum) {
    return SampleStep{me.scene ? tracedSource(*me.scene, f.settings, me.stream)
                               : gatheredSource(me.probeSamples.ptr, f.pixels, f.sampleCount, me.probeItems, me.stream),
                      maxPassItems(me.scene.get()), me.store.state(), me.stream, sum};
}

// the publish half of the exchange behind the last sub-pass of an update (addSamples' hook: inside the pass, before the source joins
// the stream, so the outbox is written when addSamples returns)
SubPassHook publishBehindLast(const PtrMultiFrame& f, const Part& me, hipEvent_t before = nullptr, hipEvent_t after = nullptr) {
    return [&f, &me, before, after](uint32_t, uint32_t, bool last) {
        if (last && f.parts > 1u) haloPublish(me.mp, me.store.e.ptr, me.edge.ptr, f.ex, me.stream, before, after);
    };
}

// a call's stats as ptr_multi.h has them: the slowest partition's time, launches summed, the samples of the call
void fillStats(const PtrMultiFrame& f, const std::vector<PtrRenderStats>& partStats, uint64_t samples, uint32_t deepest, PtrRenderStats* stats) {
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    for (uint32_t p = 0; p < f.parts; ++p) {
        stats->totalSeconds = std::max(stats->totalSeconds, f.last.partRenderSeconds[p]);
        addLaunchStats(*stats, partStats[p]);
    }
    stats->avgMsPerSample = stats->totalSeconds * 1000.0 / std::max(1u, deepest);
    stats->samples = samples;
}

void zeroState(PtrMultiFrame& f) {
    runParts(f, [&](Part& me, uint32_t, const auto&) {
        me.store.zero(me.stream);
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.ex.publishZeros();
    f.classes.clear();
    f.classes[0u] = f.pixels;
}

void accumulate(PtrMultiFrame& f, uint32_t spp, PtrRenderStats* stats) {
    const uint32_t n = f.minCount();
    std::vector<PtrRenderStats> partStats(f.parts);
    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto&) {
        if (!me.local) return;
        PtrRenderStats sum{};
        addSamples(sampleStep(f, me, stats ? &sum : nullptr), me.order.ptr, me.local, n, spp, publishBehindLast(f, me));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(me.stream));
        partStats[p] = sum;
        f.last.partSamples[p] = static_cast<uint64_t>(me.local) * spp;
    });
    f.classes.clear();
    f.classes[n + spp] = f.pixels;
    fillStats(f, partStats, static_cast<uint64_t>(f.pixels) * spp, spp, stats);
}

void refine(PtrMultiFrame& f, const PtrAdaptiveParams& params, PtrRenderStats* stats, PtrAdaptiveInfo* info) {
    const uint32_t parts = f.parts, width = f.width, height = f.height;
    const bool empty = f.empty();
    // what the partitions tell each other between two meetings: |L_p|, the smallest n in L_p, |S_p| of the round
    std::vector<uint32_t> pubActive(parts, 0u), pubMin(parts, kFrameNoCount), pubInClass(parts, 0u);
    std::vector<PtrRenderStats> partStats(parts);
    // written by partition 0's thread (every thread computes the same figures): the call's info, and the pixels every round moved
    // from n_min to n_min + k, which the classes follow once the threads are back
    PtrAdaptiveInfo local{};
    struct Move {
        uint32_t from, to;
        uint64_t pixels;
    };
    std::vector<Move> moves;
    uint32_t deepest = 0u;
    auto note = [&](uint64_t active) {
        if (local.rounds < PTR_ADAPTIVE_INFO_ROUNDS) local.activeAfter[local.rounds] = static_cast<uint32_t>(active);
        ++local.rounds;
    };
    const bool timed = parts > 1u && ptr::readKnobs().verboseLaunches;

    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto& meet) {
        hipStream_t stream = me.stream;
        PtrRenderStats sum{};
        const SampleStep step = sampleStep(f, me, stats ? &sum : nullptr);
        const AdaptiveState& st = step.state;
        const AdaptiveScratch scratch = me.store.scratch();
        // PTR_VERBOSE=launches: device events around the two halves of the exchange (tools/multi_frame_cost.py parses the line)
        EventSet marks;
        if (timed) marks.create(4u);
        const SubPassHook publish = publishBehindLast(f, me, marks[0], marks[1]);
        // the length of the list a select, a split or a merge just wrote, and (with `min`) the class minimum beside it
        auto readWords = [&](uint32_t* total, uint32_t* min) {
            uint32_t words[2] = {0u, 0u};
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(words, scratch.total, (min ? 2u : 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            *total = words[0];
            if (min) *min = words[1];
        };
        auto classMin = [&](const uint32_t* list, uint32_t count) {
            uint32_t ignored = 0u, min = kFrameNoCount;
            HIP_CHECK(hipMemsetAsync(me.store.minWord(), 0xFF, sizeof(uint32_t), stream));   // kFrameNoCount
            launchFrameClassMin(list, count, st.n, me.store.minWord(), stream);
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
                total += pubActive[q];
                inClassTotal += pubInClass[q];
                nMin = std::min(nMin, pubMin[q]);
            }
        };

        if (empty) {
            if (me.local) {
                addSamples(step, me.order.ptr, me.local, 0u, params.minSpp, publish);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipStreamSynchronize(stream));
                f.last.partSamples[p] += static_cast<uint64_t>(me.local) * params.minSpp;
            }
            if (!meet()) return;   // every partition has published
        }
        // the start list, and with it this partition's share of the first round's class minimum
        uint32_t turn = 0u, active = 0u, myMin = kFrameNoCount;
        if (me.local) {
            if (parts > 1u) haloCollect(me.mp, me.edge.ptr, st.e, f.ex, stream);
            launchAdaptiveSelect(me.order.ptr, me.local, width, height, st, params.maxSpp, params.threshold, scratch, me.store.list(0u), stream);
            readWords(&active, nullptr);
            if (active) myMin = classMin(me.store.list(0u), active);
        }
        pubActive[p] = active, pubMin[p] = myMin;
        if (!meet()) return;   // every start list is known; the outboxes may be overwritten again
        sumUp();
        if (p == 0u) {
            if (empty) {
                local.totalSamples += static_cast<uint64_t>(f.pixels) * params.minSpp;
                deepest = params.minSpp;
                note(total);
            }
        }
        for (uint32_t round = 0u; total > 0u; ++round) {
            if (nMin >= params.maxSpp) throw HipError{"ptr_multi_frame_refine: an active list holds a pixel at maxSpp"};   // (select never keeps one)
            const uint32_t k = std::min(params.stepSpp, params.maxSpp - nMin);
            const uint32_t* list = me.store.list(turn);
            // 1. S_p and its samples; behind the last update the edge rows of e go to the outbox
            uint32_t inClass = 0u;
            if (active > 0u && myMin == nMin) {
                launchFrameSplit(list, active, st.n, nMin, me.inS.ptr, scratch, me.listS.ptr, stream);
                readWords(&inClass, nullptr);
                if (inClass == 0u || inClass > active) throw HipError{"ptr_multi_frame_refine: the class of the round is empty"};
                addSamples(step, me.listS.ptr, inClass, nMin, k, publish);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipStreamSynchronize(stream));   // (the source joined the stream already: the outbox is written)
                f.last.partSamples[p] += static_cast<uint64_t>(inClass) * k;
            }
            // 2. every partition has published
            if (!meet()) return;
            // 3. the neighbours' rows, select on S_p merged into L_p, the next list's length and minimum
            if (inClass > 0u) {
                if (parts > 1u) haloCollect(me.mp, me.edge.ptr, st.e, f.ex, stream, marks[2], marks[3]);
                launchFrameMerge(list, active, me.inS.ptr, width, height, st, params.maxSpp, params.threshold, scratch, me.store.list(turn ^ 1u), stream);
                readWords(&active, nullptr);
                turn ^= 1u;
                myMin = active ? classMin(me.store.list(turn), active) : kFrameNoCount;
                if (timed) {
                    float outMs = 0.0f, inMs = 0.0f;
                    HIP_CHECK(hipEventElapsedTime(&outMs, marks[0], marks[1]));
                    HIP_CHECK(hipEventElapsedTime(&inMs, marks[2], marks[3]));
                    std::fprintf(stderr, "[multi-frame] partition %u round %u: class %u, %u entries x %u spp; halo %zu bytes each way; pack + copy %.4f ms, copy + unpack %.4f ms\n",
                                 p, round, nMin, inClass, k, f.ex.haloBytes(p), outMs, inMs);
                }
            }
            pubActive[p] = active, pubMin[p] = myMin, pubInClass[p] = inClass;
            // 4. every list is known; the outboxes may be overwritten again
            if (!meet()) return;
            // 5. the same totals on every thread: all leave or all go on
            const uint32_t from = nMin;
            sumUp();
            if (p == 0u) {
                moves.push_back(Move{from, from + k, inClassTotal});
                local.totalSamples += inClassTotal * k;
                deepest = std::max(deepest, k);
                note(total);
            }
        }
        partStats[p] = sum;
    });

    if (empty) {
        f.classes.clear();
        f.classes[params.minSpp] = f.pixels;
    }
    for (const Move& mv : moves) {
        auto it = f.classes.find(mv.from);
        if (it != f.classes.end()) {   // (always, unless an import brought counts that disagree with themselves)
            it->second -= std::min<uint64_t>(it->second, mv.pixels);
            if (it->second == 0u) f.classes.erase(it);
        }
        f.classes[mv.to] += mv.pixels;
    }
    const auto atMax = f.classes.find(params.maxSpp);
    local.pixelsAtMax = atMax == f.classes.end() ? 0u : static_cast<uint32_t>(atMax->second);
    fillStats(f, partStats, local.totalSamples, deepest, stats);
    if (info) *info = local;
}

// every partition's outputs, in band layout, on the first device
void gatherBands(PtrMultiFrame& f) {
    std::atomic<uint32_t> staged{0};
    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto&) {
        const size_t mine = multiBandPixels(me.mp);
        if (!mine) return;
        me.bandOut.ensure(mine * kOutWords);
        float* const dRgb = me.bandOut.ptr;
        launchMultiFinishBands(me.mp, me.store.state(), dRgb, dRgb + mine * 3u, reinterpret_cast<uint32_t*>(dRgb + mine * 9u), me.stream);
        HIP_CHECK(hipGetLastError());
        if (sendBandsToRoot(f.gathered.ptr + f.wordOffset[p], f.rootDevice, dRgb, me.device, mine * kOutWords * sizeof(float), me.forceStaged, me.stream)) {
            staged.fetch_add(1);
        }
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.last.stagedParts = staged.load();
}

// ... and from there into image order (dCov and dCount nullable), on `stream` of the first device, which is joined
void interleave(PtrMultiFrame& f, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(f.rootDevice));
    launchMultiInterleave(f.gathered.ptr, f.dWordOffset.ptr, f.parts, f.width, f.height, 3u, dRgb, stream);
    if (dCov) launchMultiInterleave(f.gathered.ptr, f.dWordOffset.ptr + f.parts, f.parts, f.width, f.height, 6u, dCov, stream);
    if (dCount) launchMultiInterleave(f.gathered.ptr, f.dWordOffset.ptr + 2u * f.parts, f.parts, f.width, f.height, 1u, dCount, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
}

// PTR_VERBOSE=launches: one of the two checkpoint kernels between device events (tools/multi_frame_cost.py parses the line).  The
// bytes are the ones it moves: 14 words read and 14 written per own pixel.
template <typename Launch>
void timedStateKernel(const char* name, const Part& me, bool timed, Launch&& launch) {
    EventSet marks;
    if (timed) {
        marks.create(2u);
        HIP_CHECK(hipEventRecord(marks[0], me.stream));
    }
    launch();
    HIP_CHECK(hipGetLastError());
    if (!timed) return;
    HIP_CHECK(hipEventRecord(marks[1], me.stream));
    HIP_CHECK(hipEventSynchronize(marks[1]));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, marks[0], marks[1]));
    std::fprintf(stderr, "[multi-frame] partition %u %s: %zu bytes, %.4f ms\n", me.mp.part, name,
                 static_cast<size_t>(me.local) * kMultiStateWords * sizeof(float) * 2u, ms);
}

void exportState(PtrMultiFrame& f, float* sum, float* mean, float* m, uint32_t* n, float* e) {
    const AdaptiveState image{sum, mean, m, n, e};
    const bool timed = ptr::readKnobs().verboseLaunches;
    runParts(f, [&](Part& me, uint32_t, const auto&) {
        const size_t mine = multiBandPixels(me.mp);
        if (!mine) return;
        me.packed.ensure(mine * kMultiStateWords);
        me.hostPacked.assign(mine * kMultiStateWords, 0.0f);
        timedStateKernel("k_multi_state_pack", me, timed, [&] { launchMultiStatePack(me.mp, me.store.state(), me.packed.ptr, me.stream); });
        HIP_CHECK(hipMemcpyAsync(me.hostPacked.data(), me.packed.ptr, mine * kMultiStateWords * sizeof(float), hipMemcpyDeviceToHost, me.stream));
        HIP_CHECK(hipStreamSynchronize(me.stream));
        // the partition's rows of the caller's image-order arrays (no two partitions share a row)
        for (uint32_t i = 0; i < mine; ++i) multiStateUnpack(me.mp, i, me.hostPacked.data(), image);
    });
}

void importState(PtrMultiFrame& f, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e) {
    // (the pack body reads through the state's pointers only)
    const AdaptiveState image{const_cast<float*>(sum), const_cast<float*>(mean), const_cast<float*>(m), const_cast<uint32_t*>(n), const_cast<float*>(e)};
    const bool timed = ptr::readKnobs().verboseLaunches;
    runParts(f, [&](Part& me, uint32_t, const auto&) {
        const size_t mine = multiBandPixels(me.mp);
        if (!mine) return;
        me.packed.ensure(mine * kMultiStateWords);
        me.hostPacked.assign(mine * kMultiStateWords, 0.0f);
        for (uint32_t i = 0; i < mine; ++i) multiStatePack(me.mp, i, image, me.hostPacked.data());
        HIP_CHECK(hipMemcpyAsync(me.packed.ptr, me.hostPacked.data(), mine * kMultiStateWords * sizeof(float), hipMemcpyHostToDevice, me.stream));
        timedStateKernel("k_multi_state_unpack", me, timed, [&] { launchMultiStateUnpack(me.mp, me.packed.ptr, me.store.state(), me.stream); });
        if (f.parts > 1u) haloPublish(me.mp, me.store.e.ptr, me.edge.ptr, f.ex, me.stream);
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.classes.clear();
    for (size_t p = 0; p < f.pixels; ++p) ++f.classes[n[p]];
}

std::string badSize(const std::string& w, uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u) return w + ": render size must be non-zero";
    if (pastIndexLimit(static_cast<uint64_t>(width) * height + static_cast<uint64_t>(PTR_BAND_ROWS) * width)) return w + ": image too large for a frame";
    return std::string();
}

}  // namespace

// Create, for every entry point: a scene (or, for the test-only frame, samples), the size, the devices asked for (multi_frame_host.h).
int ptrhost::createMultiFrame(const char* who, const PtrSceneDesc* scene, const PtrSettings* settings, const float* samples, uint32_t sampleCount,
                              bool sceneless, const int* ids, int n, bool listed, bool dynamic, uint32_t dynamicFlags, PtrMultiFrame** out, char* err,
                              size_t cap) {
    const std::string w(who);
    if (!(sceneless ? samples != nullptr : scene != nullptr) || !settings || !out || (listed && !ids)) return nullArgument(who, err, cap);
    std::string bad = badSize(w, settings->width, settings->height);
    if (bad.empty() && sceneless && sampleCount == 0u) bad = w + ": sample_count must be >= 1";
    if (bad.empty()) bad = badDeviceRequest(w, listed, n);
    if (!bad.empty()) return refuse(err, cap, bad);
    std::vector<int> devices;
    std::vector<char> forceStaged;
    if (const int rc = pickDevices(who, ids, n, listed, settings->height, devices, forceStaged, err, cap)) return rc;
    try {
        std::unique_ptr<PtrMultiFrame, Destroy> f(new PtrMultiFrame);
        f->settings = *settings;
        f->width = settings->width, f->height = settings->height;
        f->pixels = static_cast<size_t>(f->width) * f->height;
        f->parts = static_cast<uint32_t>(devices.size());
        f->sceneless = sceneless, f->sampleCount = sampleCount;
        f->rootDevice = devices[0];
        PreparedScene prepared;
        if (!sceneless) prepareScene(*scene, prepared, nullptr, dynamic, dynamicFlags);   // once, for every device
        if (dynamic) {
            f->dynamic = std::make_unique<MultiDynamic>();
            f->dynamic->flags = dynamicFlags;
        }

        const uint32_t parts = f->parts;
        std::vector<uint32_t> partBands(parts, 0u);
        std::vector<uint64_t> partPixel(parts + 1u, 0u);   // where partition p's band buffer starts among all of them, in pixels
        for (uint32_t p = 0; p < parts; ++p) {
            partBands[p] = ptr_part_band_count(f->height, p, parts);
            partPixel[p + 1u] = partPixel[p] + static_cast<uint64_t>(partBands[p]) * PTR_BAND_ROWS * f->width;
            auto me = std::make_unique<Part>();
            me->device = devices[p];
            me->forceStaged = forceStaged[p] != 0;
            me->mp = MultiPart{p, parts, partBands[p], f->width, f->height};
            f->part.push_back(std::move(me));
        }
        f->wordOffset.assign(static_cast<size_t>(parts) * 3u, 0u);
        for (uint32_t p = 0; p < parts; ++p) {
            const uint64_t start = partPixel[p] * kOutWords, mine = partPixel[p + 1u] - partPixel[p];
            f->wordOffset[p] = start;
            f->wordOffset[parts + p] = start + mine * 3u;
            f->wordOffset[2u * parts + p] = start + mine * 9u;
        }
        HIP_CHECK(hipSetDevice(f->rootDevice));
        f->gathered.ensure(static_cast<size_t>(partPixel[parts]) * kOutWords);
        f->image.ensure(f->pixels * kOutWords);
        f->dWordOffset.upload(f->wordOffset.data(), f->wordOffset.size());
        if (parts > 1u) f->ex.allocate(partBands, f->width);

        PtrMultiFrame& fr = *f;
        runParts(fr, [&](Part& me, uint32_t p, const auto&) {
            if (!sceneless) {
                me.scene = std::make_unique<PtrDeviceScene>();
                me.scene->device = me.device;
                uploadScene(*scene, prepared, *me.scene);
                HIP_CHECK(hipSetDevice(me.device));
            }
            HIP_CHECK(hipStreamCreateWithFlags(&me.stream, hipStreamNonBlocking));
            std::vector<uint32_t> order;
            partitionPixels(fr.width, fr.height, p, parts, order);
            me.local = static_cast<uint32_t>(order.size());
            me.store.ensure(fr.pixels);   // image order: the lists name image pixels, select reads e around them
            me.order.upload(order.data(), order.size());
            me.listS.ensure(me.local);
            me.inS.ensure(me.local);
            me.edge.ensure(static_cast<size_t>(me.mp.bands) * 2u * fr.width);
            if (sceneless) me.probeSamples.upload(reinterpret_cast<const float4*>(samples), fr.pixels * sampleCount);
            me.store.zero(me.stream);
            HIP_CHECK(hipStreamSynchronize(me.stream));
        });
        f->classes[0u] = f->pixels;
        beginCall(*f);
        *out = f.release();
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

// what every call on an existing frame refuses first
int ptrhost::refuseBroken(const char* who, const PtrMultiFrame* f, char* err, size_t cap) {
    return f->broken ? refuse(err, cap, std::string(who) + ": an earlier call failed on a device; the frame can only be released") : 0;
}

extern "C" {

int ptr_multi_frame_create(const PtrSceneDesc* scene, const PtrSettings* settings, int n_devices, PtrMultiFrame** out_frame, char* err,
                           size_t err_cap) {
    return createMultiFrame("ptr_multi_frame_create", scene, settings, nullptr, 0u, false, nullptr, n_devices, false, false, 0u, out_frame, err, err_cap);
}

int ptr_multi_frame_debug_create_on(const PtrSceneDesc* scene, const PtrSettings* settings, const int* device_ids, int n,
                                    PtrMultiFrame** out_frame, char* err, size_t err_cap) {
    return createMultiFrame("ptr_multi_frame_debug_create_on", scene, settings, nullptr, 0u, false, device_ids, n, true, false, 0u, out_frame, err, err_cap);
}

int ptr_multi_frame_debug_create(uint32_t width, uint32_t height, const float* samples, uint32_t sample_count, const int* device_ids, int n,
                                 PtrMultiFrame** out_frame, char* err, size_t err_cap) {
    PtrSettings size{};
    size.width = width, size.height = height;
    return createMultiFrame("ptr_multi_frame_debug_create", nullptr, &size, samples, sample_count, true, device_ids, n, true, false, 0u, out_frame, err, err_cap);
}

void ptr_multi_frame_release(PtrMultiFrame* frame) { destroy(frame); }

int ptr_multi_frame_reset(PtrMultiFrame* frame, const PtrSettings* settings, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_reset";
    if (!frame) return nullArgument(who, err, err_cap);
    if (settings && (settings->width != frame->width || settings->height != frame->height)) {
        return refuse(err, err_cap, std::string(who) + ": a frame keeps its width and height for its life");
    }
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    try {
        if (settings) frame->settings = *settings;
        zeroState(*frame);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_accumulate(PtrMultiFrame* frame, uint32_t spp, PtrRenderStats* stats, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_accumulate";
    if (!frame) return nullArgument(who, err, err_cap);
    if (spp == 0u) return refuse(err, err_cap, std::string(who) + ": spp must be >= 1");
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    if (!frame->uniform()) {
        return refuse(err, err_cap, std::string(who) + ": the frame is not uniform (its pixels hold different sample counts); a refine with threshold 0 "
                                                       "brings every pixel with a non-zero error up to a common count");
    }
    if (static_cast<uint64_t>(frame->minCount()) + spp > 0xFFFFFFF0ull) return refuse(err, err_cap, std::string(who) + ": too many samples");
    if (frame->sceneless && static_cast<uint64_t>(frame->minCount()) + spp > frame->sampleCount) {
        return refuse(err, err_cap, std::string(who) + ": a sample past the ones the frame was given");
    }
    try {
        accumulate(*frame, spp, stats);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_refine(PtrMultiFrame* frame, const PtrAdaptiveParams* params, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                           size_t err_cap) {
    static const char* const who = "ptr_multi_frame_refine";
    if (!frame || !params) return nullArgument(who, err, err_cap);
    const std::string bad = badAdaptiveParams(who, *params);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    if (!frame->empty() && frame->minCount() < 2u) {
        return refuse(err, err_cap, std::string(who) + ": every pixel of a frame that is not empty must hold at least 2 samples");
    }
    if (frame->sceneless && params->maxSpp > frame->sampleCount) return refuse(err, err_cap, std::string(who) + ": a sample past the ones the frame was given");
    try {
        refine(*frame, *params, stats, info);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_resolve_device(PtrMultiFrame* frame, void* d_out_rgb, void* d_out_cov, void* d_out_count, void* stream, char* err,
                                   size_t err_cap) {
    static const char* const who = "ptr_multi_frame_resolve_device";
    if (!frame || !d_out_rgb) return nullArgument(who, err, err_cap);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    try {
        gatherBands(*frame);
        interleave(*frame, static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_cov), static_cast<uint32_t*>(d_out_count),
                   static_cast<hipStream_t>(stream));
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_resolve(PtrMultiFrame* frame, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo, float* out_normal,
                            char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_resolve";
    if (!frame || !out_rgb) return nullArgument(who, err, err_cap);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    if (frame->sceneless && (out_albedo || out_normal)) return refuse(err, err_cap, std::string(who) + ": a frame without a scene has no feature buffers");
    try {
        PtrMultiFrame& f = *frame;
        gatherBands(f);
        finishAndDownload(f.image, f.pixels, out_rgb, out_cov, out_count,
                          [&](float* dRgb, float* dCov, uint32_t* dCount) { interleave(f, dRgb, dCov, dCount, nullptr); });
        if (out_albedo || out_normal) {   // the first partition's scene is on the first device
            PtrDeviceScene& scene = *f.part[0]->scene;
            RenderParams rp;
            fillRenderParams(f.settings, 1u, rp);
            f.albedo.ensure(f.pixels);
            f.normal.ensure(f.pixels);
            launchAovs(rp, scene.view, 0u, f.albedo.ptr, f.normal.ptr, coldLaunchConfig(scene), nullptr);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipDeviceSynchronize());
            if (out_albedo) f.albedo.download(reinterpret_cast<float4*>(out_albedo), f.pixels);
            if (out_normal) f.normal.download(reinterpret_cast<float4*>(out_normal), f.pixels);
        }
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_info(const PtrMultiFrame* frame, PtrFrameInfo* out, PtrMultiInfo* multi_info) {
    if (!frame || !out) return 1;
    *out = PtrFrameInfo{};
    out->width = frame->width;
    out->height = frame->height;
    out->minCount = frame->minCount();
    out->maxCount = frame->maxCount();
    for (const auto& c : frame->classes) out->totalSamples += static_cast<uint64_t>(c.first) * c.second;
    out->uniform = frame->uniform() ? 1u : 0u;
    if (multi_info) *multi_info = frame->last;
    return 0;
}

int ptr_multi_frame_export(PtrMultiFrame* frame, float* sum, float* mean, float* m, uint32_t* n, float* e, char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_export";
    if (!frame || !sum || !mean || !m || !n || !e) return nullArgument(who, err, err_cap);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    try {
        exportState(*frame, sum, mean, m, n, e);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_multi_frame_import(PtrMultiFrame* frame, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e,
                           char* err, size_t err_cap) {
    static const char* const who = "ptr_multi_frame_import";
    if (!frame || !sum || !mean || !m || !n || !e) return nullArgument(who, err, err_cap);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    try {
        importState(*frame, sum, mean, m, n, e);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
