// Host side of include/ptr_multi_frame.h: the resumable frame on several devices.  The frame object - per partition a resident scene, a
// stream, a FramePart (the state's owner, the first list, S) and the buffers of the exchange and the checkpoint; on the first device
// the gather; on the host the count classes - and the argument checks.  It adds no loop of its own: refine is the round loop of
// frame_rounds.h, which frame.cpp runs for one partition, run here on every partition's thread with the round barrier as its meeting and
// the exchange between the partitions.  The count classes and the refusals they decide are frame_classes.h's, the sample step, the
// sources and the state's owner adaptive_host.h's, the exchange, the device list, the hand-over to the first device, the gather there
// and the thread-per-partition driver multi_host.h's, finish and interleave multi.h's.  The frame object, what a partition keeps and
// the driver on a frame (runParts) are declared in multi_frame_host.h, which multi_dynamic.cpp shares.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "knobs.h"
#include "multi_frame_host.h"
#include "multi_host.h"
#include "ptr_multi_frame.h"

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
        me.fp.store.zero(me.stream);
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.ex.publishZeros();
    f.classes.reset(f.pixels);
}

void accumulate(PtrMultiFrame& f, uint32_t spp, PtrRenderStats* stats) {
    const uint32_t n = f.classes.minCount();
    std::vector<PtrRenderStats> partStats(f.parts);
    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto&) {
        if (!me.fp.local) return;
        PtrRenderStats sum{};
        // the publish half of the exchange behind the last sub-pass (addSamples' hook: inside the pass, before the source joins the stream)
        addSamples(sampleStep(me.fp, f.settings, f.sampleCount, me.stream, stats ? &sum : nullptr), me.fp.order.ptr, me.fp.local, n, spp, [&](uint32_t, uint32_t, bool last) {
            if (last && f.parts > 1u) haloPublish(me.fp.mp, me.fp.store.e.ptr, me.edge.ptr, f.ex, me.stream);
        });
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(me.stream));
        partStats[p] = sum;
        f.last.partSamples[p] = static_cast<uint64_t>(me.fp.local) * spp;
    });
    f.classes.move(n, n + spp, f.pixels);
    fillStats(f, partStats, static_cast<uint64_t>(f.pixels) * spp, spp, stats);
}

void refine(PtrMultiFrame& f, const PtrAdaptiveParams& params, PtrRenderStats* stats, PtrAdaptiveInfo* info) {
    RefineCall call("ptr_multi_frame_refine", params, f.parts, f.classes.empty(), &f.ex);
    std::vector<PtrRenderStats> partStats(f.parts);
    const bool timed = f.parts > 1u && ptr::readKnobs().verboseLaunches;

    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto& meet) {
        PtrRenderStats sum{};
        // PTR_VERBOSE=launches: device events around the two halves of the exchange (tools/multi_frame_cost.py parses the line)
        EventSet marks;
        if (timed) marks.create(kRoundMarks);
        auto report = [&](const RoundReport& r) {
            if (!timed) return;
            float outMs = 0.0f, inMs = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&outMs, marks[kMarkPublish], marks[kMarkPublish + 1]));
            HIP_CHECK(hipEventElapsedTime(&inMs, marks[kMarkCollect], marks[kMarkCollect + 1]));
            std::fprintf(stderr, "[multi-frame] partition %u round %u: class %u, %u entries x %u spp; halo %zu bytes each way; pack + copy %.4f ms, copy + unpack %.4f ms\n",
                         p, r.round, r.nMin, r.inClass, r.spp, f.ex.haloBytes(p), outMs, inMs);
        };
        const SampleStep step = sampleStep(me.fp, f.settings, f.sampleCount, me.stream, stats ? &sum : nullptr);
        f.last.partSamples[p] = refinePartition(call, p, me.fp, me.edge.ptr, step, meet, marks, report);
        partStats[p] = sum;
    });

    for (const ClassMove& mv : call.moves) f.classes.move(mv.from, mv.to, mv.pixels);
    call.info.pixelsAtMax = static_cast<uint32_t>(f.classes.pixelsAt(params.maxSpp));
    fillStats(f, partStats, call.info.totalSamples, call.deepest, stats);
    if (info) *info = call.info;
}

// every partition's outputs, in band layout, on the first device
void gatherBands(PtrMultiFrame& f) {
    std::atomic<uint32_t> staged{0};
    beginCall(f);
    runParts(f, [&](Part& me, uint32_t p, const auto&) {
        const size_t mine = f.bands.bandPixels(p);
        if (!mine) return;
        me.bandOut.ensure(mine * kOutWords);
        float* const dRgb = me.bandOut.ptr;
        launchMultiFinishBands(me.fp.mp, me.fp.store.state(), dRgb, dRgb + mine * 3u, reinterpret_cast<uint32_t*>(dRgb + mine * 9u), me.stream);
        HIP_CHECK(hipGetLastError());
        if (sendBandsToRoot(f.bands.slot(p), f.rootDevice, dRgb, me.device, f.bands.bandBytes(p), me.forceStaged, me.stream)) staged.fetch_add(1);
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.last.stagedParts = staged.load();
}

// ... and from there into image order (dCov and dCount nullable), on `stream` of the first device, which is joined
void interleave(PtrMultiFrame& f, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(f.rootDevice));
    f.bands.interleave(dRgb, dCov, dCount, stream);
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
    std::fprintf(stderr, "[multi-frame] partition %u %s: %zu bytes, %.4f ms\n", me.fp.mp.part, name,
                 static_cast<size_t>(me.fp.local) * kMultiStateWords * sizeof(float) * 2u, ms);
}

void exportState(PtrMultiFrame& f, float* sum, float* mean, float* m, uint32_t* n, float* e) {
    const AdaptiveState image{sum, mean, m, n, e};
    const bool timed = ptr::readKnobs().verboseLaunches;
    runParts(f, [&](Part& me, uint32_t, const auto&) {
        const size_t mine = multiBandPixels(me.fp.mp);
        if (!mine) return;
        me.packed.ensure(mine * kMultiStateWords);
        me.hostPacked.assign(mine * kMultiStateWords, 0.0f);
        timedStateKernel("k_multi_state_pack", me, timed, [&] { launchMultiStatePack(me.fp.mp, me.fp.store.state(), me.packed.ptr, me.stream); });
        HIP_CHECK(hipMemcpyAsync(me.hostPacked.data(), me.packed.ptr, mine * kMultiStateWords * sizeof(float), hipMemcpyDeviceToHost, me.stream));
        HIP_CHECK(hipStreamSynchronize(me.stream));
        // the partition's rows of the caller's image-order arrays (no two partitions share a row)
        for (uint32_t i = 0; i < mine; ++i) multiStateUnpack(me.fp.mp, i, me.hostPacked.data(), image);
    });
}

void importState(PtrMultiFrame& f, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e) {
    // (the pack body reads through the state's pointers only)
    const AdaptiveState image{const_cast<float*>(sum), const_cast<float*>(mean), const_cast<float*>(m), const_cast<uint32_t*>(n), const_cast<float*>(e)};
    const bool timed = ptr::readKnobs().verboseLaunches;
    runParts(f, [&](Part& me, uint32_t, const auto&) {
        const size_t mine = multiBandPixels(me.fp.mp);
        if (!mine) return;
        me.packed.ensure(mine * kMultiStateWords);
        me.hostPacked.assign(mine * kMultiStateWords, 0.0f);
        for (uint32_t i = 0; i < mine; ++i) multiStatePack(me.fp.mp, i, image, me.hostPacked.data());
        HIP_CHECK(hipMemcpyAsync(me.packed.ptr, me.hostPacked.data(), mine * kMultiStateWords * sizeof(float), hipMemcpyHostToDevice, me.stream));
        timedStateKernel("k_multi_state_unpack", me, timed, [&] { launchMultiStateUnpack(me.fp.mp, me.packed.ptr, me.fp.store.state(), me.stream); });
        if (f.parts > 1u) haloPublish(me.fp.mp, me.fp.store.e.ptr, me.edge.ptr, f.ex, me.stream);
        HIP_CHECK(hipStreamSynchronize(me.stream));
    });
    f.classes.rebuild(n, f.pixels);
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
        for (uint32_t p = 0; p < parts; ++p) {
            partBands[p] = ptr_part_band_count(f->height, p, parts);
            auto me = std::make_unique<Part>();
            me->device = devices[p];
            me->forceStaged = forceStaged[p] != 0;
            me->fp.mp = MultiPart{p, parts, partBands[p], f->width, f->height};
            f->part.push_back(std::move(me));
        }
        HIP_CHECK(hipSetDevice(f->rootDevice));
        f->bands.allocate(partBands, f->width, f->height, 3u, 9u, kOutWords);
        f->image.ensure(f->pixels * kOutWords);
        if (parts > 1u) f->ex.allocate(partBands, f->width);

        PtrMultiFrame& fr = *f;
        runParts(fr, [&](Part& me, uint32_t p, const auto&) {
            if (!sceneless) {
                me.scene = std::make_unique<PtrDeviceScene>();
                me.scene->device = me.device;
                uploadScene(*scene, prepared, *me.scene);
                me.fp.scene = me.scene.get();
                HIP_CHECK(hipSetDevice(me.device));
            }
            HIP_CHECK(hipStreamCreateWithFlags(&me.stream, hipStreamNonBlocking));
            std::vector<uint32_t> order;
            partitionPixels(fr.width, fr.height, p, parts, order);
            FramePart& fp = me.fp;
            fp.local = static_cast<uint32_t>(order.size());
            fp.store.ensure(fr.pixels);   // image order: the lists name image pixels, select reads e around them
            fp.order.upload(order.data(), order.size());
            fp.listS.ensure(fp.local);
            fp.inS.ensure(fp.local);
            me.edge.ensure(static_cast<size_t>(fp.mp.bands) * 2u * fr.width);
            if (sceneless) fp.probeSamples.upload(reinterpret_cast<const float4*>(samples), fr.pixels * sampleCount);
            fp.store.zero(me.stream);
            HIP_CHECK(hipStreamSynchronize(me.stream));
        });
        f->classes.reset(f->pixels);
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
    const std::string bad = badReset(who, frame->width, frame->height, settings);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
    const std::string bad = badAccumulate(who, frame->classes, spp, frame->sampleCount);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
    std::string bad = badAdaptiveParams(who, *params);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (const int rc = refuseBroken(who, frame, err, err_cap)) return rc;
    bad = badRefine(who, frame->classes, *params, frame->sampleCount);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
            downloadFirstHit(*f.part[0]->scene, f.settings, 0u, f.albedo, f.normal, out_albedo, out_normal);
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
    frame->classes.fill(*out);
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
