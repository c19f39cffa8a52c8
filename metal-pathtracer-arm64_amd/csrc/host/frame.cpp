// Host side of include/ptr_frame.h: the frame object (the per-pixel state of an adaptive frame, owned by the frame and kept on the device
// between calls), the argument checks, accumulate, the loop of refine (class minimum -> split -> an ordinary pass of the wavefront kernels
// over S -> update -> select on S and merge), resolve, the checkpoint, and the test-only frame whose accumulators are gathered from
// given samples instead of being traced.  The state's buffers, the sample sources and the sample step are the ones adaptive.cpp and
// multi.cpp use (adaptive_host.h); the frame's own are the first list, S, and the count classes it keeps on the host.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/frame.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "knobs.h"
#include "ptr_frame.h"

using namespace ptrhost;
using namespace ptrk;

struct PtrFrame {
    PtrDeviceScene* scene = nullptr;   // null: the test-only frame
    int device = 0;
    PtrSettings settings{};
    size_t pixels = 0;
    AdaptiveStore store;   // the state, image order; L's two buffers; the compaction's scratch and the word the class minimum arrives in
    DeviceBuffer<uint32_t> order, listS;   // the first list; S
    DeviceBuffer<uint8_t> inS;             // the flag "in S" per entry of L
    DeviceBuffer<float> out;   // ptr_frame_resolve: rgb, cov and count before they go to the host
    // the test-only frame: the samples it was given, and the accumulators of a pass gathered from them
    DeviceBuffer<float4> probeSamples, probeItems;
    uint32_t sampleCount = 0;
    // pixels per count n_p, kept on the host: a round moves |S| pixels from n_min to n_min + k, so the checks and ptr_frame_info need
    // no device call
    std::map<uint32_t, uint64_t> classes;

    bool uniform() const { return classes.size() == 1u; }
    uint32_t minCount() const { return classes.begin()->first; }
    uint32_t maxCount() const { return classes.rbegin()->first; }
};

namespace {

// what the sample steps of one call on the frame share; `sum` (nullable) collects the stats
SampleStep sampleStep(PtrFrame& f, hipStream_t stream, PtrRenderStats* sum) {
    return SampleStep{f.scene ? tracedSource(*f.scene, f.settings, stream) : gatheredSource(f.probeSamples.ptr, f.pixels, f.sampleCount, f.probeItems, stream),
                      maxPassItems(f.scene), f.store.state(), stream, sum};
}

void zeroState(PtrFrame& f, hipStream_t stream) {
    f.store.zero(stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    f.classes.clear();
    f.classes[0u] = f.pixels;
}

// the buffers of a new frame and its empty state; `device` is current
void allocate(PtrFrame& f) {
    f.store.ensure(f.pixels);
    f.listS.ensure(f.pixels);
    f.inS.ensure(f.pixels);
    std::vector<uint32_t> order;
    imagePixelOrder(f.settings.width, f.settings.height, order);
    f.order.upload(order.data(), f.pixels);
    zeroState(f, nullptr);
}

// The samples of one class: `list` (count entries, all at nBefore samples) gets spp more, and its pixels move to the new count.
void addClassSamples(PtrFrame& f, const SampleStep& step, const uint32_t* list, uint32_t count, uint32_t nBefore, uint32_t spp) {
    addSamples(step, list, count, nBefore, spp);
    auto it = f.classes.find(nBefore);
    if (it != f.classes.end()) {   // (always, unless an import brought counts that disagree with themselves)
        it->second -= std::min<uint64_t>(it->second, count);
        if (it->second == 0u) f.classes.erase(it);
    }
    f.classes[nBefore + spp] += count;
}

void accumulate(PtrFrame& f, uint32_t spp, hipStream_t stream, PtrRenderStats* stats) {
    HIP_CHECK(hipSetDevice(f.device));
    PtrRenderStats sum{};
    addClassSamples(f, sampleStep(f, stream, stats ? &sum : nullptr), f.order.ptr, static_cast<uint32_t>(f.pixels), f.minCount(), spp);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        sum.samples = static_cast<uint64_t>(f.pixels) * spp;
        sum.avgMsPerSample = sum.totalSeconds * 1000.0 / spp;
        *stats = sum;
    }
}

void refine(PtrFrame& f, const PtrAdaptiveParams& params, hipStream_t stream, PtrRenderStats* stats, PtrAdaptiveInfo* info) {
    HIP_CHECK(hipSetDevice(f.device));
    const uint32_t width = f.settings.width, height = f.settings.height, pixels = static_cast<uint32_t>(f.pixels);
    const AdaptiveScratch scratch = f.store.scratch();
    PtrAdaptiveInfo local{};
    PtrRenderStats sum{};
    const SampleStep step = sampleStep(f, stream, stats ? &sum : nullptr);
    const AdaptiveState& st = step.state;
    auto note = [&](uint32_t active) {
        if (local.rounds < PTR_ADAPTIVE_INFO_ROUNDS) local.activeAfter[local.rounds] = active;
        ++local.rounds;
    };
    // the length of the list a select or a merge just wrote, and (with `min`) the class minimum beside it
    auto readWords = [&](uint32_t* total, uint32_t* min) {
        uint32_t words[2] = {0u, 0u};
        HIP_CHECK(hipMemcpyAsync(words, scratch.total, (min ? 2u : 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        *total = words[0];
        if (min) *min = words[1];
    };

    const bool empty = f.uniform() && f.minCount() == 0u;
    uint32_t deepest = 0u;   // the most samples this call gave one pixel
    if (empty) {
        addClassSamples(f, step, f.order.ptr, pixels, 0u, params.minSpp);
        local.totalSamples += static_cast<uint64_t>(pixels) * params.minSpp;
        deepest = params.minSpp;
    }
    // the start list, and with it the class minimum of the first round
    uint32_t turn = 0u, active = 0u, nMin = kFrameNoCount;
    launchAdaptiveSelect(f.order.ptr, pixels, width, height, st, params.maxSpp, params.threshold, scratch, f.store.list(0u), stream);
    HIP_CHECK(hipGetLastError());
    readWords(&active, nullptr);
    if (empty) note(active);

    // PTR_VERBOSE=launches: device events around the kernels between the rounds (tools/frame_cost.py parses the line)
    EventSet marks;
    const bool timed = ptr::readKnobs().verboseLaunches;
    if (timed) marks.create(4u);
    while (active > 0u) {
        const uint32_t* list = f.store.list(turn);
        // n_min, then S
        if (timed) HIP_CHECK(hipEventRecord(marks[0], stream));
        HIP_CHECK(hipMemsetAsync(f.store.minWord(), 0xFF, sizeof(uint32_t), stream));   // kFrameNoCount
        launchFrameClassMin(list, active, st.n, f.store.minWord(), stream);
        HIP_CHECK(hipGetLastError());
        uint32_t ignored = 0u, inClass = 0u;
        readWords(&ignored, &nMin);
        if (nMin >= params.maxSpp) throw HipError{"ptr_frame_refine: the active list holds a pixel at maxSpp"};   // (select never keeps one)
        launchFrameSplit(list, active, st.n, nMin, f.inS.ptr, scratch, f.listS.ptr, stream);
        if (timed) HIP_CHECK(hipEventRecord(marks[1], stream));
        HIP_CHECK(hipGetLastError());
        readWords(&inClass, nullptr);
        if (inClass == 0u || inClass > active) throw HipError{"ptr_frame_refine: the class of the round is empty"};
        // its samples
        const uint32_t k = std::min(params.stepSpp, params.maxSpp - nMin);
        addClassSamples(f, step, f.listS.ptr, inClass, nMin, k);
        local.totalSamples += static_cast<uint64_t>(inClass) * k;
        deepest = std::max(deepest, k);
        // select on S, merged into the next L
        if (timed) HIP_CHECK(hipEventRecord(marks[2], stream));
        launchFrameMerge(list, active, f.inS.ptr, width, height, st, params.maxSpp, params.threshold, scratch, f.store.list(turn ^ 1u), stream);
        if (timed) HIP_CHECK(hipEventRecord(marks[3], stream));
        HIP_CHECK(hipGetLastError());
        const uint32_t before = active;
        readWords(&active, nullptr);
        if (timed) {   // debugging aid, like the [adaptive] lines of ptr_render_adaptive
            float splitMs = 0.0f, mergeMs = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&splitMs, marks[0], marks[1]));
            HIP_CHECK(hipEventElapsedTime(&mergeMs, marks[2], marks[3]));
            std::fprintf(stderr, "[frame] round %u: class %u, %u of %u active x %u spp; minimum + split %.4f ms, select + merge %.4f ms\n", local.rounds,
                         nMin, inClass, before, k, splitMs, mergeMs);
        }
        note(active);
        turn ^= 1u;
    }
    const auto atMax = f.classes.find(params.maxSpp);
    local.pixelsAtMax = atMax == f.classes.end() ? 0u : static_cast<uint32_t>(atMax->second);
    if (stats) {
        sum.samples = local.totalSamples;
        sum.avgMsPerSample = sum.totalSeconds * 1000.0 / std::max(1u, deepest);
        *stats = sum;
    }
    if (info) *info = local;
}

void resolveDevice(PtrFrame& f, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(f.device));
    launchAdaptiveFinish(f.store.state(), static_cast<uint32_t>(f.pixels), dRgb, dCov, dCount, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
}

std::string badSize(const std::string& w, uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u) return w + ": render size must be non-zero";
    if (pastIndexLimit(static_cast<uint64_t>(width) * height)) return w + ": image too large for a frame";
    return std::string();
}

}  // namespace

extern "C" {

int ptr_frame_create(PtrDeviceScene* scene, const PtrSettings* settings, PtrFrame** out_frame, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_create";
    if (!scene || !settings || !out_frame) return nullArgument(who, err, err_cap);
    const std::string bad = badSize(who, settings->width, settings->height);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (ptr_device_count() < 1) return noDevice(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(scene->device));
        auto f = std::make_unique<PtrFrame>();
        f->scene = scene;
        f->device = scene->device;
        f->settings = *settings;
        f->pixels = static_cast<size_t>(settings->width) * settings->height;
        allocate(*f);
        *out_frame = f.release();
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

void ptr_frame_release(PtrFrame* frame) {
    if (!frame) return;
    (void)hipSetDevice(frame->device);
    delete frame;
}

int ptr_frame_debug_create(uint32_t width, uint32_t height, const float* samples, uint32_t sample_count, int device, PtrFrame** out_frame,
                           char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_debug_create";
    if (!samples || !out_frame) return nullArgument(who, err, err_cap);
    const std::string bad = badSize(who, width, height);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (sample_count == 0u) return refuse(err, err_cap, std::string(who) + ": sample_count must be >= 1");
    const int available = ptr_device_count();
    if (available < 1) return noDevice(who, err, err_cap);
    if (device < 0 || device >= available) return refuse(err, err_cap, std::string(who) + ": no such HIP device");
    try {
        HIP_CHECK(hipSetDevice(device));
        auto f = std::make_unique<PtrFrame>();
        f->device = device;
        f->settings.width = width;
        f->settings.height = height;
        f->pixels = static_cast<size_t>(width) * height;
        f->sampleCount = sample_count;
        f->probeSamples.upload(reinterpret_cast<const float4*>(samples), f->pixels * sample_count);
        allocate(*f);
        *out_frame = f.release();
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_reset(PtrFrame* frame, const PtrSettings* settings, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_reset";
    if (!frame) return nullArgument(who, err, err_cap);
    if (settings && (settings->width != frame->settings.width || settings->height != frame->settings.height)) {
        return refuse(err, err_cap, std::string(who) + ": a frame keeps its width and height for its life");
    }
    try {
        HIP_CHECK(hipSetDevice(frame->device));
        if (settings) frame->settings = *settings;
        zeroState(*frame, nullptr);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_accumulate(PtrFrame* frame, uint32_t spp, void* stream, PtrRenderStats* stats, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_accumulate";
    if (!frame) return nullArgument(who, err, err_cap);
    if (spp == 0u) return refuse(err, err_cap, std::string(who) + ": spp must be >= 1");
    if (!frame->uniform()) {
        return refuse(err, err_cap, std::string(who) + ": the frame is not uniform (its pixels hold different sample counts); a refine with threshold 0 "
                                                       "brings every pixel with a non-zero error up to a common count");
    }
    if (static_cast<uint64_t>(frame->minCount()) + spp > 0xFFFFFFF0ull) return refuse(err, err_cap, std::string(who) + ": too many samples");
    if (!frame->scene && static_cast<uint64_t>(frame->minCount()) + spp > frame->sampleCount) {
        return refuse(err, err_cap, std::string(who) + ": a sample past the ones the frame was given");
    }
    try {
        accumulate(*frame, spp, static_cast<hipStream_t>(stream), stats);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_refine(PtrFrame* frame, const PtrAdaptiveParams* params, void* stream, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                     size_t err_cap) {
    static const char* const who = "ptr_frame_refine";
    if (!frame || !params) return nullArgument(who, err, err_cap);
    const std::string bad = badAdaptiveParams(who, *params);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    const bool empty = frame->uniform() && frame->minCount() == 0u;
    if (!empty && frame->minCount() < 2u) {
        return refuse(err, err_cap, std::string(who) + ": every pixel of a frame that is not empty must hold at least 2 samples");
    }
    if (!frame->scene && params->maxSpp > frame->sampleCount) return refuse(err, err_cap, std::string(who) + ": a sample past the ones the frame was given");
    try {
        refine(*frame, *params, static_cast<hipStream_t>(stream), stats, info);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_resolve_device(PtrFrame* frame, void* d_out_rgb, void* d_out_cov, void* d_out_count, void* stream, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_resolve_device";
    if (!frame || !d_out_rgb) return nullArgument(who, err, err_cap);
    try {
        resolveDevice(*frame, static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_cov), static_cast<uint32_t*>(d_out_count),
                      static_cast<hipStream_t>(stream));
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_resolve(PtrFrame* frame, float* out_rgb, float* out_cov, uint32_t* out_count, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_resolve";
    if (!frame || !out_rgb) return nullArgument(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(frame->device));
        finishAndDownload(frame->out, frame->pixels, out_rgb, out_cov, out_count,
                          [&](float* dRgb, float* dCov, uint32_t* dCount) { resolveDevice(*frame, dRgb, dCov, dCount, nullptr); });
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_info(const PtrFrame* frame, PtrFrameInfo* out) {
    if (!frame || !out) return 1;
    *out = PtrFrameInfo{};
    out->width = frame->settings.width;
    out->height = frame->settings.height;
    out->minCount = frame->minCount();
    out->maxCount = frame->maxCount();
    for (const auto& c : frame->classes) out->totalSamples += static_cast<uint64_t>(c.first) * c.second;
    out->uniform = frame->uniform() ? 1u : 0u;
    return 0;
}

int ptr_frame_export(PtrFrame* frame, float* sum, float* mean, float* m, uint32_t* n, float* e, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_export";
    if (!frame || !sum || !mean || !m || !n || !e) return nullArgument(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(frame->device));
        frame->store.download(sum, mean, m, n, e);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_import(PtrFrame* frame, const float* sum, const float* mean, const float* m, const uint32_t* n, const float* e, char* err,
                     size_t err_cap) {
    static const char* const who = "ptr_frame_import";
    if (!frame || !sum || !mean || !m || !n || !e) return nullArgument(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(frame->device));
        frame->store.upload(sum, mean, m, n, e);
        frame->classes.clear();
        for (size_t p = 0; p < frame->pixels; ++p) ++frame->classes[n[p]];
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
