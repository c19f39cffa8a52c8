// Host side of include/ptr_frame.h: the frame object (the per-pixel state of an adaptive frame, owned by the frame and kept on the device
// between calls), the argument checks, accumulate, refine, resolve, the checkpoint, and the test-only frame, whose samples are given.
// A frame is the one-partition case of the frame on several devices: on the device it keeps one FramePart, and refine is the round loop
// of frame_rounds.h on the calling thread and the caller's stream, with no thread, no barrier and no exchange.  The count classes and
// their refusals are frame_classes.h's; the state's buffers, the sample sources and the sample step adaptive_host.h's.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "adaptive_host.h"
#include "device_scene.h"
#include "frame_classes.h"
#include "frame_rounds.h"
#include "knobs.h"
#include "ptr_frame.h"

using namespace ptrhost;
using namespace ptrk;

struct PtrFrame {
    int device = 0;
    PtrSettings settings{};
    size_t pixels = 0;
    FramePart part;            // the whole image
    DeviceBuffer<float> out;   // ptr_frame_resolve: rgb, cov and count before they go to the host
    uint32_t sampleCount = 0;  // the test-only frame: the samples it was given; 0 with a scene
    CountClasses classes;
};

namespace {

void zeroState(PtrFrame& f, hipStream_t stream) {
    f.part.store.zero(stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    f.classes.reset(f.pixels);
}

// the buffers of a new frame and its empty state; `device` is current
void allocate(PtrFrame& f) {
    FramePart& me = f.part;
    me.mp = MultiPart{0u, 1u, ptr_part_band_count(f.settings.height, 0u, 1u), f.settings.width, f.settings.height};
    me.local = static_cast<uint32_t>(f.pixels);
    me.store.ensure(f.pixels);
    me.listS.ensure(f.pixels);
    me.inS.ensure(f.pixels);
    std::vector<uint32_t> order;
    imagePixelOrder(f.settings.width, f.settings.height, order);
    me.order.upload(order.data(), f.pixels);
    zeroState(f, nullptr);
}

void accumulate(PtrFrame& f, uint32_t spp, hipStream_t stream, PtrRenderStats* stats) {
    HIP_CHECK(hipSetDevice(f.device));
    PtrRenderStats sum{};
    const uint32_t n = f.classes.minCount();
    addSamples(sampleStep(f.part, f.settings, f.sampleCount, stream, stats ? &sum : nullptr), f.part.order.ptr, f.part.local, n, spp);
    f.classes.move(n, n + spp, f.pixels);
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
    PtrRenderStats sum{};
    RefineCall call("ptr_frame_refine", params, 1u, f.classes.empty(), nullptr);
    // PTR_VERBOSE=launches: device events around the kernels between the rounds (tools/frame_cost.py parses the line)
    EventSet marks;
    if (ptr::readKnobs().verboseLaunches) marks.create(kRoundMarks);
    auto report = [&](const RoundReport& r) {   // debugging aid, like the [adaptive] lines of ptr_render_adaptive
        if (!marks[0]) return;
        float minMs = 0.0f, splitMs = 0.0f, mergeMs = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&minMs, marks[kMarkMinimum], marks[kMarkMinimum + 1]));
        HIP_CHECK(hipEventElapsedTime(&splitMs, marks[kMarkSplit], marks[kMarkSplit + 1]));
        HIP_CHECK(hipEventElapsedTime(&mergeMs, marks[kMarkMerge], marks[kMarkMerge + 1]));
        std::fprintf(stderr, "[frame] round %u: class %u, %u of %u active x %u spp; minimum + split %.4f ms, select + merge %.4f ms\n",
                     r.round + (call.empty ? 1u : 0u), r.nMin, r.inClass, r.activeBefore, r.spp, minMs + splitMs, mergeMs);
    };
    const SampleStep step = sampleStep(f.part, f.settings, f.sampleCount, stream, stats ? &sum : nullptr);
    refinePartition(call, 0u, f.part, nullptr, step, [] { return true; }, marks, report);
    for (const ClassMove& mv : call.moves) f.classes.move(mv.from, mv.to, mv.pixels);
    call.info.pixelsAtMax = static_cast<uint32_t>(f.classes.pixelsAt(params.maxSpp));
    if (stats) {
        sum.samples = call.info.totalSamples;
        sum.avgMsPerSample = sum.totalSeconds * 1000.0 / std::max(1u, call.deepest);
        *stats = sum;
    }
    if (info) *info = call.info;
}

void resolveDevice(PtrFrame& f, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(f.device));
    launchAdaptiveFinish(f.part.store.state(), static_cast<uint32_t>(f.pixels), dRgb, dCov, dCount, stream);
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
        f->part.scene = scene;
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
        f->part.probeSamples.upload(reinterpret_cast<const float4*>(samples), f->pixels * sample_count);
        allocate(*f);
        *out_frame = f.release();
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_frame_reset(PtrFrame* frame, const PtrSettings* settings, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_reset";
    if (!frame) return nullArgument(who, err, err_cap);
    const std::string bad = badReset(who, frame->settings.width, frame->settings.height, settings);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
    const std::string bad = badAccumulate(who, frame->classes, spp, frame->sampleCount);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
    std::string bad = badAdaptiveParams(who, *params);
    if (bad.empty()) bad = badRefine(who, frame->classes, *params, frame->sampleCount);
    if (!bad.empty()) return refuse(err, err_cap, bad);
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
    frame->classes.fill(*out);
    return 0;
}

int ptr_frame_export(PtrFrame* frame, float* sum, float* mean, float* m, uint32_t* n, float* e, char* err, size_t err_cap) {
    static const char* const who = "ptr_frame_export";
    if (!frame || !sum || !mean || !m || !n || !e) return nullArgument(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(frame->device));
        frame->part.store.download(sum, mean, m, n, e);
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
        frame->part.store.upload(sum, mean, m, n, e);
        frame->classes.rebuild(n, frame->pixels);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
