// Host side of include/ptr_adaptive.h: the argument checks, the loop over the rounds of an adaptive frame (every round an ordinary pass
// of the wavefront kernels over the active list, then update -> select -> compact), and the test-only probe of one round.  Also what
// adaptive_host.h and adaptive_state.h declare for all three round loops (this one, multi.cpp's and the resumable frames' in
// frame_rounds.cpp): the owner of the per-pixel state, the sample sources, the sample step and the finish into staging.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../kernels/adaptive.h"
#include "../kernels/multi.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "knobs.h"
#include "ptr_adaptive.h"

using namespace ptrhost;
using namespace ptrk;

namespace ptrhost {

std::string badAdaptiveParams(const char* who, const PtrAdaptiveParams& p) {
    const std::string w(who);
    if (p.minSpp < 2u) return w + ": minSpp must be >= 2 (a sample covariance needs two samples)";
    if (p.maxSpp < p.minSpp) return w + ": maxSpp must be >= minSpp";
    if (p.stepSpp < 1u) return w + ": stepSpp must be >= 1";
    if (!(std::isfinite(p.threshold) && p.threshold >= 0.0f)) return w + ": threshold must be finite and >= 0";
    return std::string();
}

void AdaptiveStore::ensure(size_t pixelCount) {
    pixels = pixelCount;
    sum.ensure(pixels * 3u);
    mean.ensure(pixels * 3u);
    m.ensure(pixels * 6u);
    n.ensure(pixels);
    e.ensure(pixels);
    lists.ensure(pixels * 2u);
    blockWords.ensure(blocks() * 2u + 2u);
    keep.ensure(pixels);
}

void AdaptiveStore::zero(hipStream_t stream) const {
    HIP_CHECK(hipMemsetAsync(sum.ptr, 0, pixels * 3u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(mean.ptr, 0, pixels * 3u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(m.ptr, 0, pixels * 6u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(n.ptr, 0, pixels * sizeof(uint32_t), stream));
    HIP_CHECK(hipMemsetAsync(e.ptr, 0, pixels * sizeof(float), stream));
}

void AdaptiveStore::upload(const float* hSum, const float* hMean, const float* hM, const uint32_t* hN, const float* hE) {
    sum.upload(hSum, pixels * 3u);
    mean.upload(hMean, pixels * 3u);
    m.upload(hM, pixels * 6u);
    n.upload(hN, pixels);
    e.upload(hE, pixels);
}

void AdaptiveStore::download(float* hSum, float* hMean, float* hM, uint32_t* hN, float* hE) const {
    sum.download(hSum, pixels * 3u);
    mean.download(hMean, pixels * 3u);
    m.download(hM, pixels * 6u);
    n.download(hN, pixels);
    e.download(hE, pixels);
}

PassSource tracedSource(PtrDeviceScene& scene, const PtrSettings& settings, hipStream_t stream) {
    return [&scene, &settings, stream](uint32_t spp, uint32_t sampleBase, const uint32_t* dList, uint32_t active, PtrRenderStats* one,
                                       const std::function<void(const float4*)>& consume) {
        traceItems(scene, settings, spp, sampleBase, dList, active, stream, one, consume);
    };
}

PassSource gatheredSource(const float4* dSamples, size_t pixels, uint32_t sampleCount, DeviceBuffer<float4>& items, hipStream_t stream) {
    return [dSamples, pixels, sampleCount, &items, stream](uint32_t spp, uint32_t sampleBase, const uint32_t* dList, uint32_t active, PtrRenderStats*,
                                                           const std::function<void(const float4*)>& consume) {
        if (static_cast<uint64_t>(sampleBase) + spp > sampleCount) throw HipError{"a sample past the ones the frame was given"};
        items.ensure(static_cast<size_t>(active) * spp);
        launchMultiGatherItems(dSamples, pixels, dList, active, spp, sampleBase, items.ptr, stream);
        consume(items.ptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
    };
}

void addSamples(const SampleStep& step, const uint32_t* list, uint32_t count, uint32_t nBefore, uint32_t spp, const SubPassHook& inPass,
                const SubPassHook& afterPass) {
    forEachSubPass(step.maxItems, count, spp, [&](uint32_t done, uint32_t part, bool last) {
        PtrRenderStats one{};
        step.source(part, nBefore + done, list, count, step.sum ? &one : nullptr, [&](const float4* items) {
            if (step.beforeUpdate) HIP_CHECK(hipEventRecord(step.beforeUpdate, step.stream));
            launchAdaptiveUpdate(items, list, count, part, nBefore + done, last, step.state, step.stream);
            if (step.afterUpdate) HIP_CHECK(hipEventRecord(step.afterUpdate, step.stream));
            if (inPass) inPass(done, part, last);
        });
        if (step.sum) addPassStats(one, *step.sum);
        if (afterPass) afterPass(done, part, last);
    });
}

void finishAndDownload(DeviceBuffer<float>& staging, size_t pixels, float* outRgb, float* outCov, uint32_t* outCount,
                       const std::function<void(float* dRgb, float* dCov, uint32_t* dCount)>& finish) {
    staging.ensure(pixels * 10u);
    float* dRgb = staging.ptr;
    float* dCov = outCov ? dRgb + pixels * 3u : nullptr;
    uint32_t* dCount = outCount ? reinterpret_cast<uint32_t*>(dRgb + pixels * 9u) : nullptr;
    finish(dRgb, dCov, dCount);
    HIP_CHECK(hipMemcpy(outRgb, dRgb, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (outCov) HIP_CHECK(hipMemcpy(outCov, dCov, pixels * 6u * sizeof(float), hipMemcpyDeviceToHost));
    if (outCount) HIP_CHECK(hipMemcpy(outCount, dCount, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

}  // namespace ptrhost

namespace {

std::string badRender(const char* who, bool pointersOk, const PtrSettings* settings, const PtrAdaptiveParams* params) {
    const std::string w(who);
    if (!pointersOk) return w + ": null argument";
    if (settings->width == 0u || settings->height == 0u) return w + ": render size must be non-zero";
    return badAdaptiveParams(who, *params);
}

void renderAdaptive(PtrDeviceScene& ds, const PtrSettings& settings, const PtrAdaptiveParams& params, float* dRgb, float* dCov, uint32_t* dCount,
                    hipStream_t stream, PtrRenderStats* stats, PtrAdaptiveInfo* info) {
    HIP_CHECK(hipSetDevice(ds.device));
    const size_t pixels = static_cast<size_t>(settings.width) * settings.height;
    if (pastIndexLimit(pixels)) throw HipError{"image too large for an adaptive frame"};
    AdaptiveStore& b = ds.adaptive;
    b.ensure(pixels);
    std::vector<uint32_t> order;
    imagePixelOrder(settings.width, settings.height, order);
    HIP_CHECK(hipMemcpyAsync(b.list(0u), order.data(), pixels * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    b.zero(stream);
    HIP_CHECK(hipStreamSynchronize(stream));   // `order` is pageable host memory

    PtrAdaptiveInfo local{};
    PtrRenderStats sum{};
    uint32_t active = static_cast<uint32_t>(pixels), n = 0u, turn = 0u;
    // PTR_VERBOSE=launches: device events around the kernels between the rounds
    EventSet marks;
    const bool timed = ptr::readKnobs().verboseLaunches;
    if (timed) marks.create(3u);
    const SampleStep step{tracedSource(ds, settings, stream), maxPassItems(&ds), b.state(), stream, stats ? &sum : nullptr, marks[0], marks[1]};
    const AdaptiveScratch scratch = b.scratch();
    while (active > 0u && n < params.maxSpp) {
        const uint32_t roundSpp = adaptiveRoundSpp(params, n);
        const uint32_t* list = b.list(turn);
        addSamples(
            step, list, active, n, roundSpp,
            [&](uint32_t, uint32_t, bool last) {
                if (last) launchAdaptiveSelect(list, active, settings.width, settings.height, step.state, params.maxSpp, params.threshold, scratch, b.list(turn ^ 1u), stream);
                if (timed) HIP_CHECK(hipEventRecord(marks[2], stream));
            },
            [&](uint32_t done, uint32_t spp, bool last) {
                if (!timed) return;   // debugging aid, like the [launch] lines of a pass (tools/adaptive_cost.py parses it)
                float updateMs = 0.0f, selectMs = 0.0f;
                HIP_CHECK(hipEventElapsedTime(&updateMs, marks[0], marks[1]));
                HIP_CHECK(hipEventElapsedTime(&selectMs, marks[1], marks[2]));
                std::fprintf(stderr, "[adaptive] round %u first sample %u: %u active x %u spp; update %.4f ms, select + compact %.4f ms\n", local.rounds,
                             n + done, active, spp, updateMs, last ? selectMs : 0.0f);
            });
        n += roundSpp;
        local.totalSamples += static_cast<uint64_t>(active) * roundSpp;
        if (n >= params.maxSpp) local.pixelsAtMax = active;
        HIP_CHECK(hipMemcpy(&active, scratch.total, sizeof(uint32_t), hipMemcpyDeviceToHost));   // (traceItems joined the stream)
        if (local.rounds < PTR_ADAPTIVE_INFO_ROUNDS) local.activeAfter[local.rounds] = active;
        ++local.rounds;
        turn ^= 1u;
    }
    launchAdaptiveFinish(step.state, static_cast<uint32_t>(pixels), dRgb, dCov, dCount, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        sum.samples = local.totalSamples;
        sum.avgMsPerSample = sum.totalSeconds * 1000.0 / std::max(1u, n);
        *stats = sum;
    }
    if (info) *info = local;
}

}  // namespace

extern "C" {

void ptr_adaptive_default_params(PtrAdaptiveParams* out, uint32_t max_spp) {
    if (!out) return;
    out->minSpp = 8u;
    out->stepSpp = 8u;
    out->threshold = 0.05f;
    out->maxSpp = std::max(max_spp, out->minSpp);
}

int ptr_render_adaptive_device(PtrDeviceScene* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, void* d_out_rgb,
                               void* d_out_cov, void* d_out_count, void* stream, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err,
                               size_t err_cap) {
    static const char* const who = "ptr_render_adaptive_device";
    const std::string bad = badRender(who, scene && settings && params && d_out_rgb, settings, params);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (ptr_device_count() < 1) return noDevice(who, err, err_cap);
    try {
        renderAdaptive(*scene, *settings, *params, static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_cov), static_cast<uint32_t*>(d_out_count),
                       static_cast<hipStream_t>(stream), stats, info);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_render_adaptive(PtrDeviceScene* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, float* out_rgb,
                        float* out_cov, uint32_t* out_count, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err, size_t err_cap) {
    static const char* const who = "ptr_render_adaptive";
    const std::string bad = badRender(who, scene && settings && params && out_rgb, settings, params);
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (ptr_device_count() < 1) return noDevice(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(scene->device));
        finishAndDownload(scene->adaptiveOut, static_cast<size_t>(settings->width) * settings->height, out_rgb, out_cov, out_count,
                          [&](float* dRgb, float* dCov, uint32_t* dCount) { renderAdaptive(*scene, *settings, *params, dRgb, dCov, dCount, nullptr, stats, info); });
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_adaptive_debug_round(uint32_t width, uint32_t height, const PtrAdaptiveParams* params, uint32_t n_before, uint32_t round_spp,
                             int last_sub_pass, const uint32_t* list, uint32_t active_count, const float* samples, float* sum, float* mean,
                             float* m, uint32_t* n, float* e, uint32_t* out_next, uint32_t* out_next_count, char* err, size_t err_cap) {
    static const char* const who = "ptr_adaptive_debug_round";
    const bool pointersOk = params && list && samples && sum && mean && m && n && e && out_next && out_next_count;
    std::string bad;
    if (!pointersOk) {
        bad = std::string(who) + ": null argument";
    } else if (width == 0u || height == 0u || pastIndexLimit(static_cast<uint64_t>(width) * height)) {
        bad = std::string(who) + ": image size must be non-zero";
    } else if ((bad = badAdaptiveParams(who, *params)).empty()) {
        const uint64_t pixels = static_cast<uint64_t>(width) * height;
        if (active_count == 0u || active_count > pixels || round_spp == 0u) bad = std::string(who) + ": the list and the round must not be empty";
        else if (static_cast<uint64_t>(n_before) + round_spp > params->maxSpp) bad = std::string(who) + ": the round goes past maxSpp";
        else if (pastIndexLimit(static_cast<uint64_t>(active_count) * round_spp)) bad = std::string(who) + ": too many samples";
        for (uint32_t j = 0; bad.empty() && j < active_count; ++j) {
            if (list[j] >= pixels) bad = std::string(who) + ": the list names a pixel outside the image";
        }
    }
    if (!bad.empty()) return refuse(err, err_cap, bad);
    if (ptr_device_count() < 1) return noDevice(who, err, err_cap);
    try {
        HIP_CHECK(hipSetDevice(0));
        // the buffers are sized by the image, not by the list: the kernels take keep flags and block words for active_count entries at least
        AdaptiveStore b;
        DeviceBuffer<float4> dItems;
        b.ensure(static_cast<size_t>(width) * height);
        b.upload(sum, mean, m, n, e);
        const size_t listBytes = static_cast<size_t>(active_count) * sizeof(uint32_t);
        HIP_CHECK(hipMemcpy(b.list(0u), list, listBytes, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(b.list(1u), out_next, listBytes, hipMemcpyHostToDevice));   // (entries past the next count come back as they were)
        dItems.upload(reinterpret_cast<const float4*>(samples), static_cast<size_t>(active_count) * round_spp);
        launchAdaptiveUpdate(dItems.ptr, b.list(0u), active_count, round_spp, n_before, last_sub_pass != 0, b.state(), nullptr);
        uint32_t nextCount = active_count;
        if (last_sub_pass) {
            launchAdaptiveSelect(b.list(0u), active_count, width, height, b.state(), params->maxSpp, params->threshold, b.scratch(), b.list(1u), nullptr);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (last_sub_pass) {
            HIP_CHECK(hipMemcpy(&nextCount, b.scratch().total, sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out_next, b.list(1u), listBytes, hipMemcpyDeviceToHost));
        } else {
            std::memcpy(out_next, list, listBytes);
        }
        b.download(sum, mean, m, n, e);
        *out_next_count = nextCount;
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
