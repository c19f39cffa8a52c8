// Host side of include/ptr_adaptive.h: the argument checks, the loop over the rounds of an adaptive frame (every round an ordinary pass
// of the wavefront kernels over the active list, then update -> select -> compact), and the test-only probe of one round.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../kernels/adaptive.h"
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

AdaptiveBuffers ensureAdaptiveBuffers(PtrDeviceScene& ds, size_t pixels) {
    ds.adaptiveSum.ensure(pixels * 3u);
    ds.adaptiveMean.ensure(pixels * 3u);
    ds.adaptiveM.ensure(pixels * 6u);
    ds.adaptiveN.ensure(pixels);
    ds.adaptiveE.ensure(pixels);
    ds.adaptiveLists.ensure(pixels * 2u);
    const size_t blocks = (pixels + kAdaptiveBlock - 1u) / kAdaptiveBlock;
    ds.adaptiveBlockWords.ensure(blocks * 2u + 1u);
    ds.adaptiveKeep.ensure(pixels);
    AdaptiveBuffers b;
    b.state = AdaptiveState{ds.adaptiveSum.ptr, ds.adaptiveMean.ptr, ds.adaptiveM.ptr, ds.adaptiveN.ptr, ds.adaptiveE.ptr};
    b.lists[0] = ds.adaptiveLists.ptr;
    b.lists[1] = ds.adaptiveLists.ptr + pixels;
    b.scratch = AdaptiveScratch{ds.adaptiveKeep.ptr, ds.adaptiveBlockWords.ptr, ds.adaptiveBlockWords.ptr + blocks, ds.adaptiveBlockWords.ptr + 2u * blocks};
    return b;
}

void zeroAdaptiveState(const AdaptiveBuffers& b, size_t pixels, hipStream_t stream) {
    HIP_CHECK(hipMemsetAsync(b.state.sum, 0, pixels * 3u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(b.state.mean, 0, pixels * 3u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(b.state.m, 0, pixels * 6u * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(b.state.n, 0, pixels * sizeof(uint32_t), stream));
    HIP_CHECK(hipMemsetAsync(b.state.e, 0, pixels * sizeof(float), stream));
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
    if (pixels > 0xFFFF0000ull) throw HipError{"image too large for an adaptive frame"};
    const AdaptiveBuffers b = ensureAdaptiveBuffers(ds, pixels);
    std::vector<uint32_t> order;
    imagePixelOrder(settings.width, settings.height, order);
    HIP_CHECK(hipMemcpyAsync(b.lists[0], order.data(), pixels * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    zeroAdaptiveState(b, pixels, stream);
    HIP_CHECK(hipStreamSynchronize(stream));   // `order` is pageable host memory

    PtrAdaptiveInfo local{};
    PtrRenderStats sum{};
    uint32_t active = static_cast<uint32_t>(pixels), n = 0u, turn = 0u;
    const uint64_t maxItems = maxPassItems(ds);
    // PTR_VERBOSE=launches: device events around the kernels between the rounds
    struct Marks {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Marks() {
            for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev);
        }
        hipEvent_t operator[](int i) const { return e[i]; }
    } marks;
    const bool timed = ptr::readKnobs().verboseLaunches;
    if (timed) {
        for (hipEvent_t& ev : marks.e) HIP_CHECK(hipEventCreate(&ev));
    }
    while (active > 0u && n < params.maxSpp) {
        const uint32_t roundSpp = adaptiveRoundSpp(params, n);
        const uint32_t* list = b.lists[turn];
        forEachSubPass(maxItems, active, roundSpp, [&](uint32_t done, uint32_t spp, bool last) {
            PtrRenderStats one{};
            traceItems(ds, settings, spp, n + done, list, active, stream, stats ? &one : nullptr, [&](const float4* items) {
                if (timed) HIP_CHECK(hipEventRecord(marks[0], stream));
                launchAdaptiveUpdate(items, list, active, spp, n + done, last, b.state, stream);
                if (timed) HIP_CHECK(hipEventRecord(marks[1], stream));
                if (last) {
                    launchAdaptiveSelect(list, active, settings.width, settings.height, b.state, params.maxSpp, params.threshold, b.scratch,
                                         b.lists[turn ^ 1u], stream);
                }
                if (timed) HIP_CHECK(hipEventRecord(marks[2], stream));
            });
            if (stats) addPassStats(one, sum);
            if (timed) {   // debugging aid, like the [launch] lines of a pass (tools/adaptive_cost.py parses it)
                float updateMs = 0.0f, selectMs = 0.0f;
                HIP_CHECK(hipEventElapsedTime(&updateMs, marks[0], marks[1]));
                HIP_CHECK(hipEventElapsedTime(&selectMs, marks[1], marks[2]));
                std::fprintf(stderr, "[adaptive] round %u first sample %u: %u active x %u spp; update %.4f ms, select + compact %.4f ms\n", local.rounds,
                             n + done, active, spp, updateMs, last ? selectMs : 0.0f);
            }
        });
        n += roundSpp;
        local.totalSamples += static_cast<uint64_t>(active) * roundSpp;
        if (n >= params.maxSpp) local.pixelsAtMax = active;
        HIP_CHECK(hipMemcpy(&active, b.scratch.total, sizeof(uint32_t), hipMemcpyDeviceToHost));   // (traceItems joined the stream)
        if (local.rounds < PTR_ADAPTIVE_INFO_ROUNDS) local.activeAfter[local.rounds] = active;
        ++local.rounds;
        turn ^= 1u;
    }
    launchAdaptiveFinish(b.state, static_cast<uint32_t>(pixels), dRgb, dCov, dCount, stream);
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
    const std::string bad = badRender("ptr_render_adaptive_device", scene && settings && params && d_out_rgb, settings, params);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    if (ptr_device_count() < 1) {
        setErr(err, err_cap, "ptr_render_adaptive_device: no HIP device (the HIP path has no CPU fallback)");
        return 2;
    }
    try {
        renderAdaptive(*scene, *settings, *params, static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_cov), static_cast<uint32_t*>(d_out_count),
                       static_cast<hipStream_t>(stream), stats, info);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_render_adaptive(PtrDeviceScene* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, float* out_rgb,
                        float* out_cov, uint32_t* out_count, PtrRenderStats* stats, PtrAdaptiveInfo* info, char* err, size_t err_cap) {
    const std::string bad = badRender("ptr_render_adaptive", scene && settings && params && out_rgb, settings, params);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    if (ptr_device_count() < 1) {
        setErr(err, err_cap, "ptr_render_adaptive: no HIP device (the HIP path has no CPU fallback)");
        return 2;
    }
    try {
        const size_t pixels = static_cast<size_t>(settings->width) * settings->height;
        HIP_CHECK(hipSetDevice(scene->device));
        scene->adaptiveOut.ensure(pixels * 10u);   // rgb 3, cov 6, count 1 (as words)
        float* dRgb = scene->adaptiveOut.ptr;
        float* dCov = out_cov ? dRgb + pixels * 3u : nullptr;
        uint32_t* dCount = out_count ? reinterpret_cast<uint32_t*>(dRgb + pixels * 9u) : nullptr;
        renderAdaptive(*scene, *settings, *params, dRgb, dCov, dCount, nullptr, stats, info);
        HIP_CHECK(hipMemcpy(out_rgb, dRgb, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
        if (out_cov) HIP_CHECK(hipMemcpy(out_cov, dCov, pixels * 6u * sizeof(float), hipMemcpyDeviceToHost));
        if (out_count) HIP_CHECK(hipMemcpy(out_count, dCount, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
    } else if (width == 0u || height == 0u || static_cast<uint64_t>(width) * height > 0xFFFF0000ull) {
        bad = std::string(who) + ": image size must be non-zero";
    } else if ((bad = badAdaptiveParams(who, *params)).empty()) {
        const uint64_t pixels = static_cast<uint64_t>(width) * height;
        if (active_count == 0u || active_count > pixels || round_spp == 0u) bad = std::string(who) + ": the list and the round must not be empty";
        else if (static_cast<uint64_t>(n_before) + round_spp > params->maxSpp) bad = std::string(who) + ": the round goes past maxSpp";
        else if (static_cast<uint64_t>(active_count) * round_spp > 0xFFFF0000ull) bad = std::string(who) + ": too many samples";
        for (uint32_t j = 0; bad.empty() && j < active_count; ++j) {
            if (list[j] >= pixels) bad = std::string(who) + ": the list names a pixel outside the image";
        }
    }
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    if (ptr_device_count() < 1) {
        setErr(err, err_cap, std::string(who) + ": no HIP device (the HIP path has no CPU fallback)");
        return 2;
    }
    try {
        HIP_CHECK(hipSetDevice(0));
        const size_t pixels = static_cast<size_t>(width) * height;
        const size_t blocks = (static_cast<size_t>(active_count) + kAdaptiveBlock - 1u) / kAdaptiveBlock;
        DeviceBuffer<float> dSum, dMean, dM, dE;
        DeviceBuffer<uint32_t> dN, dList, dNext, dWords;
        DeviceBuffer<uint8_t> dKeep;
        DeviceBuffer<float4> dItems;
        dSum.upload(sum, pixels * 3u);
        dMean.upload(mean, pixels * 3u);
        dM.upload(m, pixels * 6u);
        dE.upload(e, pixels);
        dN.upload(n, pixels);
        dList.upload(list, active_count);
        dNext.upload(out_next, active_count);
        dWords.ensure(blocks * 2u + 1u);
        dKeep.ensure(active_count);
        dItems.upload(reinterpret_cast<const float4*>(samples), static_cast<size_t>(active_count) * round_spp);
        const AdaptiveState state{dSum.ptr, dMean.ptr, dM.ptr, dN.ptr, dE.ptr};
        launchAdaptiveUpdate(dItems.ptr, dList.ptr, active_count, round_spp, n_before, last_sub_pass != 0, state, nullptr);
        uint32_t nextCount = active_count;
        if (last_sub_pass) {
            const AdaptiveScratch scratch{dKeep.ptr, dWords.ptr, dWords.ptr + blocks, dWords.ptr + 2u * blocks};
            launchAdaptiveSelect(dList.ptr, active_count, width, height, state, params->maxSpp, params->threshold, scratch, dNext.ptr, nullptr);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (last_sub_pass) {
            HIP_CHECK(hipMemcpy(&nextCount, dWords.ptr + 2u * blocks, sizeof(uint32_t), hipMemcpyDeviceToHost));
            dNext.download(out_next, active_count);
        } else {
            std::memcpy(out_next, list, static_cast<size_t>(active_count) * sizeof(uint32_t));
        }
        dSum.download(sum, pixels * 3u);
        dMean.download(mean, pixels * 3u);
        dM.download(m, pixels * 6u);
        dE.download(e, pixels);
        dN.download(n, pixels);
        *out_next_count = nextCount;
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
