// Host side of the denoiser (include/ptr_post.h): argument checks, scratch memory, the launch sequence prepare -> a-trous passes -> finish.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../kernels/denoise.h"
#include "device_scene.h"
#include "knobs.h"
#include "ptr_post.h"
#include "ptr_stats.h"

using namespace ptrhost;

namespace {

// Which kernels run LDS-tiled by default: the ones that beat the simple kernel at 1920x1080, 16 spp, timed in one job
// (tools/denoise_bench.py -> profiles/denoise_1080p.json).  None has been measured yet, so none is on.
// PTR_DENOISE_TILED=0 / 1 forces none / all that exist.
constexpr bool kPrepareTiledByDefault = false;
constexpr bool kPassTiledByDefault[3] = {false, false, false};   // steps 1, 2, 4

bool prepareTiled(int knob) { return knob < 0 ? kPrepareTiledByDefault : knob != 0; }

bool passTiled(uint32_t step, int knob) {
    if (step > ptrk::kDenoiseMaxTiledStep || knob == 0) return false;
    return knob < 0 ? kPassTiledByDefault[step == 1u ? 0 : step == 2u ? 1 : 2] : true;
}

// "<who>: ..." for a bad argument, empty when all are good.  No device call.
std::string badArgument(const char* who, const void* rgb, const void* albedo, const void* normal, uint32_t width, uint32_t height,
                        const PtrDenoiseParams* p, const void* out) {
    const std::string w(who);
    if (!rgb || !albedo || !normal || !p || !out) return w + ": null argument";
    if (width == 0 || height == 0) return w + ": image size must be non-zero";
    if (width > 32768u || height > 32768u) return w + ": image side above 32768";
    if (p->iterations < 1u || p->iterations > PTR_DENOISE_MAX_ITERATIONS) return w + ": iterations must be in 1..8";
    for (const float sigma : {p->sigmaLuminance, p->sigmaNormal, p->sigmaDepth}) {
        if (!std::isfinite(sigma) || !(sigma > 0.0f)) return w + ": sigmas must be finite and positive";
    }
    return std::string();
}

// The scratch of a device, kept across calls and grown on demand.  A call uses it in the order of its stream; `lastUse` orders the
// next call (on whichever stream) behind it, so calls on different streams cannot overlap in it.
struct Scratch {
    DeviceBuffer<float4> colour[2], guide;
    DeviceBuffer<float> slope;
    hipEvent_t lastUse = nullptr;
};

std::mutex g_scratchMutex;
std::map<int, Scratch>& scratchByDevice() {
    static auto* m = new std::map<int, Scratch>();   // never destroyed: the runtime may be gone when statics are
    return *m;
}

struct KernelTimes {   // ptr_denoise_timed: one event before every kernel and one after the last
    std::vector<hipEvent_t> events;
    std::vector<uint32_t> tiled;
};

// The whole filter on `stream` of the current device.  Caller holds g_scratchMutex.
// dCov (nullable; include/ptr_stats.h): prepare takes the variance from it instead of the 7x7 spatial estimate.
void enqueueDenoise(Scratch& s, const void* dRgb, const void* dAlbedo, const void* dNormal, uint32_t width, uint32_t height,
                    const PtrDenoiseParams& p, void* dOut, hipStream_t stream, KernelTimes* times, const void* dCov = nullptr) {
    const size_t pixels = static_cast<size_t>(width) * height;
    if (pixels > s.guide.count) {   // growing frees the old buffers, which waits for the device: nothing can still be using them
        for (auto& c : s.colour) c.ensure(pixels);
        s.guide.ensure(pixels);
        s.slope.ensure(pixels);
    }
    if (!s.lastUse) HIP_CHECK(hipEventCreateWithFlags(&s.lastUse, hipEventDisableTiming));
    else HIP_CHECK(hipStreamWaitEvent(stream, s.lastUse, 0));
    const int knob = ptr::readKnobs().denoiseTiled;
    const ptrk::DenoiseBuffers buf{{s.colour[0].ptr, s.colour[1].ptr}, s.guide.ptr, s.slope.ptr};
    size_t at = 0;
    auto mark = [&](bool tiled) {
        if (!times) return;
        HIP_CHECK(hipEventRecord(times->events[at], stream));
        if (at < times->tiled.size()) times->tiled[at] = tiled ? 1u : 0u;
        ++at;
    };
    const auto* rgb = static_cast<const float*>(dRgb);
    const auto* albedo = static_cast<const float4*>(dAlbedo);
    if (dCov) {
        mark(false);
        ptrk::launchDenoisePrepareCov(rgb, albedo, static_cast<const float4*>(dNormal), static_cast<const float*>(dCov), width, height, p, buf, stream);
    } else {
        mark(prepareTiled(knob));
        ptrk::launchDenoisePrepare(rgb, albedo, static_cast<const float4*>(dNormal), width, height, p, buf, prepareTiled(knob), stream);
    }
    uint32_t src = 0;
    for (uint32_t i = 0; i < p.iterations; ++i, src ^= 1u) {
        mark(passTiled(1u << i, knob));
        ptrk::launchDenoiseAtrous(width, height, 1u << i, p, buf, src, passTiled(1u << i, knob), stream);
    }
    mark(false);
    ptrk::launchDenoiseFinish(rgb, albedo, width, height, p, buf, src, static_cast<float*>(dOut), stream);
    mark(false);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(s.lastUse, stream));
}

// Runs `body` with the device that owns dPtr current, and puts the caller's device back.
template <typename Body>
int onDeviceOf(const void* dPtr, char* err, size_t cap, Body&& body) {
    try {
        if (ptr_device_count() < 1) {
            setErr(err, cap, "no HIP device (the HIP path has no CPU fallback)");
            return 2;
        }
        hipPointerAttribute_t attr{};
        HIP_CHECK(hipPointerGetAttributes(&attr, dPtr));
        int before = 0;
        HIP_CHECK(hipGetDevice(&before));
        HIP_CHECK(hipSetDevice(attr.device));
        try {
            std::lock_guard<std::mutex> lock(g_scratchMutex);
            body(scratchByDevice()[attr.device]);
        } catch (...) {
            (void)hipSetDevice(before);
            throw;
        }
        HIP_CHECK(hipSetDevice(before));
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

}  // namespace

extern "C" {

void ptr_denoise_default_params(PtrDenoiseParams* params) {
    if (!params) return;
    params->iterations = 5u;
    params->sigmaLuminance = 4.0f;
    params->sigmaNormal = 128.0f;
    params->sigmaDepth = 1.0f;
    params->flags = PTR_DENOISE_DEMODULATE;
}

int ptr_denoise_device(const void* d_rgb, const void* d_albedo, const void* d_normal, uint32_t width, uint32_t height,
                       const PtrDenoiseParams* params, void* d_out_rgb, void* stream, char* err, size_t err_cap) {
    const std::string bad = badArgument("ptr_denoise_device", d_rgb, d_albedo, d_normal, width, height, params, d_out_rgb);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    return onDeviceOf(d_rgb, err, err_cap, [&](Scratch& s) {
        enqueueDenoise(s, d_rgb, d_albedo, d_normal, width, height, *params, d_out_rgb, static_cast<hipStream_t>(stream), nullptr);
    });
}

int ptr_denoise_cov_device(const void* d_rgb, const void* d_albedo, const void* d_normal, const void* d_cov, uint32_t width, uint32_t height,
                           const PtrDenoiseParams* params, void* d_out_rgb, void* stream, char* err, size_t err_cap) {
    std::string bad = badArgument("ptr_denoise_cov_device", d_rgb, d_albedo, d_normal, width, height, params, d_out_rgb);
    if (bad.empty() && !d_cov) bad = "ptr_denoise_cov_device: null argument";
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    return onDeviceOf(d_rgb, err, err_cap, [&](Scratch& s) {
        enqueueDenoise(s, d_rgb, d_albedo, d_normal, width, height, *params, d_out_rgb, static_cast<hipStream_t>(stream), nullptr, d_cov);
    });
}

int ptr_denoise_timed(const void* d_rgb, const void* d_albedo, const void* d_normal, uint32_t width, uint32_t height,
                      const PtrDenoiseParams* params, void* d_out_rgb, uint32_t runs, uint32_t warmup, double* out_ms, uint32_t* out_tiled,
                      char* err, size_t err_cap) {
    std::string bad = badArgument("ptr_denoise_timed", d_rgb, d_albedo, d_normal, width, height, params, d_out_rgb);
    if (bad.empty() && (!out_ms || runs == 0u)) bad = "ptr_denoise_timed: no runs or nowhere to put their times";
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    return onDeviceOf(d_rgb, err, err_cap, [&](Scratch& s) {
        const size_t kernels = params->iterations + 2u;
        KernelTimes times;
        times.events.resize(kernels + 1u, nullptr);
        times.tiled.assign(kernels, 0u);
        struct Release {
            std::vector<hipEvent_t>& e;
            ~Release() {
                for (hipEvent_t ev : e) {
                    if (ev) (void)hipEventDestroy(ev);
                }
            }
        } release{times.events};
        for (hipEvent_t& ev : times.events) HIP_CHECK(hipEventCreate(&ev));
        std::vector<double> sum(kernels, 0.0);
        for (uint32_t run = 0; run < warmup + runs; ++run) {
            enqueueDenoise(s, d_rgb, d_albedo, d_normal, width, height, *params, d_out_rgb, nullptr, &times);
            HIP_CHECK(hipStreamSynchronize(nullptr));
            if (run < warmup) continue;
            for (size_t i = 0; i < kernels; ++i) {
                float ms = 0.0f;
                HIP_CHECK(hipEventElapsedTime(&ms, times.events[i], times.events[i + 1u]));
                sum[i] += ms;
            }
        }
        for (size_t i = 0; i < kernels; ++i) {
            out_ms[i] = sum[i] / runs;
            if (out_tiled) out_tiled[i] = times.tiled[i];
        }
    });
}

}  // extern "C"

namespace {

// ptr_denoise / ptr_denoise_cov (cov null / given): host buffers through the device and back.
int denoiseHost(const char* who, const float* rgb, const float* albedo_rgba, const float* normal_rgba, const float* cov, uint32_t width,
                uint32_t height, const PtrDenoiseParams* params, int device, float* out_rgb, double* kernel_ms, char* err, size_t err_cap) {
    try {
        const int available = ptr_device_count();
        if (device < 0 || device >= available) {
            setErr(err, err_cap, std::string(who) + ": no such HIP device (the HIP path has no CPU fallback)");
            return 2;
        }
        HIP_CHECK(hipSetDevice(device));
        const size_t pixels = static_cast<size_t>(width) * height;
        DeviceBuffer<float> dRgb;
        DeviceBuffer<float4> dAlbedo, dNormal;
        dRgb.upload(rgb, pixels * 3u);
        dAlbedo.upload(reinterpret_cast<const float4*>(albedo_rgba), pixels);
        dNormal.upload(reinterpret_cast<const float4*>(normal_rgba), pixels);
        DeviceBuffer<float> dCov;
        if (cov) dCov.upload(cov, pixels * 6u);
        hipEvent_t begin = nullptr, end = nullptr;
        struct Release {
            hipEvent_t &a, &b;
            ~Release() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } release{begin, end};
        HIP_CHECK(hipEventCreate(&begin));
        HIP_CHECK(hipEventCreate(&end));
        {
            std::lock_guard<std::mutex> lock(g_scratchMutex);
            HIP_CHECK(hipEventRecord(begin, nullptr));
            enqueueDenoise(scratchByDevice()[device], dRgb.ptr, dAlbedo.ptr, dNormal.ptr, width, height, *params, dRgb.ptr, nullptr, nullptr,
                           cov ? dCov.ptr : nullptr);
            HIP_CHECK(hipEventRecord(end, nullptr));
        }
        HIP_CHECK(hipStreamSynchronize(nullptr));
        if (kernel_ms) {
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, begin, end));
            *kernel_ms = ms;
        }
        dRgb.download(out_rgb, pixels * 3u);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // namespace

extern "C" {

int ptr_denoise(const float* rgb, const float* albedo_rgba, const float* normal_rgba, uint32_t width, uint32_t height,
                const PtrDenoiseParams* params, int device, float* out_rgb, double* kernel_ms, char* err, size_t err_cap) {
    const std::string bad = badArgument("ptr_denoise", rgb, albedo_rgba, normal_rgba, width, height, params, out_rgb);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    return denoiseHost("ptr_denoise", rgb, albedo_rgba, normal_rgba, nullptr, width, height, params, device, out_rgb, kernel_ms, err, err_cap);
}

int ptr_denoise_cov(const float* rgb, const float* albedo_rgba, const float* normal_rgba, const float* cov, uint32_t width, uint32_t height,
                    const PtrDenoiseParams* params, int device, float* out_rgb, double* kernel_ms, char* err, size_t err_cap) {
    std::string bad = badArgument("ptr_denoise_cov", rgb, albedo_rgba, normal_rgba, width, height, params, out_rgb);
    if (bad.empty() && !cov) bad = "ptr_denoise_cov: null argument";
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    return denoiseHost("ptr_denoise_cov", rgb, albedo_rgba, normal_rgba, cov, width, height, params, device, out_rgb, kernel_ms, err, err_cap);
}

}  // extern "C"
