// Host side of temporal accumulation (include/ptr_temporal.h, include/ptr_temporal_cov.h): the handle's buffers, the argument checks, and
// the launch sequence of a step: k_surface -> k_temporal_accumulate or k_temporal_accumulate_cov -> the pose snapshot of a dynamic scene.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../kernels/temporal.h"
#include "device_scene.h"
#include "ptr_temporal.h"
#include "ptr_temporal_cov.h"

using namespace ptrhost;
using namespace ptrk;

struct PtrTemporal {
    PtrDeviceScene* scene = nullptr;
    uint32_t width = 0, height = 0;
    PtrTemporalParams params{};
    // ping-pong: [cur] is written by the step being enqueued, [cur ^ 1] holds the previous step's
    DeviceBuffer<float4> records[2][3], history[2];
    DeviceBuffer<float4> snapTris, snapSpheres;   // dynamic scenes: the rows of the previous step's pose
    bool carriesCov = false;                      // made by ptr_temporal_create_cov: one kind for life
    PtrTemporalCovParams covParams{};
    DeviceBuffer<float> covHistory[2];            // carriesCov: 6 floats per pixel in two planes (kernels/temporal.h), ping-ponged with history
    TemporalCamera prevCamera{};
    uint32_t cur = 0, frameIndex = 0;
    bool hasHistory = false, hasSnapshot = false;
    hipEvent_t events[4] = {nullptr, nullptr, nullptr, nullptr};
    ~PtrTemporal() {
        for (hipEvent_t e : events) {
            if (e) (void)hipEventDestroy(e);
        }
    }
};

namespace {

// "" or what is wrong with the params.  No device call.
std::string badParams(const PtrTemporalParams& p) {
    if (p.maxHistory < 1u || p.maxHistory > 65535u) return "maxHistory must be in 1..65535";
    if (!(p.normalCos >= -1.0f && p.normalCos <= 1.0f)) return "normalCos must be in -1..1";
    if (!(p.planeTolerance > 0.0f) || !std::isfinite(p.planeTolerance)) return "planeTolerance must be finite and positive";
    if (p.flags != 0u) return "unknown flag";
    return std::string();
}

std::string badCovParams(const PtrTemporalCovParams& p) {
    if (!(p.rejectSigma >= 0.0f) || !std::isfinite(p.rejectSigma)) return "rejectSigma must be finite and not negative";
    if (p.flags != 0u) return "unknown flag";
    return std::string();
}

std::string badSize(uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u) return "image size must be non-zero";
    if (width > 32768u || height > 32768u) return "image side above 32768";
    return std::string();
}

// "" or why a kernel on `device` cannot use `bytes` at `p`: the pointer alone is looked at, never what it points to
std::string bufferProblem(const void* p, size_t bytes, size_t align, int device) {
    if (reinterpret_cast<uintptr_t>(p) & (align - 1u)) return "is not " + std::to_string(align) + " B aligned";
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // (a pointer the runtime has never seen)
        return "is host memory, not device memory";
    }
    if (attr.type != hipMemoryTypeDevice || attr.isManaged) return "is not plain device memory";
    if (attr.device != device) return "is memory of device " + std::to_string(attr.device) + ", not of the scene's device " + std::to_string(device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();   // (no range on record)
        return std::string();
    }
    const uintptr_t end = reinterpret_cast<uintptr_t>(base) + size, at = reinterpret_cast<uintptr_t>(p);
    if (at > end || end - at < bytes) return "is shorter than the image";
    return std::string();
}

TemporalCamera cameraOf(const PtrSettings& s, RenderParams& rp) {
    fillRenderParams(s, 1u, rp);
    TemporalCamera c;
    std::memcpy(c.o, rp.cam.origin, sizeof(c.o));
    std::memcpy(c.ll, rp.cam.lowerLeft, sizeof(c.ll));
    std::memcpy(c.h, rp.cam.horizontal, sizeof(c.h));
    std::memcpy(c.w, rp.cam.vertical, sizeof(c.w));
    return c;
}

// What every step function refuses alike: 0, or 1 with the message set.  `cov`: the caller is a ptr_temporal_step_cov* function.
int refuseStep(const char* who, const PtrTemporal* t, const PtrSettings* settings, const void* rgb, const void* out, char* err, size_t cap,
               bool cov = false) {
    if (!t || !settings || !rgb || !out) return nullArgument(who, err, cap);
    if (t->carriesCov != cov) return refuse(err, cap, std::string(who) + (cov ? ": this handle carries no covariance" : ": this handle carries covariance"));
    if (settings->width != t->width || settings->height != t->height) {
        return refuse(err, cap, std::string(who) + ": the settings are " + std::to_string(settings->width) + "x" + std::to_string(settings->height) +
                                    ", the handle is " + std::to_string(t->width) + "x" + std::to_string(t->height));
    }
    return 0;
}

// One step on `stream` of the scene's device (current).  Every argument has been checked.  dCov, dOutCov: of a handle that carries
// covariance, null otherwise.
void enqueueStep(PtrTemporal& t, const PtrSettings& settings, const float* dRgb, float* dOut, float* dLength, float4* dAlbedo, float4* dNormal,
                 hipStream_t stream, PtrTemporalInfo* info, const float* dCov = nullptr, float* dOutCov = nullptr) {
    PtrDeviceScene& ds = *t.scene;
    RenderParams rp;
    const TemporalCamera camera = cameraOf(settings, rp);
    const uint32_t cur = t.cur, old = t.cur ^ 1u;
    const float4* prevTris = t.hasSnapshot ? t.snapTris.ptr : ds.view.tris;
    const float4* prevSpheres = t.hasSnapshot ? t.snapSpheres.ptr : ds.view.spheres;
    HIP_CHECK(hipEventRecord(t.events[0], stream));
    launchSurface(rp, ds.view, prevTris, prevSpheres, t.records[cur][0].ptr, t.records[cur][1].ptr, t.records[cur][2].ptr, dAlbedo, dNormal,
                  coldLaunchConfig(ds), stream);
    HIP_CHECK(hipEventRecord(t.events[1], stream));
    const TemporalBuffers buf{t.records[cur][0].ptr, t.records[cur][1].ptr, t.records[cur][2].ptr, t.records[old][0].ptr,
                              t.records[old][1].ptr, t.history[old].ptr, t.history[cur].ptr};
    const TemporalCamera& before = t.hasHistory ? t.prevCamera : camera;
    if (t.carriesCov) {
        const TemporalCovBuffers cov{dCov, dOutCov, t.covHistory[old].ptr, t.covHistory[cur].ptr};
        launchTemporalAccumulateCov(dRgb, buf, cov, camera, before, t.width, t.height, t.params, t.covParams.rejectSigma, t.hasHistory, dOut, dLength,
                                    stream);
    } else {
        launchTemporalAccumulate(dRgb, buf, camera, before, t.width, t.height, t.params, t.hasHistory, dOut, dLength, stream);
    }
    HIP_CHECK(hipEventRecord(t.events[2], stream));
    const bool snapshot = ds.dynamic != nullptr;
    if (snapshot) {
        const size_t tris = static_cast<size_t>(ds.dynamic->triCount) * 3u, spheres = ds.dynamic->sphereCount;
        if (tris) HIP_CHECK(hipMemcpyAsync(t.snapTris.ptr, ds.view.tris, tris * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        if (spheres) HIP_CHECK(hipMemcpyAsync(t.snapSpheres.ptr, ds.view.spheres, spheres * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    }
    HIP_CHECK(hipEventRecord(t.events[3], stream));
    HIP_CHECK(hipGetLastError());
    if (info) {
        info->frameIndex = t.frameIndex;
        info->hadHistory = t.hasHistory ? 1u : 0u;
    }
    t.prevCamera = camera;
    t.cur = old;
    t.hasHistory = true;
    t.hasSnapshot = snapshot;
    ++t.frameIndex;
    if (info) {
        HIP_CHECK(hipEventSynchronize(t.events[3]));
        float ms[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], t.events[i], t.events[i + 1]));
        info->surfaceMs = ms[0];
        info->accumulateMs = ms[1];
        info->snapshotMs = snapshot ? ms[2] : 0.0;
    }
}

}  // namespace

extern "C" {

void ptr_temporal_default_params(PtrTemporalParams* params) {
    if (!params) return;
    params->maxHistory = 32u;
    params->normalCos = 0.9f;
    params->planeTolerance = 0.01f;
    params->flags = 0u;
}

int ptr_temporal_check_params(const PtrTemporalParams* params, char* err, size_t err_cap) {
    if (!params) return nullArgument("ptr_temporal_check_params", err, err_cap);
    const std::string bad = badParams(*params);
    return bad.empty() ? 0 : refuse(err, err_cap, "ptr_temporal_check_params: " + bad);
}

void ptr_temporal_cov_default_params(PtrTemporalCovParams* params) {
    if (!params) return;
    params->rejectSigma = 3.0f;
    params->flags = 0u;
}

int ptr_temporal_cov_check_params(const PtrTemporalCovParams* params, char* err, size_t err_cap) {
    if (!params) return nullArgument("ptr_temporal_cov_check_params", err, err_cap);
    const std::string bad = badCovParams(*params);
    return bad.empty() ? 0 : refuse(err, err_cap, "ptr_temporal_cov_check_params: " + bad);
}

}  // extern "C"

namespace {

// ptr_temporal_create (carriesCov false, covParams unused) and ptr_temporal_create_cov
int createTemporal(const char* who, PtrDeviceScene* scene, uint32_t width, uint32_t height, const PtrTemporalParams* params, bool carriesCov,
                   const PtrTemporalCovParams* covParams, PtrTemporal** out, char* err, size_t err_cap) {
    if (out) *out = nullptr;
    if (!scene || !out) return nullArgument(who, err, err_cap);
    PtrTemporalParams p;
    ptr_temporal_default_params(&p);
    if (params) p = *params;
    PtrTemporalCovParams cp;
    ptr_temporal_cov_default_params(&cp);
    if (covParams) cp = *covParams;
    std::string bad = badParams(p);
    if (bad.empty() && carriesCov) bad = badCovParams(cp);
    if (bad.empty()) bad = badSize(width, height);
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    return deviceCall(who, scene, true, err, err_cap, [&] {
        auto t = std::make_unique<PtrTemporal>();
        t->scene = scene;
        t->width = width;
        t->height = height;
        t->params = p;
        const size_t pixels = static_cast<size_t>(width) * height;
        for (auto& set : t->records) {
            for (auto& r : set) r.ensure(pixels);
        }
        for (auto& h : t->history) h.ensure(pixels);
        t->carriesCov = carriesCov;
        t->covParams = cp;
        if (carriesCov) {
            for (auto& h : t->covHistory) h.ensure(pixels * 6u);
        }
        if (scene->dynamic) {
            t->snapTris.ensure(static_cast<size_t>(scene->dynamic->triCount) * 3u);
            t->snapSpheres.ensure(scene->dynamic->sphereCount);
        }
        for (hipEvent_t& e : t->events) HIP_CHECK(hipEventCreate(&e));
        *out = t.release();
    });
}

// in place is safe, a lane reads its own values before it writes them; at an offset lanes would race
bool overlapAtAnOffset(const void* in, const void* out, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    return a != b && a < b + bytes && b < a + bytes;
}

// ptr_temporal_step_device (cov false; d_cov and d_out_cov null) and ptr_temporal_step_cov_device
int stepDevice(const char* who, bool cov, PtrTemporal* temporal, const PtrSettings* settings, const void* d_rgb, const void* d_cov, void* d_out_rgb,
               void* d_out_cov, void* d_out_length, void* d_out_albedo, void* d_out_normal, void* stream, PtrTemporalInfo* info, char* err,
               size_t err_cap) {
    if (cov && (!d_cov || !d_out_cov)) return nullArgument(who, err, err_cap);
    if (const int rc = refuseStep(who, temporal, settings, d_rgb, d_out_rgb, err, err_cap, cov)) return rc;
    const size_t pixels = static_cast<size_t>(temporal->width) * temporal->height;
    const int device = temporal->scene->device;
    struct Buffer {
        const char* name;
        const void* p;
        size_t bytes, align;
    };
    for (const Buffer& b : {Buffer{"d_rgb", d_rgb, pixels * 12u, 4u}, Buffer{"d_cov", d_cov, pixels * 24u, 8u},
                            Buffer{"d_out_rgb", d_out_rgb, pixels * 12u, 4u}, Buffer{"d_out_cov", d_out_cov, pixels * 24u, 8u},
                            Buffer{"d_out_length", d_out_length, pixels * 4u, 4u}, Buffer{"d_out_albedo", d_out_albedo, pixels * 16u, 16u},
                            Buffer{"d_out_normal", d_out_normal, pixels * 16u, 16u}}) {
        if (!b.p) continue;
        const std::string bad = bufferProblem(b.p, b.bytes, b.align, device);
        if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + b.name + " " + bad);
    }
    if (overlapAtAnOffset(d_rgb, d_out_rgb, pixels * 12u)) return refuse(err, err_cap, std::string(who) + ": d_rgb and d_out_rgb overlap without being equal");
    if (cov && overlapAtAnOffset(d_cov, d_out_cov, pixels * 24u)) {
        return refuse(err, err_cap, std::string(who) + ": d_cov and d_out_cov overlap without being equal");
    }
    return deviceCall(who, temporal->scene, true, err, err_cap, [&] {
        enqueueStep(*temporal, *settings, static_cast<const float*>(d_rgb), static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_length),
                    static_cast<float4*>(d_out_albedo), static_cast<float4*>(d_out_normal), static_cast<hipStream_t>(stream), info,
                    static_cast<const float*>(d_cov), static_cast<float*>(d_out_cov));
    });
}

// ptr_temporal_step (cov false; cov_in and out_cov null) and ptr_temporal_step_cov
int stepHost(const char* who, bool cov, PtrTemporal* temporal, const PtrSettings* settings, const float* rgb, const float* cov_in, float* out_rgb,
             float* out_cov, float* out_length, float* out_albedo, float* out_normal, PtrTemporalInfo* info, char* err, size_t err_cap) {
    if (cov && (!cov_in || !out_cov)) return nullArgument(who, err, err_cap);
    if (const int rc = refuseStep(who, temporal, settings, rgb, out_rgb, err, err_cap, cov)) return rc;
    return deviceCall(who, temporal->scene, true, err, err_cap, [&] {
        const size_t pixels = static_cast<size_t>(temporal->width) * temporal->height;
        DeviceBuffer<float> dRgb, dCov, dLength;
        DeviceBuffer<float4> dAlbedo, dNormal;
        dRgb.upload(rgb, pixels * 3u);
        if (cov) dCov.upload(cov_in, pixels * 6u);
        if (out_length) dLength.ensure(pixels);
        if (out_albedo) dAlbedo.ensure(pixels);
        if (out_normal) dNormal.ensure(pixels);
        enqueueStep(*temporal, *settings, dRgb.ptr, dRgb.ptr, dLength.ptr, dAlbedo.ptr, dNormal.ptr, nullptr, info, dCov.ptr, dCov.ptr);
        HIP_CHECK(hipStreamSynchronize(nullptr));
        dRgb.download(out_rgb, pixels * 3u);
        if (cov) dCov.download(out_cov, pixels * 6u);
        if (out_length) dLength.download(out_length, pixels);
        if (out_albedo) dAlbedo.download(reinterpret_cast<float4*>(out_albedo), pixels);
        if (out_normal) dNormal.download(reinterpret_cast<float4*>(out_normal), pixels);
    });
}

// ptr_debug_temporal_accumulate (cov_params null, and with it cov, cov_history, out_cov, out_cov_history) and
// ptr_debug_temporal_accumulate_cov: one of the two kernels alone on host-given buffers.  The covariance histories cross the ABI in image
// order, six floats per pixel, and are put into the kernel's two planes (kernels/temporal.h) here.
int accumulateProbe(const char* who, uint32_t width, uint32_t height, const PtrTemporalParams* params, const PtrTemporalCovParams* cov_params,
                    int has_history, const float* rgb, const float* cov, const float* cur_records, const float* prev_records, const float* history,
                    const float* cov_history, const float* cam_cur, const float* cam_prev, int device, float* out_rgb, float* out_cov,
                    float* out_length, float* out_history, float* out_cov_history, char* err, size_t err_cap) {
    if (!params || !rgb || !cur_records || !prev_records || !history || !cam_cur || !cam_prev || !out_rgb || !out_length || !out_history) {
        return nullArgument(who, err, err_cap);
    }
    std::string bad = badParams(*params);
    if (bad.empty() && cov_params) bad = badCovParams(*cov_params);
    if (bad.empty()) bad = badSize(width, height);
    if (!bad.empty()) return refuse(err, err_cap, std::string(who) + ": " + bad);
    try {
        if (device < 0 || device >= ptr_device_count()) return noDevice(who, err, err_cap);
        HIP_CHECK(hipSetDevice(device));
        const size_t pixels = static_cast<size_t>(width) * height;
        DeviceBuffer<float> dRgb, dOut, dLength;
        DeviceBuffer<float4> dCur, dPrev, dHistory, dHistoryOut;
        dRgb.upload(rgb, pixels * 3u);
        dCur.upload(reinterpret_cast<const float4*>(cur_records), pixels * 3u);
        dPrev.upload(reinterpret_cast<const float4*>(prev_records), pixels * 2u);
        dHistory.upload(reinterpret_cast<const float4*>(history), pixels);
        dHistoryOut.ensure(pixels);
        dOut.ensure(pixels * 3u);
        dLength.ensure(pixels);
        TemporalCamera cams[2];
        std::memcpy(&cams[0], cam_cur, sizeof(TemporalCamera));
        std::memcpy(&cams[1], cam_prev, sizeof(TemporalCamera));
        const TemporalBuffers buf{dCur.ptr, dCur.ptr + pixels, dCur.ptr + 2u * pixels, dPrev.ptr, dPrev.ptr + pixels, dHistory.ptr, dHistoryOut.ptr};
        DeviceBuffer<float> dCov, dOutCov, dCovHistory, dCovHistoryOut;
        std::vector<float> planes(cov_params ? pixels * 6u : 0u);
        if (cov_params) {
            for (size_t i = 0; i < pixels; ++i) {
                std::memcpy(&planes[i * 4u], &cov_history[i * 6u], 4u * sizeof(float));
                std::memcpy(&planes[pixels * 4u + i * 2u], &cov_history[i * 6u + 4u], 2u * sizeof(float));
            }
            dCov.upload(cov, pixels * 6u);
            dCovHistory.upload(planes.data(), pixels * 6u);
            dOutCov.ensure(pixels * 6u);
            dCovHistoryOut.ensure(pixels * 6u);
            const TemporalCovBuffers covBuf{dCov.ptr, dOutCov.ptr, dCovHistory.ptr, dCovHistoryOut.ptr};
            launchTemporalAccumulateCov(dRgb.ptr, buf, covBuf, cams[0], cams[1], width, height, *params, cov_params->rejectSigma, has_history != 0,
                                        dOut.ptr, dLength.ptr, nullptr);
        } else {
            launchTemporalAccumulate(dRgb.ptr, buf, cams[0], cams[1], width, height, *params, has_history != 0, dOut.ptr, dLength.ptr, nullptr);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(nullptr));
        dOut.download(out_rgb, pixels * 3u);
        dLength.download(out_length, pixels);
        dHistoryOut.download(reinterpret_cast<float4*>(out_history), pixels);
        if (cov_params) {
            dOutCov.download(out_cov, pixels * 6u);
            dCovHistoryOut.download(planes.data(), pixels * 6u);
            for (size_t i = 0; i < pixels; ++i) {
                std::memcpy(&out_cov_history[i * 6u], &planes[i * 4u], 4u * sizeof(float));
                std::memcpy(&out_cov_history[i * 6u + 4u], &planes[pixels * 4u + i * 2u], 2u * sizeof(float));
            }
        }
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // namespace

extern "C" {

int ptr_temporal_create(PtrDeviceScene* scene, uint32_t width, uint32_t height, const PtrTemporalParams* params, PtrTemporal** out, char* err,
                        size_t err_cap) {
    return createTemporal("ptr_temporal_create", scene, width, height, params, false, nullptr, out, err, err_cap);
}

void ptr_temporal_release(PtrTemporal* temporal) {
    if (!temporal) return;
    (void)hipSetDevice(temporal->scene->device);
    (void)hipDeviceSynchronize();   // a step may still be running on some stream
    delete temporal;
}

int ptr_temporal_reset(PtrTemporal* temporal) {
    if (!temporal) return 1;
    temporal->hasHistory = false;
    temporal->hasSnapshot = false;
    temporal->frameIndex = 0u;
    return 0;
}

int ptr_temporal_step_device(PtrTemporal* temporal, const PtrSettings* settings, const void* d_rgb, void* d_out_rgb, void* d_out_length,
                             void* d_out_albedo, void* d_out_normal, void* stream, PtrTemporalInfo* info, char* err, size_t err_cap) {
    return stepDevice("ptr_temporal_step_device", false, temporal, settings, d_rgb, nullptr, d_out_rgb, nullptr, d_out_length, d_out_albedo,
                      d_out_normal, stream, info, err, err_cap);
}

int ptr_temporal_step(PtrTemporal* temporal, const PtrSettings* settings, const float* rgb, float* out_rgb, float* out_length, float* out_albedo,
                      float* out_normal, PtrTemporalInfo* info, char* err, size_t err_cap) {
    return stepHost("ptr_temporal_step", false, temporal, settings, rgb, nullptr, out_rgb, nullptr, out_length, out_albedo, out_normal, info, err,
                    err_cap);
}

int ptr_temporal_create_cov(PtrDeviceScene* scene, uint32_t width, uint32_t height, const PtrTemporalParams* params,
                            const PtrTemporalCovParams* cov_params, PtrTemporal** out, char* err, size_t err_cap) {
    return createTemporal("ptr_temporal_create_cov", scene, width, height, params, true, cov_params, out, err, err_cap);
}

int ptr_temporal_step_cov_device(PtrTemporal* temporal, const PtrSettings* settings, const void* d_rgb, const void* d_cov, void* d_out_rgb,
                                 void* d_out_cov, void* d_out_length, void* d_out_albedo, void* d_out_normal, void* stream,
                                 PtrTemporalInfo* info, char* err, size_t err_cap) {
    return stepDevice("ptr_temporal_step_cov_device", true, temporal, settings, d_rgb, d_cov, d_out_rgb, d_out_cov, d_out_length, d_out_albedo,
                      d_out_normal, stream, info, err, err_cap);
}

int ptr_temporal_step_cov(PtrTemporal* temporal, const PtrSettings* settings, const float* rgb, const float* cov, float* out_rgb,
                          float* out_cov, float* out_length, float* out_albedo, float* out_normal, PtrTemporalInfo* info, char* err,
                          size_t err_cap) {
    return stepHost("ptr_temporal_step_cov", true, temporal, settings, rgb, cov, out_rgb, out_cov, out_length, out_albedo, out_normal, info, err,
                    err_cap);
}

int ptr_debug_temporal_accumulate(uint32_t width, uint32_t height, const PtrTemporalParams* params, int has_history, const float* rgb,
                                  const float* cur_records, const float* prev_records, const float* history, const float* cam_cur,
                                  const float* cam_prev, int device, float* out_rgb, float* out_length, float* out_history, char* err,
                                  size_t err_cap) {
    return accumulateProbe("ptr_debug_temporal_accumulate", width, height, params, nullptr, has_history, rgb, nullptr, cur_records, prev_records,
                           history, nullptr, cam_cur, cam_prev, device, out_rgb, nullptr, out_length, out_history, nullptr, err, err_cap);
}

int ptr_debug_temporal_accumulate_cov(uint32_t width, uint32_t height, const PtrTemporalParams* params, const PtrTemporalCovParams* cov_params,
                                      int has_history, const float* rgb, const float* cov, const float* cur_records, const float* prev_records,
                                      const float* history, const float* cov_history, const float* cam_cur, const float* cam_prev, int device,
                                      float* out_rgb, float* out_cov, float* out_length, float* out_history, float* out_cov_history, char* err,
                                      size_t err_cap) {
    const char* who = "ptr_debug_temporal_accumulate_cov";
    if (!cov_params || !cov || !cov_history || !out_cov || !out_cov_history) return nullArgument(who, err, err_cap);
    return accumulateProbe(who, width, height, params, cov_params, has_history, rgb, cov, cur_records, prev_records, history, cov_history, cam_cur,
                           cam_prev, device, out_rgb, out_cov, out_length, out_history, out_cov_history, err, err_cap);
}

int ptr_debug_temporal_records(PtrTemporal* temporal, float* out_r0, float* out_r1, float* out_r2, char* err, size_t err_cap) {
    const char* who = "ptr_debug_temporal_records";
    if (!temporal) return nullArgument(who, err, err_cap);
    if (!temporal->hasHistory) return refuse(err, err_cap, std::string(who) + ": no step since create or reset");
    return deviceCall(who, temporal->scene, true, err, err_cap, [&] {
        HIP_CHECK(hipDeviceSynchronize());
        const size_t pixels = static_cast<size_t>(temporal->width) * temporal->height;
        float* outs[3] = {out_r0, out_r1, out_r2};
        for (int k = 0; k < 3; ++k) {
            if (outs[k]) temporal->records[temporal->cur ^ 1u][k].download(reinterpret_cast<float4*>(outs[k]), pixels);
        }
    });
}

int ptr_debug_temporal_camera(const PtrSettings* settings, float* out) {
    if (!settings || !out) return 1;
    RenderParams rp;
    const TemporalCamera c = cameraOf(*settings, rp);
    std::memcpy(out, &c, sizeof(c));
    return 0;
}

}  // extern "C"
