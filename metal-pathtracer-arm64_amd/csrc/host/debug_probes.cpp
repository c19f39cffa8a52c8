// The test-only entry points of include/ptr_debug.h that need the device code or the device scene: each runs one device function (or one
// production kernel) on a batch so that a test can compare it with the oracle.  Compiled with hipcc (host code only), like hip_backend.cpp;
// the host-only probes live in cabi_host.cpp, and ptr_debug_render_multi_on beside ptr_render_multi in multi.cpp.
//
// A probe is deviceCall (device_scene.h) around its buffers, its launch on the null stream and its downloads.
#include <algorithm>
#include <cmath>

#include "device_scene.h"
#include "ptr_background.h"
#include "ptr_debug.h"
#include "ptr_debug_path.h"
#include "ptr_debug_pbr.h"
#include "ptr_debug_sss.h"

using namespace ptrk;
using namespace ptrhost;

namespace {

// The production traversal kernels on a batch of rays (ptr_debug_extend_rays / ptr_debug_connect_rays): both trace from kEps, which the
// batch must state; info = {node format launched (traversalNodeFormat), stack limit, four-wide depth, LDS stack levels}.
bool checkProbeRays(const float* rays, uint64_t n, bool infiniteTmax, const char* who, char* err, size_t err_cap) {
    if (n >= (1ull << kConnectMaskShift)) {
        setErr(err, err_cap, std::string(who) + ": at most 2^27 - 1 rays");
        return false;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const float tmin = rays[i * 8 + 3], tmax = rays[i * 8 + 7];
        if (tmin != 1.0e-4f || (infiniteTmax && !(std::isinf(tmax) && tmax > 0.0f))) {
            setErr(err, err_cap, std::string(who) + ": ray " + std::to_string(i) + " has tmin " + std::to_string(tmin) + " / tmax " +
                                     std::to_string(tmax) + (infiniteTmax ? "; the kernel traces from 1e-4 to infinity" : "; the kernel traces from 1e-4"));
            return false;
        }
    }
    return true;
}

void probeInfo(const PtrDeviceScene& ds, bool count, uint32_t info[4]) {
    info[0] = static_cast<uint32_t>(traversalNodeFormat(ds.view, count));
    info[1] = ds.view.stackLimit;
    info[2] = ds.view.useWide ? ds.wideDepth : 0u;
    info[3] = kLdsStackLevels;
}

// the render's launch configuration of group 0 (coldLaunchConfig plus the scene's feeder chunk), with its work heads zeroed
LaunchConfig probeLaunchConfig(const PtrDeviceScene& ds) {
    LaunchConfig cfg = coldLaunchConfig(ds);
    cfg.feederChunk = ds.feederChunk;
    HIP_CHECK(hipMemset(cfg.workCounters, 0, 2 * sizeof(uint32_t)));
    return cfg;
}

// What the BSDF probes launch with: the material as the integrator reads it, on the device, and the settings' render parameters.
struct BsdfProbe {
    DeviceBuffer<float4> material;
    RenderParams rp;
    BsdfProbe(const PtrMaterial& m, const PtrSettings& settings) {
        std::vector<float> rows;
        compactMaterial(m, rows);
        material.upload(reinterpret_cast<const float4*>(rows.data()), kMaterialVec4);
        fillRenderParams(settings, 1, rp);
    }
};

}  // namespace

extern "C" {

int ptr_debug_render_signatures(PtrDeviceScene* scene, const PtrSettings* settings, float* out_rgb, uint32_t* out_signature, char* err,
                                size_t err_cap) {
    return deviceCall("ptr_debug_render_signatures", scene, scene && settings && out_signature, err, err_cap, [&] {
        const size_t pixels = static_cast<size_t>(settings->width) * settings->height;
        const size_t floats = static_cast<size_t>(ptr_part_band_count(settings->height, 0, 1)) * PTR_BAND_ROWS * settings->width * 3u;
        scene->outBands.ensure(floats);
        PtrRenderStats stats{};
        renderBands(*scene, *settings, 1u, 0u, 1u, scene->outBands.ptr, nullptr, 1, &stats);   // counting build, 1 spp: item = local pixel
        if (out_rgb) scene->outBands.download(out_rgb, pixels * 3u);
        std::vector<float4> items(pixels);
        std::vector<uint32_t> pixelOfLocal(pixels);
        scene->itemAccum.download(items.data(), pixels);
        scene->pixelOfLocal.download(pixelOfLocal.data(), pixels);
        for (size_t lp = 0; lp < pixels; ++lp) {
            uint32_t bits;
            std::memcpy(&bits, &items[lp].w, sizeof(bits));
            out_signature[pixelOfLocal[lp]] = bits;
        }
    });
}

int ptr_debug_texture_sample(PtrDeviceScene* scene, uint32_t texture, const float* in, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_texture_sample", scene, scene && (in || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        DeviceBuffer<float> din;
        DeviceBuffer<float4> dout;
        din.upload(in, n * 3);
        dout.ensure(n);
        launchDebugTexSample(scene->view, texture, din.ptr, n, dout.ptr, nullptr);
        dout.download(reinterpret_cast<float4*>(out), n);
    });
}

int ptr_debug_texture_sample_grad(PtrDeviceScene* scene, uint32_t texture, const float* in, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_texture_sample_grad", scene, scene && (in || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        DeviceBuffer<float> din;
        DeviceBuffer<float4> dout;
        din.upload(in, n * 6);
        dout.ensure(n);
        launchDebugTexSampleGrad(scene->view, texture, din.ptr, n, dout.ptr, nullptr);
        dout.download(reinterpret_cast<float4*>(out), n);
    });
}

int ptr_debug_first_hit_textures(PtrDeviceScene* scene, const PtrSettings* settings, const uint32_t* xys, uint64_t n, float* out, char* err,
                                 size_t err_cap) {
    return deviceCall("ptr_debug_first_hit_textures", scene, scene && settings && (xys || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        constexpr uint64_t kFloats = 36;
        DeviceBuffer<uint32_t> dxy;
        DeviceBuffer<float> dout;
        dxy.upload(xys, n * 3);
        dout.ensure(n * kFloats);
        launchDebugFirstHit(rp, scene->view, dxy.ptr, n, dout.ptr, coldLaunchConfig(*scene), nullptr);
        dout.download(out, n * kFloats);
    });
}

int ptr_debug_pbr_hits(PtrDeviceScene* scene, const float* in, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_pbr_hits", scene, scene && (in || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        DeviceBuffer<float> din, dout;
        din.upload(in, n * 20);
        dout.ensure(n * 32);
        launchDebugPbrHits(scene->view, din.ptr, n, dout.ptr, coldLaunchConfig(*scene), nullptr);
        dout.download(out, n * 32);
    });
}

int ptr_debug_surface_hits(PtrDeviceScene* scene, const float* in, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_surface_hits", scene, scene && (in || !n) && (out || !n), err, err_cap, [&] {
        if (n == 0) return;
        DeviceBuffer<float> din, dout;
        din.upload(in, n * 9);
        dout.ensure(n * 16);
        launchDebugSurfaceHits(scene->view, din.ptr, n, dout.ptr, coldLaunchConfig(*scene), nullptr);
        dout.download(out, n * 16);
    });
}

int ptr_debug_extend_rays(PtrDeviceScene* scene, const float* rays, uint64_t n, int count, PtrHit* out, uint32_t info[4], char* err,
                          size_t err_cap) {
    const bool argsOk = scene && (rays || !n) && (out || !n) && info;
    if (argsOk && !checkProbeRays(rays, n, true, "ptr_debug_extend_rays", err, err_cap)) return 1;
    return deviceCall("ptr_debug_extend_rays", scene, argsOk, err, err_cap, [&] {
        probeInfo(*scene, count != 0, info);
        if (n == 0) return;
        // the slots as k_shade leaves them for k_extend: ray0 = (origin, d.x), ray1 = (d.y, d.z, pdf, flags), alive; hit words that k_extend
        // must overwrite
        std::vector<float4> state(n * 2);
        std::vector<float2> hits(n, make_float2(-2.0f, bitsToFloat(0xFFFFFFFEu)));
        for (uint64_t i = 0; i < n; ++i) {
            const float* r = rays + i * 8;
            state[i] = make_float4(r[0], r[1], r[2], r[4]);
            state[n + i] = make_float4(r[5], r[6], 0.0f, bitsToFloat(kFlagAlive));
        }
        DeviceBuffer<float4> dState, dRays;
        DeviceBuffer<float2> dHit;
        DeviceBuffer<PtrHit> dOut;
        dState.upload(state.data(), state.size());
        dHit.upload(hits.data(), hits.size());
        dRays.upload(reinterpret_cast<const float4*>(rays), n * 2);
        dOut.ensure(n);
        PathPool pool{};
        pool.ray0 = dState.ptr;
        pool.ray1 = dState.ptr + n;
        pool.hit = dHit.ptr;
        pool.slots = static_cast<uint32_t>(n);
        pool.recStride = static_cast<uint32_t>(n);
        if (count) {
            HIP_CHECK(hipMemset(scene->counters.ptr, 0, sizeof(uint64_t) * kCounterSlots));
            pool.counters = scene->counters.ptr;
        }
        launchExtend(scene->view, pool, probeLaunchConfig(*scene), nullptr, count != 0, nullptr);
        HIP_CHECK(hipGetLastError());
        launchDebugHitRecords(scene->view, dRays.ptr, dHit.ptr, n, static_cast<uint32_t>(scene->info[2]), static_cast<uint32_t>(scene->info[3]),
                              dOut.ptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        dOut.download(out, n);
    });
}

int ptr_debug_connect_rays(PtrDeviceScene* scene, const float* rays, const uint32_t* ignore_light, uint64_t n, uint32_t records_per_slot,
                           uint32_t* occluded, uint32_t info[4], char* err, size_t err_cap) {
    const bool argsOk = scene && (rays || !n) && (occluded || !n) && info;
    if (argsOk && (records_per_slot < 1u || records_per_slot > 4u)) {
        setErr(err, err_cap, "ptr_debug_connect_rays: records_per_slot must be 1..4");
        return 1;
    }
    if (argsOk && !checkProbeRays(rays, n, false, "ptr_debug_connect_rays", err, err_cap)) return 1;
    for (uint64_t i = 0; argsOk && ignore_light && i < n; ++i) {
        if (ignore_light[i] != 0xFFFFFFFFu && ignore_light[i] >= scene->view.rectLightCount) {
            setErr(err, err_cap, "ptr_debug_connect_rays: ray " + std::to_string(i) + " ignores light " + std::to_string(ignore_light[i]) +
                                     " of " + std::to_string(scene->view.rectLightCount));
            return 1;
        }
    }
    return deviceCall("ptr_debug_connect_rays", scene, argsOk, err, err_cap, [&] {
        probeInfo(*scene, false, info);
        if (n == 0) return;
        // the ignore word of a kind-3 record: the meta word of the light's own triangles (row 6 of its record, T[1].w of half 0), where
        // k_shade takes it from (rectLightSurface)
        std::vector<float4> lights(static_cast<size_t>(scene->view.rectLightCount) * kRectLightVec4);
        scene->rectLights.download(lights.data(), lights.size());
        // ray i is record i % records_per_slot of slot i / records_per_slot; the record arrays are one allocation indexed as k_connect
        // indexes them: field f of record slot k at recBase[(k*4 + f)*slots + slot]
        const uint64_t slots = (n + records_per_slot - 1u) / records_per_slot;
        std::vector<float4> rec(slots * kRecSlots * 4u, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (uint64_t i = 0; i < n; ++i) {
            const float* r = rays + i * 8;
            const uint64_t slot = i / records_per_slot, k = i % records_per_slot;
            const uint32_t light = ignore_light ? ignore_light[i] : 0xFFFFFFFFu;
            const uint32_t kind = light == 0xFFFFFFFFu ? 0u : 3u;
            rec[(k * 4u + 0u) * slots + slot] = make_float4(r[0], r[1], r[2], r[7]);
            rec[(k * 4u + 1u) * slots + slot] = make_float4(r[4], r[5], r[6], bitsToFloat(kind));
            rec[(k * 4u + 2u) * slots + slot] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            if (kind == 3u) rec[(k * 4u + 3u) * slots + slot] = make_float4(lights[static_cast<size_t>(light) * kRectLightVec4 + 6u].w, 0.0f, 0.0f, 0.0f);
        }
        // the slots spread over the connect sub-lists unevenly, as the waves of k_shade append them, with some sub-lists left empty
        std::vector<std::vector<uint32_t>> queues(kConnectQueues);
        for (uint64_t slot = 0; slot < slots; ++slot) {
            uint32_t q = static_cast<uint32_t>(((slot * 2654435761ull) >> 7) % 97u) % kConnectQueues;
            if (q % 5u == 2u) q = (q * 3u + 1u) % kConnectQueues;
            if (q % 5u == 2u) q = (q + 1u) % kConnectQueues;
            const uint32_t records = static_cast<uint32_t>(std::min<uint64_t>(records_per_slot, n - slot * records_per_slot));
            queues[q].push_back(static_cast<uint32_t>(slot) | (((1u << records) - 1u) << kConnectMaskShift));
        }
        size_t region = 1;
        for (const auto& q : queues) region = std::max(region, q.size());
        std::vector<uint32_t> list(region * kConnectQueues, 0u), counts(kConnectQueues * kConnectCountStride, 0u);
        for (uint32_t q = 0; q < kConnectQueues; ++q) {
            std::copy(queues[q].begin(), queues[q].end(), list.begin() + static_cast<size_t>(q) * region);
            counts[q * kConnectCountStride] = static_cast<uint32_t>(queues[q].size());
        }
        DeviceBuffer<float4> dRec;
        DeviceBuffer<uint32_t> dList, dCounts;
        dRec.upload(rec.data(), rec.size());
        dList.upload(list.data(), list.size());
        dCounts.upload(counts.data(), counts.size());
        PathPool pool{};
        for (uint32_t k = 0; k < kRecSlots; ++k) {
            pool.rec[k] = ShadowRecordView{dRec.ptr + (k * 4u + 0u) * slots, dRec.ptr + (k * 4u + 1u) * slots, dRec.ptr + (k * 4u + 2u) * slots,
                                           dRec.ptr + (k * 4u + 3u) * slots};
        }
        pool.slots = static_cast<uint32_t>(slots);
        pool.recStride = static_cast<uint32_t>(slots);
        pool.connectList = dList.ptr;
        pool.connectCount = dCounts.ptr;
        pool.connectRegion = static_cast<uint32_t>(region);
        RenderParams rp{};   // MNEE off: launchConnect launches k_connect alone
        launchConnect(rp, scene->view, pool, probeLaunchConfig(*scene), false, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        dRec.download(rec.data(), rec.size());
        for (uint64_t i = 0; i < n; ++i) {
            const float4 a = rec[((i % records_per_slot) * 4u + 2u) * slots + i / records_per_slot];
            occluded[i] = (a.x == 0.0f && a.y == 0.0f && a.z == 0.0f) ? 1u : 0u;
        }
    });
}

int ptr_background_debug_cull(const PtrDeviceScene* scene, const PtrSceneDesc* desc, const PtrSettings* settings, uint32_t part, uint32_t parts,
                              int count, uint32_t out[8], double bounds[7], char* err, size_t err_cap) {
    const char* who = "ptr_background_debug_cull";
    if ((!scene && !desc) || !settings || !out) return nullArgument(who, err, err_cap);
    if (parts == 0u || part >= parts) return refuse(err, err_cap, std::string(who) + ": bad partition");
    try {
        ptr::WorldBounds world;
        if (scene) {
            world = scene->worldBounds;
        } else {
            ptr::PreparedGeometry pg;
            prepareGeometry(*desc, pg);
            world = ptr::boundsOfPrimitives(pg.geo.triData.data(), pg.geo.triData.size() / 12u, pg.geo.sphereData.data(), pg.geo.sphereData.size() / 4u);
        }
        const ptr::CullRect rect = passCullRect(world, *settings, false, count != 0 ? 1 : 0);
        std::vector<uint32_t> pixels;
        partitionPixels(settings->width, settings->height, part, parts, pixels);
        uint32_t traced = 0u;
        for (const uint32_t pixel : pixels) traced += (!rect.cull || rect.inside(pixel % settings->width, pixel / settings->width)) ? 1u : 0u;
        const uint32_t words[8] = {rect.cull ? 1u : 0u, rect.x0, rect.x1, rect.y0, rect.y1, traced, static_cast<uint32_t>(pixels.size()) - traced, 0u};
        std::copy(words, words + 8, out);
        if (bounds) {
            for (int a = 0; a < 3; ++a) bounds[a] = world.lo[a], bounds[3 + a] = world.hi[a];
            bounds[6] = world.valid ? 1.0 : 0.0;
        }
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_debug_exact_division(uint32_t d, const uint32_t* n, uint64_t count, uint32_t* out) {
    if (d == 0u || (!n && count) || (!out && count)) return 1;
    const DivU32 by = makeDivU32(d);
    for (uint64_t i = 0; i < count; ++i) out[i] = by.quotient(n[i]);
    return 0;
}

int ptr_debug_shade_kernel_set(const PtrDeviceScene* scene, const PtrSettings* settings, int count, uint32_t* out) {
    if (!scene || !settings || !out) return 1;
    RenderParams rp;
    fillRenderParams(*settings, 1, rp);
    *out = shadeKernelSet(rp, scene->view, count != 0);
    return 0;
}

int ptr_debug_eval_bsdf(const PtrMaterial* material, const PtrSettings* settings, const float* in, uint64_t n, float* out,
                        char* err, size_t err_cap) {
    return deviceCall("ptr_debug_eval_bsdf", nullptr, material && settings && (in || !n) && (out || !n), err, err_cap, [&] {
        BsdfProbe probe(*material, *settings);
        DeviceBuffer<float> din, dout;
        din.upload(in, n * 12);
        dout.ensure(n * 5);
        launchDebugEvalBsdf(probe.material.ptr, probe.rp, din.ptr, n, dout.ptr, nullptr);
        dout.download(out, n * 5);
    });
}

int ptr_debug_sample_bsdf(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* front_face,
                          const uint32_t* rng_states, uint64_t n, float* out, uint32_t* out_states, char* err, size_t err_cap) {
    const bool argsOk = material && settings && ((in && front_face && rng_states && out && out_states) || !n);
    return deviceCall("ptr_debug_sample_bsdf", nullptr, argsOk, err, err_cap, [&] {
        BsdfProbe probe(*material, *settings);
        DeviceBuffer<float> din, dout;
        DeviceBuffer<uint32_t> dfront, drng, drngOut;
        din.upload(in, n * 9);
        dfront.upload(front_face, n);
        drng.upload(rng_states, n);
        dout.ensure(n * 8);
        drngOut.ensure(n);
        launchDebugSampleBsdf(probe.material.ptr, probe.rp, din.ptr, dfront.ptr, drng.ptr, n, dout.ptr, drngOut.ptr, nullptr);
        dout.download(out, n * 8);
        drngOut.download(out_states, n);
    });
}

int ptr_debug_sample_lobes(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* front_face,
                           const uint32_t* rng_states, uint64_t n, float* out, float* out_sample, uint32_t* out_states, float* env_roughness,
                           char* err, size_t err_cap) {
    const bool argsOk = material && settings && ((in && front_face && rng_states) || !n);
    return deviceCall("ptr_debug_sample_lobes", nullptr, argsOk, err, err_cap, [&] {
        BsdfProbe probe(*material, *settings);
        DeviceBuffer<float> din, dout, dsample;
        DeviceBuffer<uint32_t> dfront, drng, drngOut;
        din.upload(in, n * 9);
        dfront.upload(front_face, n);
        drng.upload(rng_states, n);
        dout.ensure(n * 3 + 1);
        dsample.ensure(n * 8);
        drngOut.ensure(n);
        if (n > 0) {
            launchDebugSampleLobes(probe.material.ptr, probe.rp, din.ptr, dfront.ptr, drng.ptr, n, dout.ptr, dsample.ptr, drngOut.ptr, nullptr);
        } else {
            HIP_CHECK(hipMemset(dout.ptr, 0, sizeof(float)));   // no launch wrote the environment-lighting roughness: it reads 0
        }
        std::vector<float> o(n * 3 + 1, 0.0f);
        dout.download(o.data(), o.size());
        if (out) std::memcpy(out, o.data(), n * 3 * sizeof(float));
        if (env_roughness) *env_roughness = o[n * 3];
        if (out_sample) dsample.download(out_sample, n * 8);
        if (out_states) drngOut.download(out_states, n);
    });
}

int ptr_debug_env_lookup(PtrDeviceScene* scene, const PtrSettings* settings, const float* in, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_env_lookup", scene, scene && settings && (in || !n) && (out || !n), err, err_cap, [&] {
        if (scene->view.envWidth == 0u) throw HipError{"ptr_debug_env_lookup: the scene has no environment map"};
        ensureEnvMips(*scene);
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        const EnvLodView env{scene->envMips.ptr, nullptr, scene->envMipLevels, 0u};
        DeviceBuffer<float4> din, dout;
        din.upload(reinterpret_cast<const float4*>(in), n);
        dout.ensure(n);
        launchDebugEnvLookup(rp, scene->view, env, din.ptr, n, dout.ptr, nullptr);
        dout.download(reinterpret_cast<float4*>(out), n);
    });
}

int ptr_debug_env_sample(PtrDeviceScene* scene, const PtrSettings* settings, const float* u, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_env_sample", scene, scene && settings && (u || !n) && (out || !n), err, err_cap, [&] {
        if (scene->view.envWidth == 0u || !scene->view.envSampling) {
            throw HipError{"ptr_debug_env_sample: the scene has no environment map with a sampling distribution"};
        }
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<float> din;
        DeviceBuffer<float4> dout;
        din.upload(u, n * 3);
        dout.ensure(n * 2);
        launchDebugEnvSample(rp, scene->view, din.ptr, n, dout.ptr, nullptr);
        dout.download(reinterpret_cast<float4*>(out), n * 2);
    });
}

int ptr_debug_env_eval(PtrDeviceScene* scene, const PtrSettings* settings, const float* dir, uint64_t n, float* out, char* err, size_t err_cap) {
    return deviceCall("ptr_debug_env_eval", scene, scene && settings && (dir || !n) && (out || !n), err, err_cap, [&] {
        if (scene->view.envWidth == 0u) throw HipError{"ptr_debug_env_eval: the scene has no environment map"};
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<float> din;
        DeviceBuffer<float4> dout;
        din.upload(dir, n * 3);
        dout.ensure(n);
        launchDebugEnvEval(rp, scene->view, din.ptr, n, dout.ptr, nullptr);
        dout.download(reinterpret_cast<float4*>(out), n);
    });
}

int ptr_debug_rect_light_nee(PtrDeviceScene* scene, const PtrSettings* settings, const PtrMaterial* material, const float* rays, const float* thr,
                             const uint32_t* rng_states, uint64_t n, float* out, uint32_t* out_states, char* err, size_t err_cap) {
    const bool argsOk = scene && settings && ((rays && thr && rng_states && out && out_states) || !n);
    return deviceCall("ptr_debug_rect_light_nee", scene, argsOk, err, err_cap, [&] {
        if (scene->view.rectLightCount == 0u) throw HipError{"ptr_debug_rect_light_nee: the scene has no rectangle light"};
        if (n >= (1ull << kConnectMaskShift)) throw HipError{"ptr_debug_rect_light_nee: at most 2^27 - 1 rays"};
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<float4> dMaterial, dRec, dHead;
        if (material) {
            std::vector<float> rows;
            compactMaterial(*material, rows);
            dMaterial.upload(reinterpret_cast<const float4*>(rows.data()), kMaterialVec4);
        }
        DeviceBuffer<float> dRays, dThr;
        DeviceBuffer<uint32_t> dRng, dRngOut;
        dRays.upload(rays, n * 6);
        dThr.upload(thr, n * 3);
        dRng.upload(rng_states, n);
        dRngOut.ensure(n);
        dHead.ensure(n);
        // record 0 of a pool of n slots: rectLightNee's storeRecord writes slot i of {org | tmax, dir | kind, contribution | depth}; zero
        // where it queued nothing
        dRec.ensure(n * 4);
        HIP_CHECK(hipMemset(dRec.ptr, 0, n * 4 * sizeof(float4)));
        PathPool pool{};
        pool.rec[0] = ShadowRecordView{dRec.ptr, dRec.ptr + n, dRec.ptr + 2 * n, dRec.ptr + 3 * n};
        pool.slots = static_cast<uint32_t>(n);
        pool.recStride = static_cast<uint32_t>(n);
        launchDebugRectLightNee(rp, scene->view, pool, material ? dMaterial.ptr : nullptr, dRays.ptr, dThr.ptr, dRng.ptr, n, dHead.ptr, dRngOut.ptr,
                                coldLaunchConfig(*scene), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<float4> rec(n * 4), head(n);
        dRec.download(rec.data(), rec.size());
        dHead.download(head.data(), n);
        dRngOut.download(out_states, n);
        for (uint64_t i = 0; i < n; ++i) {
            const float4 org = rec[i], dir = rec[n + i], a = rec[2 * n + i];
            const float row[16] = {head[i].x, head[i].y, org.x, org.y, org.z, dir.x, dir.y, dir.z, org.w, a.x, a.y, a.z, 0.0f, 0.0f, 0.0f, 0.0f};
            std::memcpy(out + i * 16, row, sizeof(row));
        }
    });
}

int ptr_debug_light_connection(PtrDeviceScene* scene, const PtrSettings* settings, const float* in, uint64_t n, float* out, uint32_t info[2],
                               char* err, size_t err_cap) {
    return deviceCall("ptr_debug_light_connection", scene, scene && settings && (in || !n) && (out || !n) && info, err, err_cap, [&] {
        info[0] = scene->view.settleRectLights;
        info[1] = scene->view.rectLightCount;
        if (n == 0) return;
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<float> din, dout;
        din.upload(in, n * 14);
        dout.ensure(n * 12);
        launchDebugLightConnection(rp, scene->view, din.ptr, n, dout.ptr, nullptr);
        dout.download(out, n * 12);
    });
}

// ---- the random-walk subsurface path (ptr_debug_sss.h) ----
// what all three refuse before any launch
static int sssProbeRefusal(const char* who, bool argsOk, const PtrSettings* settings, uint64_t n, char* err, size_t err_cap) {
    if (!argsOk) return nullArgument(who, err, err_cap);
    if (n == 0) return refuse(err, err_cap, std::string(who) + ": n == 0");
    if (settings->sssMaxSteps > PTR_SSS_MAX_STEPS) return refuse(err, err_cap, std::string(who) + ": sssMaxSteps > 64");
    return 0;
}

int ptr_debug_sss_walk_begin(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* rng_states, uint64_t n,
                             float* out, uint32_t* out_states, char* err, size_t err_cap) {
    const bool argsOk = material && settings && in && rng_states && out && out_states;
    if (const int rc = sssProbeRefusal("ptr_debug_sss_walk_begin", argsOk, settings, n, err, err_cap)) return rc;
    return deviceCall("ptr_debug_sss_walk_begin", nullptr, argsOk, err, err_cap, [&] {
        BsdfProbe probe(*material, *settings);
        DeviceBuffer<float> din, dout;
        DeviceBuffer<uint32_t> drng, drngOut;
        din.upload(in, n * PTR_SSS_BEGIN_IN);
        drng.upload(rng_states, n);
        dout.ensure(n * PTR_SSS_BEGIN_OUT);
        drngOut.ensure(n);
        launchDebugSssBegin(probe.material.ptr, probe.rp, din.ptr, drng.ptr, n, dout.ptr, drngOut.ptr, nullptr);
        dout.download(out, n * PTR_SSS_BEGIN_OUT);
        drngOut.download(out_states, n);
    });
}

int ptr_debug_sss_walk_step(const PtrMaterial* material, const PtrSettings* settings, const float* in, const uint32_t* rng_states, uint64_t n,
                            float* out, uint32_t* out_states, char* err, size_t err_cap) {
    const bool argsOk = material && settings && in && rng_states && out && out_states;
    if (const int rc = sssProbeRefusal("ptr_debug_sss_walk_step", argsOk, settings, n, err, err_cap)) return rc;
    return deviceCall("ptr_debug_sss_walk_step", nullptr, argsOk, err, err_cap, [&] {
        BsdfProbe probe(*material, *settings);
        DeviceBuffer<float> din, dout;
        DeviceBuffer<uint32_t> drng, drngOut;
        din.upload(in, n * PTR_SSS_STEP_IN);
        drng.upload(rng_states, n);
        dout.ensure(n * PTR_SSS_STEP_OUT);
        drngOut.ensure(n);
        // (the limit as the settings state it, not the render's max(., 1): the function's own clamp is part of what is tested)
        launchDebugSssStep(probe.material.ptr, settings->sssMaxSteps, din.ptr, drng.ptr, n, dout.ptr, drngOut.ptr, nullptr);
        dout.download(out, n * PTR_SSS_STEP_OUT);
        drngOut.download(out_states, n);
    });
}

int ptr_debug_sss_walks(PtrDeviceScene* scene, const PtrSettings* settings, const uint32_t* xys, uint64_t n, uint32_t step_cap, float* out_steps,
                        float* out_final, char* err, size_t err_cap) {
    const bool argsOk = scene && settings && xys && out_steps && out_final;
    if (const int rc = sssProbeRefusal("ptr_debug_sss_walks", argsOk, settings, n, err, err_cap)) return rc;
    if (step_cap == 0u || step_cap > PTR_SSS_MAX_STEPS) return refuse(err, err_cap, "ptr_debug_sss_walks: step_cap must be 1..64");
    for (uint64_t i = 0; i < n; ++i) {
        if (xys[i * 3] >= settings->width || xys[i * 3 + 1] >= settings->height) {
            return refuse(err, err_cap, "ptr_debug_sss_walks: sample " + std::to_string(i) + " is outside the image");
        }
    }
    return deviceCall("ptr_debug_sss_walks", scene, argsOk, err, err_cap, [&] {
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<uint32_t> dxy;
        DeviceBuffer<float> dsteps, dfinal;
        dxy.upload(xys, n * 3);
        dsteps.ensure(n * step_cap * PTR_SSS_WALK_STEP);
        dfinal.ensure(n * PTR_SSS_WALK_FINAL);
        HIP_CHECK(hipMemset(dsteps.ptr, 0, n * step_cap * PTR_SSS_WALK_STEP * sizeof(float)));
        DeviceBuffer<float> dstate, drows, dstepOut;
        DeviceBuffer<uint32_t> drowRng, drowMaterial, dstepRng;
        dstate.ensure(n * kSssWalkStateWords);
        drows.ensure(n * PTR_SSS_STEP_IN);
        dstepOut.ensure(n * PTR_SSS_STEP_OUT);
        drowRng.ensure(n);
        drowMaterial.ensure(n);
        dstepRng.ensure(n);
        const SssWalkScratch scratch{dstate.ptr, drows.ptr, drowRng.ptr, drowMaterial.ptr, dstepOut.ptr, dstepRng.ptr};
        launchDebugSssWalks(rp, scene->view, dxy.ptr, n, step_cap, dsteps.ptr, dfinal.ptr, scratch, coldLaunchConfig(*scene), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        dsteps.download(out_steps, n * step_cap * PTR_SSS_WALK_STEP);
        dfinal.download(out_final, n * PTR_SSS_WALK_FINAL);
    });
}

// ---- the path state, iteration by iteration (ptr_debug_path.h) ----
int ptr_debug_path_states(PtrDeviceScene* scene, const PtrSettings* settings, const uint32_t* pixels, uint64_t n, uint32_t sample,
                          uint32_t max_iterations, uint32_t* out_states, uint32_t* out_iterations, float* out_items, char* err, size_t err_cap) {
    const char* who = "ptr_debug_path_states";
    const bool argsOk = scene && settings && pixels && out_states && out_iterations && out_items;
    if (!argsOk) return nullArgument(who, err, err_cap);
    if (n == 0 || n > PTR_PATH_MAX_PIXELS) return refuse(err, err_cap, std::string(who) + ": n must be 1..2^20");
    if (max_iterations == 0u) return refuse(err, err_cap, std::string(who) + ": max_iterations == 0");
    for (uint64_t i = 0; i < n; ++i) {
        if (pixels[i] >= static_cast<uint64_t>(settings->width) * settings->height) {
            return refuse(err, err_cap, std::string(who) + ": pixel " + std::to_string(i) + " is outside the image");
        }
    }
    return deviceCall(who, scene, argsOk, err, err_cap, [&] {
        // the production loop over one group of exactly n slots, no tail kernels: the scene's knobs are put back whatever happens
        struct Knobs {
            PtrDeviceScene& ds;
            const uint64_t tailBelow, poolSlots;
            ~Knobs() { ds.tailBelow = tailBelow, ds.poolSlots = poolSlots; }
        } knobs{*scene, scene->tailBelow, scene->poolSlots};
        scene->tailBelow = 0u;
        scene->poolSlots = std::max<uint64_t>(scene->poolSlots, n);
        const uint32_t slots = static_cast<uint32_t>(n);
        DeviceBuffer<uint32_t> dPixels;
        dPixels.upload(pixels, n);
        std::memset(out_states, 0, static_cast<size_t>(max_iterations) * n * PTR_PATH_STATE_WORDS * sizeof(uint32_t));
        std::vector<float4> state(n * 4u), rec(n * kRecSlots * 4u);
        std::vector<float2> hit(n), cone(n);
        std::vector<uint4> medium(n);
        std::vector<uint32_t> flushItem(n);
        uint64_t ran = 0;
        const IterationHook hook = [&](uint64_t iteration, const PathPool& pool) {
            HIP_CHECK(hipDeviceSynchronize());
            ran = iteration + 1u;
            if (iteration >= max_iterations) return;
            if (pool.slots != slots || pool.recStride != slots) throw HipError{"ptr_debug_path_states: the pool is not one slot per pixel"};
            // (ray0, ray1, thr, accum and the record rows are one allocation each, `slots` apart: slotRange)
            HIP_CHECK(hipMemcpy(state.data(), pool.ray0, state.size() * sizeof(float4), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(rec.data(), pool.rec[0].org, rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(hit.data(), pool.hit, n * sizeof(float2), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(flushItem.data(), pool.flushItem, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (pool.medium) HIP_CHECK(hipMemcpy(medium.data(), pool.medium, n * sizeof(uint4), hipMemcpyDeviceToHost));
            if (pool.cone) HIP_CHECK(hipMemcpy(cone.data(), pool.cone, n * sizeof(float2), hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t* o = out_states + (iteration * n + i) * PTR_PATH_STATE_WORDS;
                for (uint32_t f = 0; f < 2u; ++f) std::memcpy(o + 4u * f, &state[f * n + i], sizeof(float4));
                std::memcpy(o + 8, &hit[i], sizeof(float2));
                for (uint32_t f = 2; f < 4u; ++f) std::memcpy(o + 2u + 4u * f, &state[f * n + i], sizeof(float4));
                if (pool.medium) std::memcpy(o + 18, &medium[i], sizeof(uint4));
                if (pool.cone) std::memcpy(o + 22, &cone[i], sizeof(float2));
                for (uint32_t k = 0; k < kRecSlots; ++k) {
                    std::memcpy(o + 24u + k, &rec[(k * 4u + 1u) * n + i].w, sizeof(uint32_t));
                    std::memcpy(o + 32u + 3u * k, &rec[(k * 4u + 2u) * n + i], 3u * sizeof(float));
                }
                o[29] = flushItem[i];
            }
        };
        traceItems(*scene, *settings, 1u, sample, dPixels.ptr, slots, nullptr, nullptr,
                   [&](const float4* items) { HIP_CHECK(hipMemcpyAsync(out_items, items, n * sizeof(float4), hipMemcpyDeviceToHost, nullptr)); }, 2, &hook);
        *out_iterations = static_cast<uint32_t>(ran);
    });
}

int ptr_debug_env_mips(const float* rgba, uint32_t w, uint32_t h, float* out, uint64_t cap_floats, uint32_t* levels_out) {
    if (!rgba || w == 0u || h == 0u) return 1;
    try {
        const PtrTexture t{rgba, w, h, 0u, 0u, 1u, 0u};
        std::vector<float> chain;
        std::vector<uint32_t> info;
        appendTextureWithMips(t, chain, info);
        if (levels_out) *levels_out = info[2];
        if (!out) return 0;
        if (cap_floats < chain.size()) return 1;
        std::memcpy(out, chain.data(), chain.size() * sizeof(float));
        return 0;
    } catch (...) {
        return 1;
    }
}

int ptr_debug_camera_rays(const PtrSettings* settings, const uint32_t* xys, uint64_t n, float* out, uint32_t* out_states,
                          char* err, size_t err_cap) {
    return deviceCall("ptr_debug_camera_rays", nullptr, settings && ((xys && out && out_states) || !n), err, err_cap, [&] {
        RenderParams rp;
        fillRenderParams(*settings, 1, rp);
        DeviceBuffer<uint32_t> dxy, drng;
        DeviceBuffer<float> dout;
        dxy.upload(xys, n * 3);
        dout.ensure(n * 6);
        drng.ensure(n);
        launchDebugCameraRays(rp, dxy.ptr, n, dout.ptr, drng.ptr, nullptr);
        dout.download(out, n * 6);
        drng.download(out_states, n);
    });
}

}  // extern "C"
