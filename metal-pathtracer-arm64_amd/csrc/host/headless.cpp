#include "headless.h"

#include <algorithm>
#include <cstdio>

namespace ptr {

void FillPtrSettings(const RenderSettings& s, PtrSettings& o) {
    o = PtrSettings{};
    o.width = s.renderWidth > 0 ? s.renderWidth : 1280u;   // EmbreeHeadlessRenderer.mm:2462-2463
    o.height = s.renderHeight > 0 ? s.renderHeight : 720u;
    o.maxDepth = s.maxDepth;
    o.seed = s.fixedRngSeed;
    o.enableRussianRoulette = s.enableRussianRoulette ? 1u : 0u;
    o.enableSpecularNee = s.enableSpecularNee ? 1u : 0u;
    o.enableMnee = s.enableMnee ? 1u : 0u;
    o.enableMneeSecondary = s.enableMneeSecondary ? 1u : 0u;
    o.cameraTarget[0] = s.cameraTarget.x;
    o.cameraTarget[1] = s.cameraTarget.y;
    o.cameraTarget[2] = s.cameraTarget.z;
    o.cameraDistance = s.cameraDistance;
    o.cameraYaw = s.cameraYaw;
    o.cameraPitch = s.cameraPitch;
    o.cameraVerticalFov = s.cameraVerticalFov;
    o.cameraDefocusAngle = s.cameraDefocusAngle;
    o.cameraFocusDistance = s.cameraFocusDistance;
    o.backgroundMode = static_cast<uint32_t>(s.backgroundMode);
    o.backgroundColor[0] = s.backgroundColor.x;
    o.backgroundColor[1] = s.backgroundColor.y;
    o.backgroundColor[2] = s.backgroundColor.z;
    o.environmentRotation = s.environmentRotation;
    o.environmentIntensity = s.environmentIntensity;
    o.fireflyClampEnabled = s.fireflyClampEnabled ? 1u : 0u;
    o.fireflyClampFactor = s.fireflyClampFactor;
    o.fireflyClampFloor = s.fireflyClampFloor;
    o.throughputClamp = s.throughputClamp;
    o.specularTailClampBase = s.specularTailClampBase;
    o.specularTailClampRoughnessScale = s.specularTailClampRoughnessScale;
    o.minSpecularPdf = s.minSpecularPdf;
    o.fireflyClampMaxContribution = s.fireflyClampMaxContribution;
    o.emissionScale = 1.0f;
    o.metalSemantics = s.metalSemantics;
    o.sssMode = static_cast<uint32_t>(s.sssMode);
    o.sssMaxSteps = s.sssMaxSteps;
    o.debugShadowSlack = 0.0f;
}

bool HipHeadlessRenderer::render(const HeadlessScene& scene, const HeadlessCamera&, const RenderSettings& settings,
                                 uint32_t sppTotal, bool verbose, HeadlessRenderOutput& out, std::string& error) {
    if (!scene.resources) {
        error = "HIP backend requires scene resources";
        return false;
    }
    PtrSceneDesc desc;
    scene.resources->fillSceneDesc(desc);
    PtrSettings ps;
    FillPtrSettings(settings, ps);

    const uint32_t spp = std::max<uint32_t>(1u, sppTotal);
    out.linearRGB.assign(static_cast<size_t>(ps.width) * ps.height * 3u, 0.0f);
    char err[512] = {0};
    m_stats = PtrRenderStats{};
    m_aovAlbedo.clear();
    m_aovNormal.clear();
    m_denoiseMs = 0.0;
    const bool captureAovs = m_captureAovs || m_denoise;   // the denoiser's guides are the feature buffers
    const bool sampleVariance = m_denoise && m_denoiseFromSamples;
    if (sampleVariance && (m_devices != 1 || spp < 2u)) {
        error = m_devices != 1 ? "the denoiser's sample variance needs a frame rendered on one device (--devices=1)"
                               : "the denoiser's sample variance needs at least 2 samples per pixel";
        return false;
    }
    std::vector<float> cov;
    m_sampleCounts.clear();
    m_adaptiveInfo = PtrAdaptiveInfo{};
    if (m_adaptive) {
        if (m_devices != 1) {
            error = "an adaptive frame is rendered on one device (--devices=1)";
            return false;
        }
        // one upload serves the frame and, where asked for, the first-hit feature buffers
        PtrAdaptiveParams ap = m_adaptiveParams;
        ap.maxSpp = spp;
        PtrDeviceScene* ds = nullptr;
        if (ptr_scene_upload(&desc, 0, &ds, err, sizeof(err)) != 0) {
            error = err[0] ? err : "HIP scene upload failed";
            return false;
        }
        const size_t pixels = static_cast<size_t>(ps.width) * ps.height;
        m_sampleCounts.assign(pixels, 0u);
        if (sampleVariance) cov.resize(pixels * 6u);   // already the covariance of each pixel's mean: unequal counts need no special case
        bool ok = ptr_render_adaptive(ds, &ps, &ap, out.linearRGB.data(), sampleVariance ? cov.data() : nullptr, m_sampleCounts.data(), &m_stats,
                                      &m_adaptiveInfo, err, sizeof(err)) == 0;
        if (ok && captureAovs) {
            m_aovAlbedo.assign(pixels * 4u, 0.0f);
            m_aovNormal.assign(pixels * 4u, 0.0f);
            ok = ptr_render_aovs(ds, &ps, 0u, m_aovAlbedo.data(), m_aovNormal.data(), err, sizeof(err)) == 0;
        }
        ptr_scene_release(ds);
        if (!ok) {
            error = err[0] ? err : "HIP render failed";
            return false;
        }
        if (verbose) {
            std::fprintf(stderr, "adaptive: %u rounds, %.2f samples per pixel on average, %u pixels at %u spp\n", m_adaptiveInfo.rounds,
                         static_cast<double>(m_adaptiveInfo.totalSamples) / static_cast<double>(pixels), m_adaptiveInfo.pixelsAtMax, spp);
        }
    } else if (!m_snapshots.empty()) {
        if (m_devices != 1) {
            error = "snapshots are taken of a frame rendered on one device (--devices=1)";
            return false;
        }
        // one upload serves the frame, its snapshots and, where asked for, the first-hit feature buffers
        PtrDeviceScene* ds = nullptr;
        if (ptr_scene_upload(&desc, 0, &ds, err, sizeof(err)) != 0) {
            error = err[0] ? err : "HIP scene upload failed";
            return false;
        }
        const size_t pixels = static_cast<size_t>(ps.width) * ps.height;
        PtrFrame* frame = nullptr;
        bool ok = ptr_frame_create(ds, &ps, &frame, err, sizeof(err)) == 0;
        std::vector<uint32_t> stops = m_snapshots;
        stops.push_back(spp);
        uint32_t done = 0u;
        for (size_t i = 0; ok && i < stops.size(); ++i) {
            if (stops[i] <= done) {
                std::snprintf(err, sizeof(err), "snapshot counts must ascend and stay below the frame's samples per pixel");
                ok = false;
                break;
            }
            PtrRenderStats one{};
            ok = ptr_frame_accumulate(frame, stops[i] - done, nullptr, &one, err, sizeof(err)) == 0;
            if (!ok) break;
            done = stops[i];
            m_stats.totalSeconds += one.totalSeconds;
            m_stats.samples += one.samples;
            const bool last = i + 1u == stops.size();
            if (last && sampleVariance) cov.resize(pixels * 6u);
            ok = ptr_frame_resolve(frame, out.linearRGB.data(), last && sampleVariance ? cov.data() : nullptr, nullptr, err, sizeof(err)) == 0;
            if (ok && !last) {
                std::string sinkError;
                if (m_snapshotSink && !m_snapshotSink(done, ps.width, ps.height, out.linearRGB.data(), sinkError)) {
                    std::snprintf(err, sizeof(err), "%s", sinkError.c_str());
                    ok = false;
                }
                if (ok && verbose) std::fprintf(stderr, "snapshot: %u spp after %.3f s\n", done, m_stats.totalSeconds);
            }
        }
        m_stats.avgMsPerSample = m_stats.totalSeconds * 1000.0 / spp;
        ptr_frame_release(frame);
        if (ok && captureAovs) {
            m_aovAlbedo.assign(pixels * 4u, 0.0f);
            m_aovNormal.assign(pixels * 4u, 0.0f);
            ok = ptr_render_aovs(ds, &ps, 0u, m_aovAlbedo.data(), m_aovNormal.data(), err, sizeof(err)) == 0;
        }
        ptr_scene_release(ds);
        if (!ok) {
            error = err[0] ? err : "HIP render failed";
            return false;
        }
    } else if (m_devices != 1) {
        // the frame in interleaved bands over several devices of the node, gathered on the first one
        if (ptr_render_multi(&desc, &ps, spp, m_devices, verbose ? 1 : 0, out.linearRGB.data(), &m_stats, err, sizeof(err)) != 0) {
            error = err[0] ? err : "HIP render failed";
            return false;
        }
    } else if (!captureAovs) {
        if (ptr_render(&desc, &ps, spp, verbose ? 1 : 0, out.linearRGB.data(), &m_stats, err, sizeof(err)) != 0) {
            error = err[0] ? err : "HIP render failed";
            return false;
        }
    }
    if (captureAovs && !m_adaptive && m_snapshots.empty()) {
        // one upload serves the frame (single device) and the first-hit feature buffers
        PtrDeviceScene* ds = nullptr;
        if (ptr_scene_upload(&desc, 0, &ds, err, sizeof(err)) != 0) {
            error = err[0] ? err : "HIP scene upload failed";
            return false;
        }
        bool ok = true;
        if (m_devices == 1) {
            const uint32_t bands = ptr_part_band_count(ps.height, 0, 1);
            std::vector<float> banded(static_cast<size_t>(bands) * PTR_BAND_ROWS * ps.width * 3u);
            if (sampleVariance) {
                cov.resize(banded.size() * 2u);   // one partition: its bands are the image's rows in order, then padding
                ok = ptr_render_bands_cov(ds, &ps, spp, 0, 1, banded.data(), cov.data(), 0, &m_stats, err, sizeof(err)) == 0;
            } else {
                ok = ptr_render_bands(ds, &ps, spp, 0, 1, banded.data(), 0, &m_stats, err, sizeof(err)) == 0;
            }
            if (ok) std::copy(banded.begin(), banded.begin() + static_cast<std::ptrdiff_t>(out.linearRGB.size()), out.linearRGB.begin());
        }
        if (ok) {
            m_aovAlbedo.assign(static_cast<size_t>(ps.width) * ps.height * 4u, 0.0f);
            m_aovNormal.assign(static_cast<size_t>(ps.width) * ps.height * 4u, 0.0f);
            ok = ptr_render_aovs(ds, &ps, 0u, m_aovAlbedo.data(), m_aovNormal.data(), err, sizeof(err)) == 0;
        }
        ptr_scene_release(ds);
        if (!ok) {
            error = err[0] ? err : "HIP render failed";
            return false;
        }
    }
    if (m_denoise) {
        const int rc = sampleVariance ? ptr_denoise_cov(out.linearRGB.data(), m_aovAlbedo.data(), m_aovNormal.data(), cov.data(), ps.width, ps.height,
                                                        &m_denoiseParams, 0, out.linearRGB.data(), &m_denoiseMs, err, sizeof(err))
                                      : ptr_denoise(out.linearRGB.data(), m_aovAlbedo.data(), m_aovNormal.data(), ps.width, ps.height, &m_denoiseParams,
                                                    0, out.linearRGB.data(), &m_denoiseMs, err, sizeof(err));
        if (rc != 0) {
            error = err[0] ? err : "HIP denoise failed";
            return false;
        }
        if (verbose) {
            std::fprintf(stderr, "denoise: %u a-trous passes, %.3f ms on device 0\n", m_denoiseParams.iterations, m_denoiseMs);
            std::fprintf(stderr, "denoise: variance from %s\n", sampleVariance ? "the per-pixel sample covariance" : "the 7x7 spatial estimate");
        }
    }
    out.width = ps.width;
    out.height = ps.height;
    out.samples = spp;
    out.totalSeconds = m_stats.totalSeconds;
    out.avgMsPerSample = m_stats.avgMsPerSample;
    return true;
}

}  // namespace ptr
