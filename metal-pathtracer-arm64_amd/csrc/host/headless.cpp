#include "headless.h"

#include <algorithm>
#include <cstdio>
#include <exception>
#include <memory>

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

namespace {

struct Release {
    void operator()(PtrDeviceScene* scene) const { ptr_scene_release(scene); }
    void operator()(PtrFrame* frame) const { ptr_frame_release(frame); }
};

}  // namespace

bool HipHeadlessRenderer::plan(const HeadlessScene& scene, uint32_t sppTotal, HeadlessPlan& p, std::string& error) const {
    using Frame = HeadlessPlan::Frame;
    p = HeadlessPlan{};
    p.spp = std::max<uint32_t>(1u, sppTotal);
    p.features = m_captureAovs || m_denoise;   // the denoiser's guides are the feature buffers
    p.covariance = m_denoise && m_denoiseFromSamples;
    p.frame = m_adaptive ? Frame::Adaptive : !m_snapshots.empty() ? Frame::Snapshots : m_devices != 1 ? Frame::Multi : p.features ? Frame::Bands : Frame::Whole;
    p.ownScene = p.features || p.frame == Frame::Adaptive || p.frame == Frame::Snapshots;
    const char* refusal = nullptr;
    if (!scene.resources) {
        refusal = "HIP backend requires scene resources";
    } else if (p.covariance && m_devices != 1) {
        refusal = "the denoiser's sample variance needs a frame rendered on one device (--devices=1)";
    } else if (p.covariance && p.spp < 2u) {
        refusal = "the denoiser's sample variance needs at least 2 samples per pixel";
    } else if (p.frame == Frame::Adaptive && m_devices != 1) {
        refusal = "an adaptive frame is rendered on one device (--devices=1)";
    } else if (p.frame == Frame::Snapshots && m_devices != 1) {
        refusal = "snapshots are taken of a frame rendered on one device (--devices=1)";
    } else if (p.frame == Frame::Snapshots) {
        uint32_t done = 0u;
        for (const uint32_t stop : m_snapshots) {
            if (stop <= done || stop >= p.spp) refusal = "snapshot counts must ascend and stay below the frame's samples per pixel";
            done = stop;
        }
    }
    if (refusal) error = refusal;
    return !refusal;
}

bool HipHeadlessRenderer::render(const HeadlessScene& scene, const HeadlessCamera&, const RenderSettings& settings,
                                 uint32_t sppTotal, bool verbose, HeadlessRenderOutput& out, std::string& error) try {
    using Frame = HeadlessPlan::Frame;
    m_stats = PtrRenderStats{};
    m_aovAlbedo.clear();
    m_aovNormal.clear();
    m_denoiseMs = 0.0;
    m_sampleCounts.clear();
    m_adaptiveInfo = PtrAdaptiveInfo{};
    HeadlessPlan p;
    if (!plan(scene, sppTotal, p, error)) return false;

    PtrSceneDesc desc;
    scene.resources->fillSceneDesc(desc);
    PtrSettings ps;
    FillPtrSettings(settings, ps);
    const size_t pixels = static_cast<size_t>(ps.width) * ps.height;
    out.linearRGB.assign(pixels * 3u, 0.0f);
    float* const rgb = out.linearRGB.data();
    std::vector<float> cov;
    char err[512] = {0};
    const auto fail = [&](const char* fallback) {
        error = err[0] ? err : fallback;
        return false;
    };

    // a frame step in two halves.  These two kinds upload for themselves (several devices: interleaved bands, gathered on the first one), so
    // they are over before device 0 gets this function's scene; the other three are rendered on it
    if (p.frame == Frame::Whole || p.frame == Frame::Multi) {
        const int rc = p.frame == Frame::Whole ? ptr_render(&desc, &ps, p.spp, verbose ? 1 : 0, rgb, &m_stats, err, sizeof(err))
                                               : ptr_render_multi(&desc, &ps, p.spp, m_devices, verbose ? 1 : 0, rgb, &m_stats, err, sizeof(err));
        if (rc != 0) return fail("HIP render failed");
    }

    // one upload serves the frame, its snapshots and, where asked for, the first-hit feature buffers
    std::unique_ptr<PtrDeviceScene, Release> ds;
    if (p.ownScene) {
        PtrDeviceScene* uploaded = nullptr;
        if (ptr_scene_upload(&desc, 0, &uploaded, err, sizeof(err)) != 0) return fail("HIP scene upload failed");
        ds.reset(uploaded);
    }

    switch (p.frame) {
    default:
        break;   // Whole, Multi: rendered above
    case Frame::Bands: {
        const uint32_t bands = ptr_part_band_count(ps.height, 0, 1);
        std::vector<float> banded(static_cast<size_t>(bands) * PTR_BAND_ROWS * ps.width * 3u);
        if (p.covariance) cov.resize(banded.size() * 2u);   // one partition: its bands are the image's rows in order, then padding
        const int rc = p.covariance ? ptr_render_bands_cov(ds.get(), &ps, p.spp, 0, 1, banded.data(), cov.data(), 0, &m_stats, err, sizeof(err))
                                    : ptr_render_bands(ds.get(), &ps, p.spp, 0, 1, banded.data(), 0, &m_stats, err, sizeof(err));
        if (rc != 0) return fail("HIP render failed");
        std::copy(banded.begin(), banded.begin() + static_cast<std::ptrdiff_t>(out.linearRGB.size()), out.linearRGB.begin());
        break;
    }
    case Frame::Adaptive: {
        PtrAdaptiveParams ap = m_adaptiveParams;
        ap.maxSpp = p.spp;
        m_sampleCounts.assign(pixels, 0u);
        if (p.covariance) cov.resize(pixels * 6u);   // already the covariance of each pixel's mean: unequal counts need no special case
        if (ptr_render_adaptive(ds.get(), &ps, &ap, rgb, p.covariance ? cov.data() : nullptr, m_sampleCounts.data(), &m_stats, &m_adaptiveInfo, err,
                                sizeof(err)) != 0) {
            return fail("HIP render failed");
        }
        break;
    }
    case Frame::Snapshots: {
        // the frame's state leaves the device at the end of this block: before the feature pass, and before the scene
        PtrFrame* created = nullptr;
        if (ptr_frame_create(ds.get(), &ps, &created, err, sizeof(err)) != 0) return fail("HIP render failed");
        const std::unique_ptr<PtrFrame, Release> frame(created);
        std::vector<uint32_t> stops = m_snapshots;
        stops.push_back(p.spp);
        uint32_t done = 0u;
        for (const uint32_t stop : stops) {
            PtrRenderStats one{};
            if (ptr_frame_accumulate(frame.get(), stop - done, nullptr, &one, err, sizeof(err)) != 0) return fail("HIP render failed");
            done = stop;
            m_stats.totalSeconds += one.totalSeconds;   // the other fields of the stats stay zero
            m_stats.samples += one.samples;
            m_stats.avgMsPerSample = m_stats.totalSeconds * 1000.0 / p.spp;
            const bool last = done == p.spp;
            if (last && p.covariance) cov.resize(pixels * 6u);
            if (ptr_frame_resolve(frame.get(), rgb, last && p.covariance ? cov.data() : nullptr, nullptr, err, sizeof(err)) != 0) return fail("HIP render failed");
            if (last) break;
            std::string sinkError;
            if (m_snapshotSink && !m_snapshotSink(done, ps.width, ps.height, rgb, sinkError)) {
                std::snprintf(err, sizeof(err), "%s", sinkError.c_str());
                return fail("HIP render failed");
            }
            if (verbose) std::fprintf(stderr, "snapshot: %u spp after %.3f s\n", done, m_stats.totalSeconds);
        }
        break;
    }
    }

    if (p.features) {
        m_aovAlbedo.assign(pixels * 4u, 0.0f);
        m_aovNormal.assign(pixels * 4u, 0.0f);
        if (ptr_render_aovs(ds.get(), &ps, 0u, m_aovAlbedo.data(), m_aovNormal.data(), err, sizeof(err)) != 0) return fail("HIP render failed");
    }
    ds.reset();   // the denoiser gets device 0 without the scene on it
    if (p.frame == Frame::Adaptive && verbose) {   // only of a frame whose feature pass went through too
        std::fprintf(stderr, "adaptive: %u rounds, %.2f samples per pixel on average, %u pixels at %u spp\n", m_adaptiveInfo.rounds,
                     static_cast<double>(m_adaptiveInfo.totalSamples) / static_cast<double>(pixels), m_adaptiveInfo.pixelsAtMax, p.spp);
    }

    if (m_denoise) {
        const int rc = p.covariance ? ptr_denoise_cov(rgb, m_aovAlbedo.data(), m_aovNormal.data(), cov.data(), ps.width, ps.height, &m_denoiseParams, 0, rgb,
                                                      &m_denoiseMs, err, sizeof(err))
                                    : ptr_denoise(rgb, m_aovAlbedo.data(), m_aovNormal.data(), ps.width, ps.height, &m_denoiseParams, 0, rgb, &m_denoiseMs, err,
                                                  sizeof(err));
        if (rc != 0) return fail("HIP denoise failed");
        if (verbose) {
            std::fprintf(stderr, "denoise: %u a-trous passes, %.3f ms on device 0\n", m_denoiseParams.iterations, m_denoiseMs);
            std::fprintf(stderr, "denoise: variance from %s\n", p.covariance ? "the per-pixel sample covariance" : "the 7x7 spatial estimate");
        }
    }
    out.width = ps.width;
    out.height = ps.height;
    out.samples = p.spp;
    out.totalSeconds = m_stats.totalSeconds;
    out.avgMsPerSample = m_stats.avgMsPerSample;
    return true;
} catch (const std::exception& e) {
    error = std::string("exception: ") + e.what();
    return false;
}

}  // namespace ptr
