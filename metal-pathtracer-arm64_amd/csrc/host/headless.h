// Headless backend plug-in boundary.  Same shape as the reference's
// include/headless/IHeadlessRenderer.h:17-52 (HeadlessScene / HeadlessCamera / HeadlessRenderOutput /
// IHeadlessRenderer::render) so that the CLI code path stays `renderer->render(...)`.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "ptr_adaptive.h"
#include "ptr_frame.h"
#include "ptr_post.h"
#include "ptr_stats.h"
#include "render_settings.h"
#include "scene_resources.h"

namespace ptr {

enum class HeadlessBackend { Hip = 0 };

// What the caller hands over: where the scene came from and the parsed CPU-side arrays (the HIP backend, like the
// reference's Embree backend, consumes `resources`; `source` / `isPath` are kept for messages).
struct HeadlessScene {
    const SceneResources* resources = nullptr;
    std::string source;
    bool isPath = false;
};

// Orbit camera as the CLI resolved it.  Passed for interface parity only: both reference backends rebuild the camera
// from the settings (quirk Q5), and so does this one.
struct HeadlessCamera {
    float3 target{0.0f, 0.0f, 0.0f};
    float distance = 0.0f, yaw = 0.0f, pitch = 0.0f;
    float verticalFov = 0.0f, defocusAngle = 0.0f, focusDistance = 0.0f;
};

// Result: linear RGB, width*height*3 floats, row 0 = top, mean over the samples; timing of the integrate phase.
struct HeadlessRenderOutput {
    uint32_t width = 0, height = 0, samples = 0;
    double totalSeconds = 0.0, avgMsPerSample = 0.0;
    std::vector<float> linearRGB;
};

// The plug-in interface: false + message on failure, no exceptions across it, called once from the main thread.
class IHeadlessRenderer {
public:
    virtual bool render(const HeadlessScene& scene, const HeadlessCamera& camera, const RenderSettings& settings,
                        uint32_t sppTotal, bool verbose, HeadlessRenderOutput& out, std::string& error) = 0;
    virtual ~IHeadlessRenderer() = default;
};

// What HipHeadlessRenderer::render decides before its first device call.
struct HeadlessPlan {
    // the call the frame comes from: ptr_render, ptr_render_multi, ptr_render_bands[_cov], ptr_render_adaptive, a PtrFrame
    enum class Frame { Whole, Multi, Bands, Adaptive, Snapshots };
    Frame frame = Frame::Whole;
    uint32_t spp = 1;
    bool features = false;     // the first-hit feature buffers: asked for, or the denoiser's guides
    bool covariance = false;   // the frame's per-pixel sample covariance: the denoiser's variance
    bool ownScene = false;     // render() uploads a scene of its own to device 0: for Bands, Adaptive, Snapshots and for the feature buffers
};

// MI355X backend: wraps the C-ABI (include/ptr_abi.h and the five headers beside it) behind the reference's interface.
class HipHeadlessRenderer : public IHeadlessRenderer {
public:
    // plan(), then in one line: the frame, the feature buffers (ptr_render_aovs, sample 0), the denoiser.  Anything thrown on the way
    // comes back as false with "exception: <what>".
    bool render(const HeadlessScene& scene, const HeadlessCamera& camera, const RenderSettings& settings,
                uint32_t sppTotal, bool verbose, HeadlessRenderOutput& out, std::string& error) override;
    // what render() would do with the setters' state as it is, or false and why it refuses; makes no device call
    bool plan(const HeadlessScene& scene, uint32_t sppTotal, HeadlessPlan& plan, std::string& error) const;
    const PtrRenderStats& lastStats() const { return m_stats; }
    // devices of this node to spread the frame over (1 = the first device only, 0 = all visible): --devices of the CLI
    void setDeviceCount(int n) { m_devices = n; }
    // also keep the first-hit feature buffers of the frame (albedo rgb | hit, shading normal * 0.5 + 0.5 | distance; width*height*4
    // floats each) - what the reference hands to its denoiser (shaders/pathtrace.metal:6424-6435, 9813-9815): --aovExr of the CLI
    void setCaptureAovs(bool on) { m_captureAovs = on; }
    const std::vector<float>& aovAlbedo() const { return m_aovAlbedo; }
    const std::vector<float>& aovNormal() const { return m_aovNormal; }
    // denoise the frame with the filter of include/ptr_post.h, guided by those feature buffers, on device 0 (after the gather of a
    // multi-device frame); null = off.  Its time goes to the verbose output, not into totalSeconds: --denoise of the CLI
    void setDenoise(const PtrDenoiseParams* params) {
        m_denoise = params != nullptr;
        if (params) m_denoiseParams = *params;
    }
    double lastDenoiseMs() const { return m_denoiseMs; }
    // where the denoiser's variance comes from: false = the filter's own 7x7 spatial estimate (include/ptr_post.h), true = the frame's
    // per-pixel sample covariance (include/ptr_stats.h; needs sppTotal >= 2 and one device): --denoiseVariance of the CLI
    void setDenoiseVariance(bool fromSamples) { m_denoiseFromSamples = fromSamples; }
    // render the frame adaptively (include/ptr_adaptive.h; one device): null = off.  maxSpp is taken from render()'s sppTotal:
    // --adaptive of the CLI
    void setAdaptive(const PtrAdaptiveParams* params) {
        m_adaptive = params != nullptr;
        if (params) m_adaptiveParams = *params;
    }
    // of the last adaptive frame: samples per pixel in image order, and the rounds it took
    const std::vector<uint32_t>& sampleCounts() const { return m_sampleCounts; }
    const PtrAdaptiveInfo& lastAdaptiveInfo() const { return m_adaptiveInfo; }

    // render the frame through a PtrFrame (include/ptr_frame.h; one device, not adaptive) and hand `sink` the raw resolved image - linear
    // RGB, width*height*3 floats - at each of `counts` samples per pixel on the way to sppTotal (strictly ascending, each below sppTotal);
    // a false return of the sink ends the render with its message.  Empty = off: --snapshots of the CLI
    using SnapshotSink = std::function<bool(uint32_t spp, uint32_t width, uint32_t height, const float* linearRGB, std::string& error)>;
    void setSnapshots(const std::vector<uint32_t>& counts, SnapshotSink sink) {
        m_snapshots = counts;
        m_snapshotSink = std::move(sink);
    }

private:
    std::vector<uint32_t> m_snapshots;
    SnapshotSink m_snapshotSink;
    PtrRenderStats m_stats{};
    int m_devices = 1;
    bool m_captureAovs = false;
    std::vector<float> m_aovAlbedo, m_aovNormal;
    bool m_denoise = false;
    PtrDenoiseParams m_denoiseParams{};
    double m_denoiseMs = 0.0;
    bool m_denoiseFromSamples = false;
    bool m_adaptive = false;
    PtrAdaptiveParams m_adaptiveParams{};
    PtrAdaptiveInfo m_adaptiveInfo{};
    std::vector<uint32_t> m_sampleCounts;
};

// RenderSettings -> POD settings of the C-ABI.
void FillPtrSettings(const RenderSettings& settings, PtrSettings& out);

}  // namespace ptr
