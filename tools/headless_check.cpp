// Host check of HipHeadlessRenderer::render (csrc/host/headless.cpp), for a machine without a device.  It loads a scene through
// SceneManager and asserts (1) that every refusal of the plan - null resources, sample variance on two devices or at 1 spp, an adaptive
// frame or snapshots on two devices, snapshot lists {8,4} and {4,16} at 16 spp - returns false with exactly its message and without a
// device call, and (2) where ptr_device_count() is 0, that each of the five frame kinds, alone, with feature buffers, with the denoiser
// and with its sample variance, returns false with the device check's "no CPU fallback": every early exit of render()'s owners.
// tests/test_headless_host.py builds it against the library and runs it:
//   g++ -std=c++17 -O1 -g -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host tools/headless_check.cpp -Lmetal-pathtracer-arm64_amd -lptr_hip \
//       -Wl,-rpath,$PWD/metal-pathtracer-arm64_amd -o /tmp/headless_check && /tmp/headless_check tests/golden/smoke.scene
// By hand, with headless.cpp compiled into the program under the address and undefined-behaviour sanitizers (its copy of render() is
// the one that runs; the rest comes from the library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host \
//       tools/headless_check.cpp metal-pathtracer-arm64_amd/csrc/host/headless.cpp -Lmetal-pathtracer-arm64_amd -lptr_hip \
//       -Wl,-rpath,$PWD/metal-pathtracer-arm64_amd -o /tmp/headless_check_asan && /tmp/headless_check_asan tests/golden/smoke.scene
#include <cstdio>
#include <string>
#include <vector>

#include "headless.h"
#include "ptr_abi.h"
#include "scene_manager.h"

namespace {

struct Mode {
    int devices = 1;
    bool adaptive = false, aovs = false, denoise = false, sampleVariance = false;
    std::vector<uint32_t> snapshots;
};

int findings = 0;

// One render() of `mode`; it must return false.  `exact`: the whole message; otherwise the message must contain `part`.
void expectFailure(const char* name, const ptr::HeadlessScene& scene, const ptr::RenderSettings& settings, const Mode& mode, uint32_t spp,
                   const std::string& exact, const char* part) {
    ptr::HipHeadlessRenderer renderer;
    renderer.setDeviceCount(mode.devices);
    renderer.setCaptureAovs(mode.aovs);
    PtrDenoiseParams dp;
    ptr_denoise_default_params(&dp);
    if (mode.denoise) renderer.setDenoise(&dp);
    renderer.setDenoiseVariance(mode.sampleVariance);
    PtrAdaptiveParams ap;
    ptr_adaptive_default_params(&ap, spp);
    if (mode.adaptive) renderer.setAdaptive(&ap);
    unsigned sunk = 0;
    renderer.setSnapshots(mode.snapshots, [&](uint32_t, uint32_t, uint32_t, const float*, std::string&) {
        ++sunk;
        return true;
    });
    ptr::HeadlessRenderOutput out;
    std::string error;
    const bool ok = renderer.render(scene, ptr::HeadlessCamera{}, settings, spp, false, out, error);
    // "HIP" is in every message of a device call; of the refusals only the null-resources text has the word itself
    const bool good = !ok && sunk == 0u && (part ? error.find(part) != std::string::npos : error == exact) &&
                      (part || !scene.resources || error.find("HIP") == std::string::npos);
    std::printf("%s %s: %s\n", good ? "ok     " : "FINDING", name, ok ? "(rendered)" : error.c_str());
    findings += good ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <path to a .scene file>\n", argv[0]);
        return 2;
    }
    ptr::SceneManager manager;
    ptr::SceneResources resources;
    ptr::RenderSettings settings{};
    std::string error;
    if (!manager.loadSceneFromPath(argv[1], resources, settings, &error)) {
        std::fprintf(stderr, "cannot load %s: %s\n", argv[1], error.c_str());
        return 2;
    }
    settings.renderWidth = 64;
    settings.renderHeight = 48;
    ptr::HeadlessScene scene;
    scene.resources = &resources;
    scene.source = argv[1];
    scene.isPath = true;

    // (1) the refusals
    const auto mode = [](int devices, bool adaptive, std::vector<uint32_t> snapshots, bool sampleVariance) {
        Mode m;
        m.devices = devices;
        m.adaptive = adaptive;
        m.snapshots = std::move(snapshots);
        m.denoise = m.sampleVariance = sampleVariance;
        return m;
    };
    const std::string ascend = "snapshot counts must ascend and stay below the frame's samples per pixel";
    expectFailure("refusal-null-resources", ptr::HeadlessScene{}, settings, Mode{}, 16, "HIP backend requires scene resources", nullptr);
    expectFailure("refusal-variance-two-devices", scene, settings, mode(2, false, {}, true), 16,
                  "the denoiser's sample variance needs a frame rendered on one device (--devices=1)", nullptr);
    expectFailure("refusal-variance-1spp", scene, settings, mode(1, false, {}, true), 1, "the denoiser's sample variance needs at least 2 samples per pixel",
                  nullptr);
    expectFailure("refusal-adaptive-two-devices", scene, settings, mode(2, true, {}, false), 16, "an adaptive frame is rendered on one device (--devices=1)",
                  nullptr);
    expectFailure("refusal-snapshots-two-devices", scene, settings, mode(2, false, {4, 8}, false), 16,
                  "snapshots are taken of a frame rendered on one device (--devices=1)", nullptr);
    expectFailure("refusal-snapshots-8-4", scene, settings, mode(1, false, {8, 4}, false), 16, ascend, nullptr);
    expectFailure("refusal-snapshots-4-16", scene, settings, mode(1, false, {4, 16}, false), 16, ascend, nullptr);

    // (2) without a device: every kind as far as its first device call
    if (ptr_device_count() == 0) {
        const struct {
            const char* name;
            int devices;
            bool adaptive;
            std::vector<uint32_t> snapshots;
        } kinds[] = {{"whole", 1, false, {}}, {"multi", 2, false, {}}, {"adaptive", 1, true, {}}, {"snapshots", 1, false, {4, 8}}};
        for (const auto& kind : kinds) {
            for (int with = 0; with < 4; ++with) {   // alone, feature buffers, denoiser, denoiser on the sample variance
                if (with == 3 && kind.devices != 1) continue;
                Mode m = mode(kind.devices, kind.adaptive, kind.snapshots, with == 3);
                m.aovs = with == 1;
                m.denoise = with >= 2;
                const char* const names[] = {"", "+features", "+denoise", "+denoise-sample"};
                const std::string frame = kind.devices == 1 && !kind.adaptive && kind.snapshots.empty() && with > 0 ? "bands" : kind.name;
                expectFailure(("no-device-" + frame + names[with]).c_str(), scene, settings, m, 16, "", "no CPU fallback");
            }
        }
    } else {
        std::printf("a device is present: the frame kinds are left to the GPU tests\n");
    }
    std::printf("%d finding(s) in all\n", findings);
    return findings ? 1 : 0;
}
