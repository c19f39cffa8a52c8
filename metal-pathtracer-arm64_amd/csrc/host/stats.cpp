// Host side of include/ptr_stats.h's render entry points: argument checks, the covariance buffer beside the image, and the test-only
// download of a frame's per-sample accumulators.  (ptr_denoise_cov* live with the rest of the denoiser in denoise.cpp.)
#include <string>
#include <vector>

#include "device_scene.h"
#include "ptr_stats.h"

using namespace ptrhost;

namespace {

// "<who>: ..." for a bad argument, empty when all are good.  No device call.
std::string badArgument(const char* who, bool pointersOk, const PtrSettings* settings, uint32_t spp, uint32_t part, uint32_t parts) {
    const std::string w(who);
    if (!pointersOk) return w + ": null argument";
    if (spp < 2u) return w + ": a sample covariance needs spp >= 2";
    if (parts == 0u || part >= parts) return w + ": bad partition";
    if (settings->width == 0u || settings->height == 0u) return w + ": render size must be non-zero";
    return std::string();
}

size_t bandPixels(const PtrSettings& s, uint32_t part, uint32_t parts) {
    return static_cast<size_t>(ptr_part_band_count(s.height, part, parts)) * PTR_BAND_ROWS * s.width;
}

}  // namespace

extern "C" {

int ptr_render_bands_cov_device(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index,
                                uint32_t part_count, void* d_out_rgb, void* d_out_cov, void* stream, int count_traversal,
                                PtrRenderStats* stats, char* err, size_t err_cap) {
    const std::string bad = badArgument("ptr_render_bands_cov_device", scene && settings && d_out_rgb && d_out_cov, settings, spp, part_index, part_count);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    try {
        renderBands(*scene, *settings, spp, part_index, part_count, static_cast<float*>(d_out_rgb), static_cast<hipStream_t>(stream),
                    count_traversal, stats, static_cast<float*>(d_out_cov));
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_render_bands_cov(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, uint32_t part_index, uint32_t part_count,
                         float* out_rgb_bands, float* out_cov_bands, int count_traversal, PtrRenderStats* stats, char* err,
                         size_t err_cap) {
    const std::string bad = badArgument("ptr_render_bands_cov", scene && settings && out_rgb_bands && out_cov_bands, settings, spp, part_index, part_count);
    if (!bad.empty()) {
        setErr(err, err_cap, bad);
        return 1;
    }
    try {
        const size_t pixels = bandPixels(*settings, part_index, part_count);
        HIP_CHECK(hipSetDevice(scene->device));
        scene->outBands.ensure(pixels * 3u);
        scene->covBands.ensure(pixels * 6u);
        renderBands(*scene, *settings, spp, part_index, part_count, scene->outBands.ptr, nullptr, count_traversal, stats, scene->covBands.ptr);
        scene->outBands.download(out_rgb_bands, pixels * 3u);
        scene->covBands.download(out_cov_bands, pixels * 6u);
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

int ptr_stats_debug_samples(PtrDeviceScene* scene, const PtrSettings* settings, uint32_t spp, float* out_samples, char* err, size_t err_cap) {
    if (scene && settings && out_samples && (spp < 1u || settings->width == 0u || settings->height == 0u)) {
        setErr(err, err_cap, "ptr_stats_debug_samples: spp and the render size must be non-zero");
        return 1;
    }
    return deviceCall("ptr_stats_debug_samples", scene, scene && settings && out_samples, err, err_cap, [&] {
        if (framePasses(*scene, *settings, spp) > 1u) throw HipError{"ptr_stats_debug_samples: the frame needs more than one pass"};
        const size_t pixels = static_cast<size_t>(settings->width) * settings->height;
        scene->outBands.ensure(bandPixels(*settings, 0u, 1u) * 3u);
        // (mode 4: every pixel through the pool - the accumulators read below are the per-sample values of the whole image)
        renderBands(*scene, *settings, spp, 0u, 1u, scene->outBands.ptr, nullptr, 4, nullptr);
        std::vector<float4> items(pixels * spp);
        std::vector<uint32_t> pixelOfLocal(pixels);
        scene->itemAccum.download(items.data(), items.size());
        scene->pixelOfLocal.download(pixelOfLocal.data(), pixels);
        for (uint32_t c = 0; c < spp; ++c) {
            for (size_t lp = 0; lp < pixels; ++lp) {
                const float4& a = items[c * pixels + lp];
                float* o = out_samples + (c * pixels + pixelOfLocal[lp]) * 3u;
                o[0] = a.x;
                o[1] = a.y;
                o[2] = a.z;
            }
        }
    });
}

}  // extern "C"
