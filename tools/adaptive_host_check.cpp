// Host check of the index arithmetic of the adaptive kernels' per-element bodies (csrc/kernels/adaptive.h): the bodies are host + device
// functions, and this program drives them over every image size 1x1 .. 130x70 on heap buffers of exactly the size the renderer gives
// them, so that an address or undefined-behaviour sanitizer sees any step outside.  Build and run on the host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imetal-pathtracer-arm64_amd/csrc/kernels \
//       tools/adaptive_host_check.cpp -o /tmp/adaptive_host_check && /tmp/adaptive_host_check
// (The ranks of the compaction come from a wave ballot and exist on the device only; the tests compare its output with the restatement.)
#include <cstdio>
#include <memory>
#include <vector>

#include "adaptive.h"

int main() {
    unsigned long long kept = 0, visited = 0;
    for (uint32_t h = 1; h <= 70; ++h) {
        for (uint32_t w = 1; w <= 130; ++w) {
            const size_t pixels = static_cast<size_t>(w) * h;
            std::unique_ptr<float[]> sum(new float[pixels * 3]()), mean(new float[pixels * 3]()), m(new float[pixels * 6]()), e(new float[pixels]());
            std::unique_ptr<uint32_t[]> n(new uint32_t[pixels]());
            const ptrk::AdaptiveState st{sum.get(), mean.get(), m.get(), n.get(), e.get()};
            // the list in the renderer's order: 8-row bands, 8x8 blocks
            std::vector<uint32_t> list;
            for (uint32_t ty = 0; ty < h; ty += 8)
                for (uint32_t tx = 0; tx < w; tx += 8)
                    for (uint32_t y = ty; y < ty + 8 && y < h; ++y)
                        for (uint32_t x = tx; x < tx + 8 && x < w; ++x) list.push_back(y * w + x);
            if (list.size() != pixels) return 2;
            const uint32_t spp = 3;
            std::unique_ptr<float[]> items(new float[pixels * spp * 4]);
            for (size_t i = 0; i < pixels * spp * 4; ++i) items[i] = static_cast<float>((i * 2654435761u) % 1000u) * 1e-3f;
            for (size_t j = 0; j < pixels; ++j) {   // k_adaptive_update's body
                ptrk::AdaptivePixel p;
                p.load(st, list[j]);
                for (uint32_t c = 0; c < spp; ++c) {
                    const float* x = items.get() + (static_cast<size_t>(c) * pixels + j) * 4;
                    p.add(x[0], x[1], x[2], c + 1u);
                }
                p.store(st, list[j]);
                n[list[j]] = spp;
                e[list[j]] = p.error(spp);
            }
            for (size_t j = 0; j < pixels; ++j) {   // k_adaptive_select's body
                kept += ptrk::adaptiveKeep(list[j], w, h, e.get(), n.get(), 8u, 0.2f) ? 1u : 0u;
                ++visited;
            }
        }
    }
    std::printf("adaptive host check: %llu entries visited, %llu kept, no finding\n", visited, kept);
    return visited > 0 && kept > 0 && kept < visited ? 0 : 1;
}
