// Host check of the index arithmetic of the multi-device kernels' per-element bodies (csrc/kernels/multi.h): pack, the host's collection of
// the neighbour rows, unpack, finish-bands and interleave, over every image size 1x1 .. 130x70 with P = 1, 2, 3 and the number of bands,
// on heap buffers of exactly the size the renderer gives them, so that an address or undefined-behaviour sanitizer sees any step outside.
// Build and run on the host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imetal-pathtracer-arm64_amd/csrc/kernels \
//       tools/multi_host_check.cpp -o /tmp/multi_host_check && /tmp/multi_host_check
// Checked besides the addresses: pack -> collect -> unpack puts exactly the rows above and below a partition's bands, with the owners'
// values, into its e image and touches nothing else; every image row is written by exactly one partition's finish; the interleaved
// images of 3, 6 and 1 words per pixel are the single-device outputs, and so is the rgb image of the plain frame's rgb-only layout.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "multi.h"

namespace {

uint32_t bandCount(uint32_t height, uint32_t part, uint32_t parts) {   // ptr_part_band_count
    const uint32_t bands = (height + 7u) / 8u;
    return bands > part ? (bands - part + parts - 1u) / parts : 0u;
}

unsigned long long checked = 0;

int checkSize(uint32_t w, uint32_t h, uint32_t parts) {
    const size_t pixels = static_cast<size_t>(w) * h;
    const uint32_t totalBands = (h + 7u) / 8u;
    // the true state of the image: every pixel's e is its index + 1
    std::unique_ptr<float[]> truth(new float[pixels]), sum(new float[pixels * 3]), m(new float[pixels * 6]), mean(new float[pixels * 3]());
    std::unique_ptr<uint32_t[]> n(new uint32_t[pixels]);
    for (size_t p = 0; p < pixels; ++p) {
        truth[p] = static_cast<float>(p + 1u);
        n[p] = 2u + static_cast<uint32_t>(p % 5u);
        for (int c = 0; c < 3; ++c) sum[p * 3 + c] = static_cast<float>((p * 3 + c) % 97u) * 0.25f;
        for (int c = 0; c < 6; ++c) m[p * 6 + c] = static_cast<float>((p * 6 + c) % 89u) * 0.5f;
    }
    std::vector<size_t> offset(parts + 1u, 0u);
    std::vector<uint64_t> partPixel(parts + 1u, 0u);
    for (uint32_t p = 0; p < parts; ++p) {
        offset[p + 1u] = offset[p] + static_cast<size_t>(bandCount(h, p, parts)) * 2u * w;
        partPixel[p + 1u] = partPixel[p] + static_cast<uint64_t>(bandCount(h, p, parts)) * 8u * w;
    }
    // ---- pack: every partition publishes from an e image that is right on its own rows and -1 elsewhere
    std::unique_ptr<float[]> outboxes(new float[offset[parts]]);
    std::vector<std::unique_ptr<float[]>> eOf(parts);
    for (uint32_t p = 0; p < parts; ++p) {
        const ptrk::MultiPart mp{p, parts, bandCount(h, p, parts), w, h};
        eOf[p].reset(new float[pixels]);
        for (uint32_t y = 0; y < h; ++y) {
            for (uint32_t x = 0; x < w; ++x) eOf[p][static_cast<size_t>(y) * w + x] = (y / 8u) % parts == p ? truth[static_cast<size_t>(y) * w + x] : -1.0f;
        }
        std::unique_ptr<float[]> edge(new float[static_cast<size_t>(mp.bands) * 2u * w]);
        for (uint32_t i = 0; i < mp.bands * 2u * w; ++i) ptrk::multiHaloPack(mp, i, eOf[p].get(), edge.get());
        std::memcpy(outboxes.get() + offset[p], edge.get(), static_cast<size_t>(mp.bands) * 2u * w * sizeof(float));
    }
    // ---- collect and unpack: the rows next to the own bands become right, everything else stays as it was
    for (uint32_t p = 0; p < parts && parts > 1u; ++p) {
        const ptrk::MultiPart mp{p, parts, bandCount(h, p, parts), w, h};
        const size_t floats = static_cast<size_t>(mp.bands) * 2u * w;
        std::unique_ptr<float[]> inbox(new float[floats]);
        for (size_t i = 0; i < floats; ++i) inbox[i] = -7.0f;   // slots outside the image must not be unpacked
        ptrk::multiCollectNeighbourRows(mp, outboxes.get(), offset.data(), inbox.get());
        for (uint32_t i = 0; i < mp.bands * 2u * w; ++i) ptrk::multiHaloUnpack(mp, i, inbox.get(), eOf[p].get());
        for (uint32_t y = 0; y < h; ++y) {
            const uint32_t b = y / 8u;
            const bool own = b % parts == p;
            // a row of another partition is a neighbour when it is the last row of the band above an own band or the first of the band below
            const bool above = !own && y % 8u == 7u && b + 1u < totalBands && (b + 1u) % parts == p;
            const bool below = !own && y % 8u == 0u && b > 0u && (b - 1u) % parts == p;
            for (uint32_t x = 0; x < w; ++x) {
                const float got = eOf[p][static_cast<size_t>(y) * w + x];
                const float want = own || above || below ? truth[static_cast<size_t>(y) * w + x] : -1.0f;
                if (got != want) {
                    std::printf("%ux%u P=%u: partition %u has e(%u, %u) = %g, expected %g\n", w, h, parts, p, x, y, got, want);
                    return 1;
                }
                ++checked;
            }
        }
    }
    // ---- finish in band layout, then interleave
    // (the renderer's layout on the first device: each partition's rgb, cov and count in one piece, the partitions one after the other)
    std::unique_ptr<uint32_t[]> gathered(new uint32_t[partPixel[parts] * 10]);
    std::vector<uint64_t> rgbAt(parts), covAt(parts), countAt(parts);
    std::vector<uint32_t> writers(h, 0u);
    for (uint32_t p = 0; p < parts; ++p) {
        const ptrk::MultiPart mp{p, parts, bandCount(h, p, parts), w, h};
        const size_t mine = static_cast<size_t>(partPixel[p + 1u] - partPixel[p]);
        std::unique_ptr<float[]> rgb(new float[mine * 3]), cov(new float[mine * 6]);
        std::unique_ptr<uint32_t[]> count(new uint32_t[mine]);
        // the partition's state is the image's on its own rows and zero elsewhere, as on the device
        std::unique_ptr<uint32_t[]> nOf(new uint32_t[pixels]);
        for (size_t q = 0; q < pixels; ++q) nOf[q] = ((q / w) / 8u) % parts == p ? n[q] : 0u;
        const ptrk::AdaptiveState st{sum.get(), mean.get(), m.get(), nOf.get(), eOf[p].get()};
        for (uint32_t i = 0; i < mp.bands * 8u * w; ++i) {
            ptrk::multiFinishBands(mp, i, st, rgb.get(), cov.get(), count.get());
            const uint32_t row = i / w, y = ptrk::multiBandTop(mp, row / 8u) + row % 8u;
            if (i % w == 0u && y < h) ++writers[y];
            if (y < h && count[i] == 0u) {
                std::printf("%ux%u P=%u: partition %u finished a pixel it does not own (row %u)\n", w, h, parts, p, y);
                return 1;
            }
        }
        if (mine) ptrk::multiFinishBands(mp, 0u, st, rgb.get(), nullptr, nullptr);   // cov and count are optional
        rgbAt[p] = partPixel[p] * 10u, covAt[p] = rgbAt[p] + mine * 3u, countAt[p] = rgbAt[p] + mine * 9u;
        std::memcpy(gathered.get() + rgbAt[p], rgb.get(), mine * 3 * sizeof(float));
        std::memcpy(gathered.get() + covAt[p], cov.get(), mine * 6 * sizeof(float));
        std::memcpy(gathered.get() + countAt[p], count.get(), mine * sizeof(uint32_t));
    }
    for (uint32_t y = 0; y < h; ++y) {
        if (writers[y] != 1u) {
            std::printf("%ux%u P=%u: row %u is written by %u partitions\n", w, h, parts, y, writers[y]);
            return 1;
        }
    }
    std::unique_ptr<float[]> iRgb(new float[pixels * 3]), iCov(new float[pixels * 6]);
    std::unique_ptr<uint32_t[]> iCount(new uint32_t[pixels]);
    for (uint64_t i = 0; i < pixels * 3; ++i) ptrk::multiInterleave(i, gathered.get(), rgbAt.data(), parts, w, 3u, reinterpret_cast<uint32_t*>(iRgb.get()));
    for (uint64_t i = 0; i < pixels * 6; ++i) ptrk::multiInterleave(i, gathered.get(), covAt.data(), parts, w, 6u, reinterpret_cast<uint32_t*>(iCov.get()));
    for (uint64_t i = 0; i < pixels; ++i) ptrk::multiInterleave(i, gathered.get(), countAt.data(), parts, w, 1u, iCount.get());
    // the plain frame's layout: every partition's rgb and nothing else, in a buffer of exactly that size
    std::unique_ptr<uint32_t[]> plain(new uint32_t[partPixel[parts] * 3]);
    std::vector<uint64_t> plainAt(parts);
    for (uint32_t p = 0; p < parts; ++p) {
        plainAt[p] = partPixel[p] * 3u;
        std::memcpy(plain.get() + plainAt[p], gathered.get() + rgbAt[p], static_cast<size_t>(partPixel[p + 1u] - partPixel[p]) * 3 * sizeof(float));
    }
    std::unique_ptr<float[]> iPlain(new float[pixels * 3]);
    for (uint64_t i = 0; i < pixels * 3; ++i) ptrk::multiInterleave(i, plain.get(), plainAt.data(), parts, w, 3u, reinterpret_cast<uint32_t*>(iPlain.get()));
    if (std::memcmp(iPlain.get(), iRgb.get(), pixels * 3 * sizeof(float)) != 0) {
        std::printf("%ux%u P=%u: the image interleaved from the rgb-only layout is not the one from the full layout\n", w, h, parts);
        return 1;
    }
    for (size_t p = 0; p < pixels; ++p) {
        const float fn = static_cast<float>(n[p]), norm = fn * static_cast<float>(n[p] - 1u);
        bool same = iCount[p] == n[p];
        for (int c = 0; c < 3; ++c) same = same && iRgb[p * 3 + c] == sum[p * 3 + c] / fn;
        for (int c = 0; c < 6; ++c) same = same && iCov[p * 6 + c] == m[p * 6 + c] / norm;
        if (!same) {
            std::printf("%ux%u P=%u: pixel %zu of the interleaved image is not the single-device output\n", w, h, parts, p);
            return 1;
        }
        ++checked;
    }
    return 0;
}

}  // namespace

int main() {
    unsigned long long cases = 0;
    for (uint32_t h = 1; h <= 70; ++h) {
        const uint32_t bands = (h + 7u) / 8u;
        for (uint32_t w = 1; w <= 130; ++w) {
            uint32_t last = 0u;
            for (uint32_t parts : {1u, 2u, 3u, bands}) {
                if (parts == last || (parts == bands && bands <= 3u)) continue;   // (the number of bands is one of 1, 2, 3 for small images)
                last = parts;
                if (checkSize(w, h, parts)) return 1;
                ++cases;
            }
        }
    }
    std::printf("multi host check: %llu cases, %llu values compared, no finding\n", cases, checked);
    return cases > 0 && checked > 0 ? 0 : 1;
}
