// Host check of the index arithmetic of the checkpoint kernels' per-element bodies (csrc/kernels/multi.h: multiStatePack and
// multiStateUnpack, include/ptr_multi_frame.h), over every image size 1x1 .. 130x70 with P = 1, 2, 3 and the number of bands, on heap
// buffers of exactly the size the renderer gives them, so that an address or undefined-behaviour sanitizer sees any step outside.
// Build and run on the host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imetal-pathtracer-arm64_amd/csrc/kernels \
//       tools/multi_frame_host_check.cpp -o /tmp/multi_frame_host_check && /tmp/multi_frame_host_check
// Checked besides the addresses, with distinct words in every plane and NaNs among them: pack writes every word of the partition's own
// pixels to its place in the planar band layout and leaves the positions of a ragged last band outside the image alone; the packed
// buffers of all partitions unpacked into one set of image-order arrays - what an export does on the host - give the image's state,
// every word written exactly once; unpack into a partition's arrays writes its own pixels and nothing else.
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

// five image-order arrays as words; value(plane, index) is distinct per plane and position, with NaN bit patterns among the floats
struct Image {
    std::unique_ptr<uint32_t[]> sum, mean, m, n, e;
    explicit Image(size_t pixels) : sum(new uint32_t[pixels * 3]), mean(new uint32_t[pixels * 3]), m(new uint32_t[pixels * 6]), n(new uint32_t[pixels]), e(new uint32_t[pixels]) {}
    ptrk::AdaptiveState state() const {
        return ptrk::AdaptiveState{reinterpret_cast<float*>(sum.get()), reinterpret_cast<float*>(mean.get()), reinterpret_cast<float*>(m.get()), n.get(),
                                   reinterpret_cast<float*>(e.get())};
    }
    void fill(size_t pixels, uint32_t salt) {
        auto word = [&](uint32_t plane, size_t i) {
            const uint32_t v = salt + plane * 0x01000000u + static_cast<uint32_t>(i);
            return i % 7u == 3u ? 0x7FC00000u | (v & 0x3FFFFFu) : v;   // (a quiet NaN that keeps its payload)
        };
        for (size_t i = 0; i < pixels * 3; ++i) sum[i] = word(1u, i), mean[i] = word(2u, i);
        for (size_t i = 0; i < pixels * 6; ++i) m[i] = word(3u, i);
        for (size_t i = 0; i < pixels; ++i) n[i] = word(4u, i), e[i] = word(5u, i);
    }
    bool samePixel(const Image& o, size_t p) const {
        return std::memcmp(&sum[p * 3], &o.sum[p * 3], 12) == 0 && std::memcmp(&mean[p * 3], &o.mean[p * 3], 12) == 0 &&
               std::memcmp(&m[p * 6], &o.m[p * 6], 24) == 0 && n[p] == o.n[p] && e[p] == o.e[p];
    }
};

int checkSize(uint32_t w, uint32_t h, uint32_t parts) {
    const size_t pixels = static_cast<size_t>(w) * h;
    Image truth(pixels), exported(pixels);
    truth.fill(pixels, 0x10000000u);
    exported.fill(pixels, 0x20000000u);   // every word must be overwritten by exactly one partition
    std::vector<uint32_t> writers(pixels, 0u);
    for (uint32_t p = 0; p < parts; ++p) {
        const ptrk::MultiPart mp{p, parts, bandCount(h, p, parts), w, h};
        const size_t b = ptrk::multiBandPixels(mp), words = b * ptrk::kMultiStateWords;
        const uint32_t sentinel = 0x0BADF00Du;
        std::unique_ptr<uint32_t[]> packed(new uint32_t[words ? words : 1u]);
        for (size_t i = 0; i < words; ++i) packed[i] = sentinel;
        float* const fp = reinterpret_cast<float*>(packed.get());
        for (uint32_t i = 0; i < b; ++i) ptrk::multiStatePack(mp, i, truth.state(), fp);
        // every position of the band layout: the pixel's words in the five planes, or the sentinel outside the image
        for (uint32_t i = 0; i < b; ++i) {
            size_t px = 0;
            const bool inside = ptrk::multiBandPixel(mp, i, &px);
            bool ok = true;
            for (uint32_t c = 0; c < 3u; ++c) {
                ok = ok && packed[static_cast<size_t>(i) * 3u + c] == (inside ? truth.sum[px * 3u + c] : sentinel);
                ok = ok && packed[3u * b + static_cast<size_t>(i) * 3u + c] == (inside ? truth.mean[px * 3u + c] : sentinel);
            }
            for (uint32_t c = 0; c < 6u; ++c) ok = ok && packed[6u * b + static_cast<size_t>(i) * 6u + c] == (inside ? truth.m[px * 6u + c] : sentinel);
            ok = ok && packed[12u * b + i] == (inside ? truth.n[px] : sentinel) && packed[13u * b + i] == (inside ? truth.e[px] : sentinel);
            if (inside && (px / w / 8u) % parts != p) ok = false;   // only its own rows
            if (!ok) {
                std::printf("%ux%u P=%u: partition %u packed position %u wrongly\n", w, h, parts, p, i);
                return 1;
            }
            if (inside) ++writers[px];
            ++checked;
        }
        // the host side of an export: this partition's rows of the caller's image-order arrays
        for (uint32_t i = 0; i < b; ++i) ptrk::multiStateUnpack(mp, i, fp, exported.state());
        // the device side of an import: into the partition's own arrays, which hold something else everywhere
        Image mine(pixels), before(pixels);
        mine.fill(pixels, 0x30000000u);
        before.fill(pixels, 0x30000000u);
        for (uint32_t i = 0; i < b; ++i) ptrk::multiStateUnpack(mp, i, fp, mine.state());
        for (size_t px = 0; px < pixels; ++px) {
            const bool own = (px / w / 8u) % parts == p;
            if (!mine.samePixel(own ? truth : before, px)) {
                std::printf("%ux%u P=%u: partition %u unpacked pixel %zu wrongly (own: %d)\n", w, h, parts, p, px, own ? 1 : 0);
                return 1;
            }
            ++checked;
        }
    }
    for (size_t px = 0; px < pixels; ++px) {
        if (writers[px] != 1u || !exported.samePixel(truth, px)) {
            std::printf("%ux%u P=%u: pixel %zu is exported by %u partitions or with other words\n", w, h, parts, px, writers[px]);
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
            for (uint32_t parts : {1u, 2u, 3u, bands, bands + 2u}) {   // (bands + 2: partitions without pixels)
                if (parts == last || (parts == bands && bands <= 3u)) continue;
                last = parts;
                if (checkSize(w, h, parts)) return 1;
                ++cases;
            }
        }
    }
    std::printf("multi frame host check: %llu cases, %llu positions and pixels compared, no finding\n", cases, checked);
    return cases > 0 && checked > 0 ? 0 : 1;
}
