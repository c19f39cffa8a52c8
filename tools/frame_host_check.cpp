// Host check of the index arithmetic of the resumable frame's per-element bodies (csrc/kernels/frame.h): the bodies are host + device
// functions, and this program drives them - the class minimum, the split predicate and the merge predicate - over every image size
// 1x1 .. 130x70 on heap buffers of exactly the size the frame gives them, so that an address or undefined-behaviour sanitizer sees any
// step outside.  Beside them it drives the frames' host table of pixels per count (csrc/host/frame_classes.h) with the moves those
// rounds make - the class minimum, the size of S - and compares it after every move with the histogram of the counts themselves.
// Build and run on the host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host \
//       -Imetal-pathtracer-arm64_amd/csrc/kernels tools/frame_host_check.cpp -o /tmp/frame_host_check && /tmp/frame_host_check
// (The ranks of the compaction come from a wave ballot and exist on the device only; the tests compare its output with the restatement.)
#include <cstdio>
#include <memory>
#include <vector>

#include "frame.h"
#include "frame_classes.h"

namespace {

constexpr uint32_t kLastClass = 16u, kMaxCount = kLastClass + 4u;   // the counts start at 4, 8, 12 and 16, and every class takes one step of 4

// the table against the histogram of n, count by count, and what it derives from itself against what n says
bool sameAsCounts(const ptrhost::CountClasses& classes, const uint32_t* n, size_t pixels) {
    uint64_t hist[kMaxCount + 1u] = {};
    uint64_t total = 0;
    uint32_t lo = n[0], hi = n[0];
    for (size_t p = 0; p < pixels; ++p) {
        if (n[p] > kMaxCount) return false;
        ++hist[n[p]];
        total += n[p];
        lo = n[p] < lo ? n[p] : lo;
        hi = n[p] > hi ? n[p] : hi;
    }
    for (uint32_t c = 0; c <= kMaxCount; ++c) {
        if (classes.pixelsAt(c) != hist[c]) return false;
    }
    PtrFrameInfo info{};
    classes.fill(info);
    return classes.minCount() == lo && classes.maxCount() == hi && classes.uniform() == (lo == hi) && classes.empty() == (hi == 0u) &&
           classes.pixelsAt(classes.maxCount()) == hist[hi] && info.minCount == lo && info.maxCount == hi && info.totalSamples == total &&
           info.uniform == (lo == hi ? 1u : 0u);
}

}  // namespace

int main() {
    unsigned long long visited = 0, inClass = 0, kept = 0, dropped = 0, moves = 0;
    for (uint32_t h = 1; h <= 70; ++h) {
        for (uint32_t w = 1; w <= 130; ++w) {
            const size_t pixels = static_cast<size_t>(w) * h;
            std::unique_ptr<float[]> e(new float[pixels]);
            std::unique_ptr<uint32_t[]> n(new uint32_t[pixels]);
            for (size_t p = 0; p < pixels; ++p) {   // counts 4, 8, 12 and 16 interleaved; errors 0 .. 1
                const uint32_t r = static_cast<uint32_t>((p + w) * 2654435761u);
                n[p] = 4u + 4u * ((r >> 13) & 3u);
                e[p] = static_cast<float>((r >> 7) % 1000u) * 1e-3f;
            }
            // L: about three quarters of the image in the renderer's order (8-row bands, 8x8 blocks), in a buffer of exactly its length
            std::vector<uint32_t> order;
            for (uint32_t ty = 0; ty < h; ty += 8)
                for (uint32_t tx = 0; tx < w; tx += 8)
                    for (uint32_t y = ty; y < ty + 8 && y < h; ++y)
                        for (uint32_t x = tx; x < tx + 8 && x < w; ++x)
                            if ((y * w + x) % 4u != 1u || pixels == 1u) order.push_back(y * w + x);
            const uint32_t count = static_cast<uint32_t>(order.size());
            if (count == 0u) continue;
            // the table: every pixel at 0, the first samples of all of them, then the counts as an import brings them
            ptrhost::CountClasses classes;
            classes.reset(pixels);
            if (!classes.empty() || classes.pixelsAt(0u) != pixels) return 6;
            classes.move(0u, 4u, pixels);
            if (!classes.uniform() || classes.minCount() != 4u || classes.pixelsAt(4u) != pixels || classes.pixelsAt(0u) != 0u) return 6;
            classes.rebuild(n.get(), pixels);
            if (!sameAsCounts(classes, n.get(), pixels)) return 6;
            std::unique_ptr<uint32_t[]> list(new uint32_t[count]);
            for (uint32_t j = 0; j < count; ++j) list[j] = order[j];
            uint32_t nMin = ptrk::kFrameNoCount, want = ptrk::kFrameNoCount;
            for (uint32_t j = 0; j < count; ++j) {   // k_frame_class_min's body
                nMin = ptrk::frameClassMin(nMin, list.get(), j, n.get());
                if (n[order[j]] < want) want = n[order[j]];
            }
            if (nMin != want || nMin == ptrk::kFrameNoCount) return 2;
            std::unique_ptr<uint8_t[]> inS(new uint8_t[count]);
            uint32_t members = 0;
            for (uint32_t j = 0; j < count; ++j) {   // k_frame_split's body
                inS[j] = ptrk::frameInClass(list.get(), j, n.get(), nMin) ? 1u : 0u;
                members += inS[j];
            }
            if (members == 0u) return 3;
            for (uint32_t j = 0; j < count; ++j) {   // the update of S, then k_frame_merge's body
                if (inS[j]) n[list[j]] = nMin + 4u;
            }
            for (uint32_t j = 0; j < count; ++j) {
                const bool keep = ptrk::frameMergeKeep(list.get(), j, inS.get(), w, h, e.get(), n.get(), 16u, 0.9f);
                if (!inS[j] && !keep) return 4;   // an entry outside S stays
                if (inS[j] && keep != ptrk::adaptiveKeep(list[j], w, h, e.get(), n.get(), 16u, 0.9f)) return 5;
                kept += keep ? 1u : 0u;
                dropped += keep ? 0u : 1u;
                ++visited;
            }
            inClass += members;
            classes.move(nMin, nMin + 4u, members);
            ++moves;
            if (!sameAsCounts(classes, n.get(), pixels)) return 7;
            // the rounds that follow on the same list, lowest class first, until every entry is past the last class
            for (;;) {
                uint32_t next = ptrk::kFrameNoCount, size = 0;
                for (uint32_t j = 0; j < count; ++j) next = ptrk::frameClassMin(next, list.get(), j, n.get());
                if (next > kLastClass) break;
                for (uint32_t j = 0; j < count; ++j) {
                    if (!ptrk::frameInClass(list.get(), j, n.get(), next)) continue;
                    n[list[j]] = next + 4u;
                    ++size;
                }
                classes.move(next, next + 4u, size);
                ++moves;
                if (size == 0u || !sameAsCounts(classes, n.get(), pixels)) return 7;
            }
        }
    }
    std::printf("frame host check: %llu entries visited, %llu in their round's class, %llu kept, %llu dropped, %llu class moves, no finding\n", visited,
                inClass, kept, dropped, moves);
    return visited > 0 && inClass > 0 && inClass < visited && kept > 0 && dropped > 0 && moves > 0 ? 0 : 1;
}
