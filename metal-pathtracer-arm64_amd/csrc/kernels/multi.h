// An adaptive or covariance-carrying frame on several devices (include/ptr_multi.h, whose text this file follows): the per-element
// bodies of the kernels in multi.hip, written as host + device functions on plain pointers so that the renderer, the test-only probe and
// a host program that walks the index arithmetic (tools/multi_host_check.cpp) all run the same code, and the launchers.  The two
// checkpoint bodies of the resumable frame on several devices (include/ptr_multi_frame.h; tools/multi_frame_host_check.cpp) are here too.
//
// A partition p of P owns the image bands b = p + k P, k = 0 .. bands_p - 1 (k: its local band).  Band b covers the image rows
// 8 b .. min(8 b + 8, height) - 1.  Two layouts besides the image:
//   edge rows   [bands_p][2][width]        slot (k, 0): a row at the top of local band k, slot (k, 1): a row at its bottom
//   band layout [bands_p][8][width][ch]    the layout of ptr_render_bands; rows of the last band past the image are padding
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "adaptive.h"

namespace ptrk {

constexpr uint32_t kMultiBandRows = 8u;   // PTR_BAND_ROWS

// which partition and bands a launch works on
struct MultiPart {
    uint32_t part, parts;    // p of P
    uint32_t bands;          // local bands of p (ptr_part_band_count)
    uint32_t width, height;
};

PTR_HD uint32_t multiBandTop(const MultiPart& mp, uint32_t localBand) { return (mp.part + localBand * mp.parts) * kMultiBandRows; }
// the row after the band's last
PTR_HD uint32_t multiBandEnd(const MultiPart& mp, uint32_t localBand) {
    const uint32_t end = multiBandTop(mp, localBand) + kMultiBandRows;
    return end < mp.height ? end : mp.height;
}

// Pack, float i of the edge rows (i < bands * 2 * width): the partition's OWN first (slot 0) and last (slot 1) row of every band, read
// from its image-order e array.  A band of one row publishes that row twice.
PTR_HD void multiHaloPack(const MultiPart& mp, uint32_t i, const float* e, float* edge) {
    const uint32_t slot = i / mp.width, x = i - slot * mp.width;
    const uint32_t k = slot >> 1;
    const uint32_t y = (slot & 1u) ? multiBandEnd(mp, k) - 1u : multiBandTop(mp, k);
    edge[i] = e[static_cast<size_t>(y) * mp.width + x];
}

// Unpack, float i of the edge rows: the NEIGHBOURS' rows - slot 0 the row above the band, slot 1 the row below it - written into the
// image-order e array where that row is in the image (the first band has no row above, the last none below).
PTR_HD void multiHaloUnpack(const MultiPart& mp, uint32_t i, const float* edge, float* e) {
    const uint32_t slot = i / mp.width, x = i - slot * mp.width;
    const uint32_t k = slot >> 1;
    uint32_t y;
    if (slot & 1u) {
        y = multiBandTop(mp, k) + kMultiBandRows;
        if (y >= mp.height) return;
    } else {
        y = multiBandTop(mp, k);
        if (y == 0u) return;
        y -= 1u;
    }
    e[static_cast<size_t>(y) * mp.width + x] = edge[i];
}

// Finish, position i of the band layout (i < bands * 8 * width): the outputs of ptr_adaptive.h for the image pixel at that position,
// the arithmetic of k_adaptive_finish; padding rows get zeros.  cov and count may be null.
PTR_HD void multiFinishBands(const MultiPart& mp, uint32_t i, const AdaptiveState& st, float* rgb, float* cov, uint32_t* count) {
    const uint32_t row = i / mp.width, x = i - row * mp.width;
    const uint32_t y = multiBandTop(mp, row / kMultiBandRows) + row % kMultiBandRows;
    float* o = rgb + static_cast<size_t>(i) * 3u;
    float* c = cov ? cov + static_cast<size_t>(i) * 6u : nullptr;
    if (y >= mp.height) {
        o[0] = o[1] = o[2] = 0.0f;
        if (c) {
            for (uint32_t k = 0; k < 6u; ++k) c[k] = 0.0f;
        }
        if (count) count[i] = 0u;
        return;
    }
    const size_t p = static_cast<size_t>(y) * mp.width + x;
    const uint32_t n = st.n[p];
    const float fn = static_cast<float>(n);
    const float* s = st.sum + p * 3u;
    o[0] = s[0] / fn;
    o[1] = s[1] / fn;
    o[2] = s[2] / fn;
    if (c) {
        const float norm = fn * static_cast<float>(n - 1u);
        const float* m = st.m + p * 6u;
        for (uint32_t k = 0; k < 6u; ++k) c[k] = m[k] / norm;
    }
    if (count) count[i] = n;
}

// Interleave, word i of an image of `channels` 4-byte words per pixel (i < width * height * channels): the gather step of a frame on
// several devices, image band b = local band b / P of partition b % P.  `gathered` holds the partitions' buffers; this output's band
// layout of partition p starts at word partWordOffset[p] (any layout of the buffers around it: ptr_render_multi's hold rgb alone).  Words are copied as bits (the count image is uint32).
PTR_HD void multiInterleave(uint64_t i, const uint32_t* gathered, const uint64_t* partWordOffset, uint32_t parts, uint32_t width, uint32_t channels,
                            uint32_t* image) {
    const uint64_t rowWords = static_cast<uint64_t>(width) * channels;
    const uint32_t y = static_cast<uint32_t>(i / rowWords);
    const uint64_t inRow = i - static_cast<uint64_t>(y) * rowWords;
    const uint32_t band = y / kMultiBandRows, part = band % parts, localBand = band / parts;
    image[i] = gathered[partWordOffset[part] + (static_cast<uint64_t>(localBand) * kMultiBandRows + y % kMultiBandRows) * rowWords + inRow];
}

// Host side of the exchange.  `outboxes` holds the edge rows every partition packed, partition q's at float offset[q]; `inbox` receives
// partition mp.part's neighbour rows in multiHaloUnpack's layout (slot 0: the row above the band, slot 1: the row below).  Slots whose row
// is outside the image are left alone; the unpack skips them too.  mp.parts >= 2: a neighbouring band always belongs to another partition.
inline void multiCollectNeighbourRows(const MultiPart& mp, const float* outboxes, const size_t* offset, float* inbox) {
    const uint32_t totalBands = (mp.height + kMultiBandRows - 1u) / kMultiBandRows;
    for (uint32_t k = 0; k < mp.bands; ++k) {
        const uint32_t b = mp.part + k * mp.parts;
        if (b > 0u) {   // the bottom row of band b - 1
            const uint32_t q = (b - 1u) % mp.parts, kq = (b - 1u) / mp.parts;
            const float* src = outboxes + offset[q] + static_cast<size_t>(2u * kq + 1u) * mp.width;
            float* dst = inbox + static_cast<size_t>(2u * k) * mp.width;
            for (uint32_t x = 0; x < mp.width; ++x) dst[x] = src[x];
        }
        if (b + 1u < totalBands) {   // the top row of band b + 1
            const uint32_t q = (b + 1u) % mp.parts, kq = (b + 1u) / mp.parts;
            const float* src = outboxes + offset[q] + static_cast<size_t>(2u * kq) * mp.width;
            float* dst = inbox + static_cast<size_t>(2u * k + 1u) * mp.width;
            for (uint32_t x = 0; x < mp.width; ++x) dst[x] = src[x];
        }
    }
}

// The checkpoint buffer of a partition (include/ptr_multi_frame.h): its own pixels' state, dense, in band layout and planar - with
// B = bands * 8 * width band pixels the words sum [B][3] at 0, mean [B][3] at 3 B, M [B][6] at 6 B, n [B] at 12 B, e [B] at 13 B.
constexpr uint32_t kMultiStateWords = 14u;
PTR_HD size_t multiBandPixels(const MultiPart& mp) { return static_cast<size_t>(mp.bands) * kMultiBandRows * mp.width; }
// the image pixel at position i of the band layout; false for a row of a ragged last band that lies outside the image
PTR_HD bool multiBandPixel(const MultiPart& mp, uint32_t i, size_t* pixel) {
    const uint32_t row = i / mp.width, x = i - row * mp.width;
    const uint32_t y = multiBandTop(mp, row / kMultiBandRows) + row % kMultiBandRows;
    if (y >= mp.height) return false;
    *pixel = static_cast<size_t>(y) * mp.width + x;
    return true;
}

// Pack, position i of the band layout (i < B): the state of the image pixel at that position goes from the image-order arrays into the
// planes of `packed`.  Positions outside the image are neither read nor written.  Words are copied as they are (n is a uint32 plane).
PTR_HD void multiStatePack(const MultiPart& mp, uint32_t i, const AdaptiveState& st, float* packed) {
    size_t p;
    if (!multiBandPixel(mp, i, &p)) return;
    const size_t b = multiBandPixels(mp), at = i;
    for (uint32_t c = 0; c < 3u; ++c) packed[at * 3u + c] = st.sum[p * 3u + c];
    for (uint32_t c = 0; c < 3u; ++c) packed[3u * b + at * 3u + c] = st.mean[p * 3u + c];
    for (uint32_t c = 0; c < 6u; ++c) packed[6u * b + at * 6u + c] = st.m[p * 6u + c];
    reinterpret_cast<uint32_t*>(packed)[12u * b + at] = st.n[p];
    packed[13u * b + at] = st.e[p];
}

// Unpack, position i of the band layout: the reverse.
PTR_HD void multiStateUnpack(const MultiPart& mp, uint32_t i, const float* packed, const AdaptiveState& st) {
    size_t p;
    if (!multiBandPixel(mp, i, &p)) return;
    const size_t b = multiBandPixels(mp), at = i;
    for (uint32_t c = 0; c < 3u; ++c) st.sum[p * 3u + c] = packed[at * 3u + c];
    for (uint32_t c = 0; c < 3u; ++c) st.mean[p * 3u + c] = packed[3u * b + at * 3u + c];
    for (uint32_t c = 0; c < 6u; ++c) st.m[p * 6u + c] = packed[6u * b + at * 6u + c];
    st.n[p] = reinterpret_cast<const uint32_t*>(packed)[12u * b + at];
    st.e[p] = packed[13u * b + at];
}

#if defined(__HIPCC__)
// dPacked: multiBandPixels(mp) * kMultiStateWords words.  Nothing is launched for a partition without bands.
void launchMultiStatePack(const MultiPart& mp, const AdaptiveState& state, float* dPacked, hipStream_t stream);
void launchMultiStateUnpack(const MultiPart& mp, const float* dPacked, const AdaptiveState& state, hipStream_t stream);
// dEdge: mp.bands * 2 * mp.width floats.  Nothing is launched for a partition without bands.
void launchMultiHaloPack(const MultiPart& mp, const float* dE, float* dEdge, hipStream_t stream);
void launchMultiHaloUnpack(const MultiPart& mp, const float* dEdge, float* dE, hipStream_t stream);
// dRgb / dCov / dCount: mp.bands * 8 * mp.width pixels of 3 / 6 / 1 words (dCov and dCount may be null)
void launchMultiFinishBands(const MultiPart& mp, const AdaptiveState& state, float* dRgb, float* dCov, uint32_t* dCount, hipStream_t stream);
void launchMultiInterleave(const void* dGathered, const uint64_t* dPartWordOffset, uint32_t parts, uint32_t width, uint32_t height, uint32_t channels,
                           void* dImage, hipStream_t stream);
// Probe only: items[c * active + j] = samples[(nBefore + c) * pixels + list[j]], c < spp
void launchMultiGatherItems(const float4* dSamples, size_t pixels, const uint32_t* dList, uint32_t active, uint32_t spp, uint32_t nBefore, float4* dItems,
                            hipStream_t stream);
#endif

}  // namespace ptrk
