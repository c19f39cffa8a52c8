// The one owner of an adaptive frame's device memory: the per-pixel state in image order, the two active lists and the scratch of the
// compaction between the rounds.  The device scene holds one (ptr_render_adaptive, the partitions of multi.cpp), every PtrFrame holds one,
// the test-only probe of one round builds one.  The word layout of the scratch is stated here and nowhere else.
// device_scene.h includes this file between DeviceBuffer and PtrDeviceScene; include that header, not this one.  Implemented in adaptive.cpp.
#pragma once

#include "../kernels/adaptive.h"

namespace ptrhost {

constexpr uint32_t kAdaptiveBlock = 256u;   // threads per block of the compaction kernels (adaptive.hip)

struct AdaptiveStore {
    size_t pixels = 0;   // of the image the last ensure() was for (the buffers only grow)
    DeviceBuffer<float> sum, mean, m, e;
    DeviceBuffer<uint32_t> n, lists, blockWords;
    DeviceBuffer<uint8_t> keep;

    // room for a `pixelCount`-pixel image, grown on demand; the contents are undefined until zero() or upload()
    void ensure(size_t pixelCount);
    // the state of every pixel set to zero (asynchronous on `stream`)
    void zero(hipStream_t stream) const;
    // the five state arrays from / to host memory (blocking)
    void upload(const float* hSum, const float* hMean, const float* hM, const uint32_t* hN, const float* hE);
    void download(float* hSum, float* hMean, float* hM, uint32_t* hN, float* hE) const;

    ptrk::AdaptiveState state() const { return ptrk::AdaptiveState{sum.ptr, mean.ptr, m.ptr, n.ptr, e.ptr}; }
    // blockWords: a count per block of 256 list entries, an offset per block, the total, the class minimum (frame.hip)
    size_t blocks() const { return (pixels + kAdaptiveBlock - 1u) / kAdaptiveBlock; }
    ptrk::AdaptiveScratch scratch() const {
        return ptrk::AdaptiveScratch{keep.ptr, blockWords.ptr, blockWords.ptr + blocks(), blockWords.ptr + 2u * blocks()};
    }
    uint32_t* minWord() const { return scratch().total + 1; }
    uint32_t* list(uint32_t i) const { return lists.ptr + i * pixels; }   // i = 0, 1: the lists ping-pong
};

}  // namespace ptrhost
