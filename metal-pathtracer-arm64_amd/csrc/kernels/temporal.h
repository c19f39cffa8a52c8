// Host-callable launcher of the temporal accumulation kernel (defined in temporal.hip; the rule is spelled out in include/ptr_temporal.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptr_temporal.h"

namespace ptrk {

// A camera as the filter projects through it: origin, lower-left corner, horizontal, vertical (CameraParams' first four fields).
struct TemporalCamera {
    float o[3], ll[3], h[3], w[3];
};

// The buffers of one step, width*height entries each.
struct TemporalBuffers {
    const float4* r0;        // this step's records
    const float4* r1;
    const float4* r2;
    const float4* prevR0;    // the previous step's (never read without history)
    const float4* prevR1;
    const float4* history;   // (rgb, length) of the previous step (never read without history)
    float4* historyOut;      // a different buffer from `history`: a lane reads four taps other lanes write
};

// dOut may equal dRgb; dLength may be null
void launchTemporalAccumulate(const float* dRgb, const TemporalBuffers& buf, const TemporalCamera& cur, const TemporalCamera& prev, uint32_t width,
                              uint32_t height, const PtrTemporalParams& p, bool hasHistory, float* dOut, float* dLength, hipStream_t stream);

}  // namespace ptrk
