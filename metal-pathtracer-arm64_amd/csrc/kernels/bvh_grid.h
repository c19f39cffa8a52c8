// The 16-bit grid of the quantised nodes, shared by the host builder (plain C++) and the device refit (kernels/dynamic.hip): the rule that
// derives the grid from the root box, and the quantiser of one coordinate and of one child record.  Both sides compile these functions, so
// a refit on the device reproduces the builder's words bit for bit.  All arithmetic is double: division, floor and ceil are exact-rounded
// on both sides.
#pragma once

#include <cstdint>

#include "bvh_layout.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTR_GRID_HD __host__ __device__ inline
#else
#include <math.h>
#define PTR_GRID_HD inline
#endif

namespace ptrk {

constexpr double kGridCells = 65531.0;   // cells 2..65533 span the root box, the rest is padding

// Grid of one axis from the root box: cell = extent / 65531 (1 for an axis without extent), origin = lo - 2 cell.
PTR_GRID_HD void gridAxis(float lo, float hi, float& origin, float& cell) {
    const double extent = static_cast<double>(hi) - lo;
    const double c = extent > 0.0 ? extent / kGridCells : 1.0;
    cell = static_cast<float>(c);
    origin = static_cast<float>(lo - 2.0 * c);
}

// lo is rounded down and hi up, plus one cell of padding on each side, so a quantised box always contains the float box.
PTR_GRID_HD uint32_t quantiseCoord(float v, float origin, float cell, bool up) {
    const double g = (static_cast<double>(v) - origin) / static_cast<double>(cell);
    const double q = up ? ceil(g) + 1.0 : floor(g) - 1.0;
    return static_cast<uint32_t>(q < 0.0 ? 0.0 : (q > 65535.0 ? 65535.0 : q));
}

// One 16 B child record of a quantised node from the float box of the child and its reference; an empty child has a zero box.
PTR_GRID_HD void quantiseChild(const float lo[3], const float hi[3], uint32_t ref, const float origin[3], const float cell[3], uint32_t w[4]) {
    if (ref == kRefEmpty) {
        w[0] = w[1] = w[2] = 0u;
    } else {
        w[0] = quantiseCoord(lo[0], origin[0], cell[0], false) | (quantiseCoord(lo[1], origin[1], cell[1], false) << 16);
        w[1] = quantiseCoord(lo[2], origin[2], cell[2], false) | (quantiseCoord(hi[0], origin[0], cell[0], true) << 16);
        w[2] = quantiseCoord(hi[1], origin[1], cell[1], true) | (quantiseCoord(hi[2], origin[2], cell[2], true) << 16);
    }
    w[3] = ref;
}

}  // namespace ptrk
