// The kernels of include/ptr_rebuild.h (launchers in rebuild.h; the header numbers the steps).  Compiled like dynamic.hip: unfused, with
// correctly rounded division, so tests/rebuild_ref.py restates every value bit for bit.  What bounds each kernel:
// k_tree_cost        streams the 64 B float nodes once (four 16 B loads per lane); the block sum is 256 serial float64 adds by one lane
//                    out of LDS, which fixes the order.  Bandwidth bound but for that tail.
// k_rb_keys          one leaf per lane: a 4 B reference, then 2 x 16 B per primitive of the leaf (at most 8), gathered through the
//                    reference but contiguous within a leaf; 8 B out.  Float64 only for the three divisions of the key.
// k_rb_topology      one radix node per lane: about 2 log2(range) key loads (8 B, nearby positions first), no stores but 20 B.  Latency bound.
// k_rb_number        a walk up the parent words, at most the depth of the tree; 4 B loads, scattered.
// k_rb_nodes         64 B out per lane at a scattered (preorder) place, two 8 B key loads and two 4 B gathers in.
// k_rb_heights       one launch per height: 2 x 16 B of the node, one byte per internal child; a byte out for the nodes that settle.
// k_rb_level_offsets streams the sorted heights (1 B per lane).
// k_rb_wide_mark     one launch per wide level over all nodes: a byte per lane, and for the few wide roots of the level the
//                    chooseWideChildren walk (up to 8 x 16 B of records).  k_rb_wide_write does that walk once per wide root.
// Nothing here hands data between workgroups inside a launch: a value one lane writes is read by other lanes in a later launch only,
// or (k_rb_heights, k_rb_wide_mark) decides nothing in the launch that writes it.  The sorts and the scan are rocprim's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bvh_layout.h"
#include "rebuild.h"

namespace ptrk {

namespace {

constexpr uint32_t kBlock = kRebuildBlock;

__device__ inline float minOf(float a, float b) { return b < a ? b : a; }
__device__ inline float maxOf(float a, float b) { return a < b ? b : a; }
__device__ inline bool internalRef(uint32_t ref, uint32_t nodeCount) { return ref != kRefEmpty && !(ref & kRefLeafBit) && ref < nodeCount; }

__device__ inline double halfAreaOf(float4 lo, float4 hi) {
    const double dx = static_cast<double>(hi.x) - lo.x, dy = static_cast<double>(hi.y) - lo.y, dz = static_cast<double>(hi.z) - lo.z;
    return dx * dy + dy * dz + dz * dx;
}

__global__ void __launch_bounds__(kBlock) k_tree_cost(const float4* __restrict__ boxes, uint32_t nodeCount, double rootHalfArea, double rootArea,
                                                      double* __restrict__ partials) {
    __shared__ double terms[kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double term = 0.0;
    if (i < nodeCount) {
        if (i == 0u) term = rootHalfArea / rootArea;
        const size_t node = i;
        float4 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) row[q] = boxes[node * 4 + q];
        const uint32_t refs[2] = {__float_as_uint(row[0].w), __float_as_uint(row[1].w)};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t r = refs[c];
            if (r == kRefEmpty) continue;
            const double weight = (r & kRefLeafBit) ? static_cast<double>(((r >> kRefCountShift) & 0xFu) + 1u) : 1.0;
            term += halfAreaOf(row[c * 2], row[c * 2 + 1]) / rootArea * weight;
        }
    }
    terms[threadIdx.x] = term;
    __syncthreads();
    if (threadIdx.x == 0u) {
        double sum = 0.0;
        for (uint32_t k = 0; k < kBlock; ++k) sum += terms[k];
        partials[blockIdx.x] = sum;
    }
}

struct RootBox {
    float lo[3], hi[3];
};

__device__ inline uint32_t expandBits10(uint32_t v) {   // bit k of a 10-bit value to bit 3k
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__device__ inline uint32_t mortonAxis(float lo, float hi, float rootLo, float rootHi) {
    const double m = (static_cast<double>(lo) + static_cast<double>(hi)) * 0.5;
    const double extent = static_cast<double>(rootHi) - static_cast<double>(rootLo);
    const double u = extent > 0.0 ? (m - static_cast<double>(rootLo)) / extent : 0.0;
    const double q = floor(u * 1024.0);
    return static_cast<uint32_t>(q >= 1023.0 ? 1023.0 : (q > 0.0 ? q : 0.0));   // (a NaN lands in cell 0)
}

__global__ void __launch_bounds__(kBlock) k_rb_keys(const uint32_t* __restrict__ leaves, uint32_t leafCount, const float4* __restrict__ triBounds,
                                                    const float4* __restrict__ sphereBounds, RootBox root, uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= leafCount) return;
    const uint32_t ref = leaves[i];
    const float4* bounds = (ref & kRefSphereBit) ? sphereBounds : triBounds;
    const size_t first = ref & kRefOffsetMask;
    const uint32_t prims = ((ref >> kRefCountShift) & 0xFu) + 1u;
    const float inf = __uint_as_float(0x7F800000u);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (uint32_t p = 0; p < prims; ++p) {
        const float4 l = bounds[(first + p) * 2], h = bounds[(first + p) * 2 + 1];
        lo[0] = minOf(lo[0], l.x), lo[1] = minOf(lo[1], l.y), lo[2] = minOf(lo[2], l.z);
        hi[0] = maxOf(hi[0], h.x), hi[1] = maxOf(hi[1], h.y), hi[2] = maxOf(hi[2], h.z);
    }
    const uint32_t code = (expandBits10(mortonAxis(lo[0], hi[0], root.lo[0], root.hi[0])) << 2) |
                          (expandBits10(mortonAxis(lo[1], hi[1], root.lo[1], root.hi[1])) << 1) |
                          expandBits10(mortonAxis(lo[2], hi[2], root.lo[2], root.hi[2]));
    keys[i] = (static_cast<uint64_t>(code) << 32) | i;
}

// delta(i, j) of the header; keys are unique, so the exclusive or is never zero
__device__ inline int deltaOf(const uint64_t* __restrict__ keys, int64_t n, uint64_t ki, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __clzll(static_cast<long long>(ki ^ keys[j]));
}

__global__ void __launch_bounds__(kBlock) k_rb_topology(const uint64_t* __restrict__ keys, uint32_t leafCount, uint32_t* __restrict__ firstOf,
                                                        uint2* __restrict__ kids, uint32_t* __restrict__ parent) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    if (lane + 1u >= leafCount) return;
    const int64_t n = leafCount, i = lane;
    const uint64_t ki = keys[i];
    const int64_t d = deltaOf(keys, n, ki, i + 1) > deltaOf(keys, n, ki, i - 1) ? 1 : -1;
    const int dMin = deltaOf(keys, n, ki, i - d);
    int64_t lMax = 2;
    while (deltaOf(keys, n, ki, i + lMax * d) > dMin) lMax *= 2;   // ends: past the array delta is -1 <= dMin
    int64_t l = 0;
    for (int64_t t = lMax / 2; t >= 1; t /= 2) {
        if (deltaOf(keys, n, ki, i + (l + t) * d) > dMin) l += t;
    }
    const int64_t j = i + l * d;
    const int dNode = deltaOf(keys, n, ki, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (deltaOf(keys, n, ki, i + (s + t) * d) > dNode) s += t;
    } while (t > 1);
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const bool leftLeaf = first == gamma, rightLeaf = last == gamma + 1;
    firstOf[lane] = static_cast<uint32_t>(first);
    kids[lane] = make_uint2(static_cast<uint32_t>(gamma) | (leftLeaf ? 0x80000000u : 0u), static_cast<uint32_t>(gamma + 1) | (rightLeaf ? 0x80000000u : 0u));
    if (!leftLeaf) parent[gamma] = lane | 0x80000000u;
    if (!rightLeaf) parent[gamma + 1] = lane;
    if (lane == 0u) parent[0] = 0u;
}

__global__ void __launch_bounds__(kBlock) k_rb_number(const uint32_t* __restrict__ firstOf, const uint32_t* __restrict__ parent, uint32_t nodeCount,
                                                      uint32_t* __restrict__ pre) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    uint32_t j = i, leftSteps = 0u;
    // Before a node in preorder come its ancestors and the subtrees to their left, where the path from the root turns right: those
    // subtrees hold the `first` leaves before its range in as many subtrees as there are right turns, so first - (right turns) nodes.
    // That leaves first + (left turns); the walk to the root takes at most one step per key bit.
    for (uint32_t guard = 0; guard < 64u && j != 0u; ++guard) {
        const uint32_t p = parent[j];
        leftSteps += p >> 31;
        j = p & 0x7FFFFFFFu;
    }
    pre[i] = firstOf[i] + leftSteps;
}

__global__ void __launch_bounds__(kBlock) k_rb_nodes(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ leaves, const uint2* __restrict__ kids,
                                                     const uint32_t* __restrict__ pre, uint32_t nodeCount, float4* __restrict__ boxes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    const uint2 k = kids[i];
    const uint32_t child[2] = {k.x, k.y};
    uint32_t ref[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint32_t at = child[c] & 0x7FFFFFFFu;
        ref[c] = (child[c] & 0x80000000u) ? leaves[static_cast<uint32_t>(keys[at] & 0xFFFFFFFFull)] : pre[at];
    }
    const size_t node = pre[i];
    boxes[node * 4 + 0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[0]));
    boxes[node * 4 + 1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[1]));
    boxes[node * 4 + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    boxes[node * 4 + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(kBlock) k_rb_heights(const float4* __restrict__ boxes, uint32_t nodeCount, uint32_t k, uint8_t* __restrict__ heights,
                                                       uint32_t* __restrict__ iota) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    if (k == 0u) iota[i] = i;
    if (heights[i] != kHeightUnknown) return;
    const size_t node = i;
    const uint32_t refs[2] = {__float_as_uint(boxes[node * 4 + 0].w), __float_as_uint(boxes[node * 4 + 1].w)};
    uint32_t h = 0u;
    bool settled = true;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!internalRef(refs[c], nodeCount)) continue;
        // a height written in THIS launch is k, an unwritten one kHeightUnknown: either way not below k, and the node waits
        const uint32_t hc = heights[refs[c]];
        if (hc >= k) settled = false;
        else h = hc + 1u > h ? hc + 1u : h;
    }
    if (settled && h == k) heights[i] = static_cast<uint8_t>(k);
}

__global__ void __launch_bounds__(kBlock) k_rb_level_offsets(const uint8_t* __restrict__ sortedHeights, uint32_t nodeCount, uint32_t* __restrict__ offsets) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    const uint32_t h = sortedHeights[i];
    if (h < kMaxTreeDepth && (i == 0u || sortedHeights[i - 1u] != h)) offsets[h] = i;
}

struct CellArgs {
    float cell[3];
};

__device__ inline double quantArea(uint4 rec, const CellArgs& g) {
    const double x = (static_cast<double>(rec.y >> 16) - (rec.x & 0xFFFFu)) * g.cell[0];
    const double y = (static_cast<double>(rec.z & 0xFFFFu) - (rec.x >> 16)) * g.cell[1];
    const double z = (static_cast<double>(rec.z >> 16) - (rec.y & 0xFFFFu)) * g.cell[2];
    return x * y + y * z + z * x;
}

// chooseWideChildren(byArea) of host/bvh_builder.cpp with record indices (node * 2 + side) for pointers
struct WideChoice {
    uint4 rec[4];
    uint32_t at[4];
    uint32_t count;
};
__device__ inline uint32_t childrenOf(const uint4* __restrict__ q, uint32_t node, uint4 rec[2], uint32_t at[2]) {
    uint32_t got = 0u;
#pragma unroll
    for (uint32_t side = 0; side < 2u; ++side) {
        const uint4 r = q[static_cast<size_t>(node) * 2u + side];
        if (r.w != kRefEmpty) {
            if (got == 0u) rec[0] = r, at[0] = node * 2u + side;
            else rec[1] = r, at[1] = node * 2u + side;
            ++got;
        }
    }
    return got;
}
__device__ inline WideChoice chooseWide(const uint4* __restrict__ q, uint32_t nodeCount, const CellArgs& g, uint32_t n) {
    WideChoice c;
    c.count = childrenOf(q, n, c.rec, c.at);
    while (c.count < 4u) {
        int best = -1;
        double bestArea = -1.0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (k >= c.count || !internalRef(c.rec[k].w, nodeCount)) continue;
            const double a = quantArea(c.rec[k], g);
            if (a > bestArea) bestArea = a, best = static_cast<int>(k);
        }
        if (best < 0) break;
        uint4 two[2];
        uint32_t twoAt[2];
        uint32_t open = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (static_cast<int>(k) == best) open = c.rec[k].w;
        }
        const uint32_t got = childrenOf(q, open, two, twoAt);
        if (got == 0u) break;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (static_cast<int>(k) == best) c.rec[k] = two[0], c.at[k] = twoAt[0];
            if (got > 1u && k == c.count) c.rec[k] = two[1], c.at[k] = twoAt[1];
        }
        if (got > 1u) ++c.count;
    }
    return c;
}

__global__ void __launch_bounds__(kBlock) k_rb_wide_mark(const uint4* __restrict__ q, uint32_t nodeCount, CellArgs g, uint32_t d, uint8_t* __restrict__ depth,
                                                         uint32_t* __restrict__ marks, uint32_t* __restrict__ reached) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= nodeCount || depth[n] != d) return;   // (a depth written in this launch is d + 1: its node is handled by the next)
    marks[n] = 1u;
    const WideChoice c = chooseWide(q, nodeCount, g, n);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (k >= c.count || !internalRef(c.rec[k].w, nodeCount)) continue;
        depth[c.rec[k].w] = static_cast<uint8_t>(d + 1u);
        reached[d + 1u] = 1u;
    }
}

__global__ void __launch_bounds__(kBlock) k_rb_wide_write(const uint4* __restrict__ q, uint32_t nodeCount, CellArgs g, const uint32_t* __restrict__ marks,
                                                          const uint32_t* __restrict__ wideIndex, uint4* __restrict__ wnodes,
                                                          uint32_t* __restrict__ wideSource) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= nodeCount || marks[n] == 0u) return;
    const size_t w = wideIndex[n];
    const WideChoice c = chooseWide(q, nodeCount, g, n);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (k < c.count) {
            uint32_t ref = c.rec[k].w;
            if (internalRef(ref, nodeCount)) ref = wideIndex[ref];   // its wide node
            wnodes[w * 4 + k] = make_uint4(0u, 0u, 0u, ref);
            wideSource[w * 4 + k] = c.at[k];
        } else {
            wnodes[w * 4 + k] = make_uint4(0xFFFFFFFFu, 0x0000FFFFu, 0x00000000u, kRefEmpty);   // emptyWidePlace
            wideSource[w * 4 + k] = 0xFFFFFFFFu;
        }
    }
}

uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

constexpr unsigned kKeyBits = 62u, kHeightBits = 6u;

}  // namespace

void launchTreeCost(const float4* dBoxes, uint32_t nodeCount, double rootHalfArea, double rootArea, double* dPartials, hipStream_t stream) {
    if (nodeCount > 0u) hipLaunchKernelGGL(k_tree_cost, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dBoxes, nodeCount, rootHalfArea, rootArea, dPartials);
}

void launchRebuildKeys(const uint32_t* dLeaves, uint32_t leafCount, const float4* dTriBounds, const float4* dSphereBounds, const float rootLo[3],
                       const float rootHi[3], uint64_t* dKeys, hipStream_t stream) {
    RootBox root;
    for (int a = 0; a < 3; ++a) root.lo[a] = rootLo[a], root.hi[a] = rootHi[a];
    if (leafCount > 0u) hipLaunchKernelGGL(k_rb_keys, dim3(blocksFor(leafCount)), dim3(kBlock), 0, stream, dLeaves, leafCount, dTriBounds, dSphereBounds, root, dKeys);
}

size_t rebuildSortKeysScratch(uint32_t count) {
    size_t bytes = 0;
    check(rocprim::radix_sort_keys(nullptr, bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), count, 0u, kKeyBits), "radix_sort_keys (size)");
    return bytes;
}

void launchRebuildSortKeys(void* dScratch, size_t scratchBytes, const uint64_t* dKeysIn, uint64_t* dKeysOut, uint32_t count, hipStream_t stream) {
    check(rocprim::radix_sort_keys(dScratch, scratchBytes, dKeysIn, dKeysOut, count, 0u, kKeyBits, stream), "radix_sort_keys");
}

void launchRebuildTopology(const uint64_t* dSortedKeys, uint32_t leafCount, uint32_t* dFirst, uint2* dKids, uint32_t* dParent, hipStream_t stream) {
    if (leafCount > 1u) hipLaunchKernelGGL(k_rb_topology, dim3(blocksFor(leafCount - 1u)), dim3(kBlock), 0, stream, dSortedKeys, leafCount, dFirst, dKids, dParent);
}

void launchRebuildNumber(const uint32_t* dFirst, const uint32_t* dParent, uint32_t nodeCount, uint32_t* dPre, hipStream_t stream) {
    if (nodeCount > 0u) hipLaunchKernelGGL(k_rb_number, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dFirst, dParent, nodeCount, dPre);
}

void launchRebuildNodes(const uint64_t* dSortedKeys, const uint32_t* dLeaves, const uint2* dKids, const uint32_t* dPre, uint32_t nodeCount,
                        float4* dBoxes, hipStream_t stream) {
    if (nodeCount > 0u) hipLaunchKernelGGL(k_rb_nodes, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dSortedKeys, dLeaves, dKids, dPre, nodeCount, dBoxes);
}

void launchRebuildHeights(const float4* dBoxes, uint32_t nodeCount, uint32_t k, uint8_t* dHeights, uint32_t* dIota, hipStream_t stream) {
    if (nodeCount > 0u) hipLaunchKernelGGL(k_rb_heights, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dBoxes, nodeCount, k, dHeights, dIota);
}

size_t rebuildSortScheduleScratch(uint32_t count) {
    size_t bytes = 0;
    check(rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const uint8_t*>(nullptr), static_cast<uint8_t*>(nullptr), static_cast<const uint32_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr), count, 0u, kHeightBits),
          "radix_sort_pairs (size)");
    return bytes;
}

void launchRebuildSchedule(void* dScratch, size_t scratchBytes, const uint8_t* dHeights, uint8_t* dHeightsSorted, const uint32_t* dIota,
                           uint32_t* dSchedule, uint32_t nodeCount, uint32_t* dLevelOffsets, hipStream_t stream) {
    if (nodeCount == 0u) return;
    check(rocprim::radix_sort_pairs(dScratch, scratchBytes, dHeights, dHeightsSorted, dIota, dSchedule, nodeCount, 0u, kHeightBits, stream), "radix_sort_pairs");
    hipLaunchKernelGGL(k_rb_level_offsets, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dHeightsSorted, nodeCount, dLevelOffsets);
}

void launchRebuildWideMark(const uint4* dQnodes, uint32_t nodeCount, const float cell[3], uint32_t d, uint8_t* dDepth, uint32_t* dMarks,
                           uint32_t* dReached, hipStream_t stream) {
    CellArgs g;
    for (int a = 0; a < 3; ++a) g.cell[a] = cell[a];
    if (nodeCount > 0u) hipLaunchKernelGGL(k_rb_wide_mark, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dQnodes, nodeCount, g, d, dDepth, dMarks, dReached);
}

size_t rebuildScanScratch(uint32_t count) {
    size_t bytes = 0;
    check(rocprim::exclusive_scan(nullptr, bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, static_cast<size_t>(count)), "exclusive_scan (size)");
    return bytes;
}

void launchRebuildWideScan(void* dScratch, size_t scratchBytes, const uint32_t* dMarks, uint32_t* dWideIndex, uint32_t nodeCount, hipStream_t stream) {
    check(rocprim::exclusive_scan(dScratch, scratchBytes, dMarks, dWideIndex, 0u, static_cast<size_t>(nodeCount), rocprim::plus<uint32_t>(), stream), "exclusive_scan");
}

void launchRebuildWideWrite(const uint4* dQnodes, uint32_t nodeCount, const float cell[3], const uint32_t* dMarks, const uint32_t* dWideIndex,
                            uint4* dWnodes, uint32_t* dWideSource, hipStream_t stream) {
    CellArgs g;
    for (int a = 0; a < 3; ++a) g.cell[a] = cell[a];
    if (nodeCount > 0u) hipLaunchKernelGGL(k_rb_wide_write, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dQnodes, nodeCount, g, dMarks, dWideIndex, dWnodes, dWideSource);
}

}  // namespace ptrk
