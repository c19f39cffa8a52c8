// Launchers of the rebuild kernels (rebuild.hip; include/ptr_rebuild.h, whose step numbers the comments use).  Every array is the
// caller's; sizes are in elements.  The boxes a rebuild writes are fitted, quantised and copied by the launchers of dynamic.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ptrk {

constexpr uint32_t kRebuildBlock = 256u;
constexpr uint8_t kHeightUnknown = 0xFFu;

// Tree cost: one partial sum per block of kRebuildBlock nodes (blocks = ceil(nodeCount / kRebuildBlock)), terms in index order.
// rootHalfArea / rootArea come from node 0, which the host reads first.
void launchTreeCost(const float4* dBoxes, uint32_t nodeCount, double rootHalfArea, double rootArea, double* dPartials, hipStream_t stream);

// Steps 2-3: key = morton(leaf box centre in the root box) << 32 | leaf index
void launchRebuildKeys(const uint32_t* dLeaves, uint32_t leafCount, const float4* dTriBounds, const float4* dSphereBounds, const float rootLo[3],
                       const float rootHi[3], uint64_t* dKeys, hipStream_t stream);
// Step 4 (rocprim): bytes of scratch a sort of `count` keys needs; the sort itself
size_t rebuildSortKeysScratch(uint32_t count);
void launchRebuildSortKeys(void* dScratch, size_t scratchBytes, const uint64_t* dKeysIn, uint64_t* dKeysOut, uint32_t count, hipStream_t stream);

// Steps 5-6.  Lane i of launchRebuildTopology owns radix node i of leafCount - 1: dFirst[i] = start of its range, dKids[i] = its children
// (bit 31: a sorted position, otherwise a radix node), dParent[child radix node] = i | (left child ? bit 31 : 0); dParent[0] = 0.
// launchRebuildNumber: dPre[i] = preorder index.  launchRebuildNodes: the 64 B rows of the new tree, references set and boxes zero.
void launchRebuildTopology(const uint64_t* dSortedKeys, uint32_t leafCount, uint32_t* dFirst, uint2* dKids, uint32_t* dParent, hipStream_t stream);
void launchRebuildNumber(const uint32_t* dFirst, const uint32_t* dParent, uint32_t nodeCount, uint32_t* dPre, hipStream_t stream);
void launchRebuildNodes(const uint64_t* dSortedKeys, const uint32_t* dLeaves, const uint2* dKids, const uint32_t* dPre, uint32_t nodeCount,
                        float4* dBoxes, hipStream_t stream);

// Step 7.  One launch settles the nodes of height `k` (dHeights starts as kHeightUnknown everywhere); dIota[i] = i beside it in launch 0.
void launchRebuildHeights(const float4* dBoxes, uint32_t nodeCount, uint32_t k, uint8_t* dHeights, uint32_t* dIota, hipStream_t stream);
// the schedule: the stable sort of the node indices by height (rocprim), and where each height starts (dLevelOffsets[h], h <= height of node 0)
size_t rebuildSortScheduleScratch(uint32_t count);
void launchRebuildSchedule(void* dScratch, size_t scratchBytes, const uint8_t* dHeights, uint8_t* dHeightsSorted, const uint32_t* dIota,
                           uint32_t* dSchedule, uint32_t nodeCount, uint32_t* dLevelOffsets, hipStream_t stream);

// Step 10.  dDepth (bytes: 0 everywhere but dDepth[0] = 1) and dMarks (words, 0 everywhere): the launch of level `d` handles the wide
// roots of depth d: marks them, gives every internal child they keep depth d + 1 and sets dReached[d + 1] when there is one.
void launchRebuildWideMark(const uint4* dQnodes, uint32_t nodeCount, const float cell[3], uint32_t d, uint8_t* dDepth, uint32_t* dMarks,
                           uint32_t* dReached, hipStream_t stream);
size_t rebuildScanScratch(uint32_t count);
void launchRebuildWideScan(void* dScratch, size_t scratchBytes, const uint32_t* dMarks, uint32_t* dWideIndex, uint32_t nodeCount, hipStream_t stream);
// per wide root: the reference words (box words zero: k_dyn_wide fills them), the unused places, the wide-source table
void launchRebuildWideWrite(const uint4* dQnodes, uint32_t nodeCount, const float cell[3], const uint32_t* dMarks, const uint32_t* dWideIndex,
                            uint4* dWnodes, uint32_t* dWideSource, hipStream_t stream);

}  // namespace ptrk
