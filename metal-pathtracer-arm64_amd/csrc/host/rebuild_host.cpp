// include/ptr_rebuild.h without a device (rebuild_host.h).
#include "rebuild_host.h"

#include <algorithm>
#include <cstring>
#include <memory>

#include "../kernels/bvh_grid.h"
#include "../kernels/bvh_layout.h"
#include "ptr_rebuild.h"

namespace ptr {

namespace {

inline uint32_t refOf(const float* nodes, uint32_t node, int slot) {
    uint32_t ref;
    std::memcpy(&ref, nodes + static_cast<size_t>(node) * 16u + (slot == 0 ? 3 : 7), 4);
    return ref;
}

inline double halfArea(const float* lo, const float* hi) {
    const double dx = static_cast<double>(hi[0]) - lo[0], dy = static_cast<double>(hi[1]) - lo[1], dz = static_cast<double>(hi[2]) - lo[2];
    return dx * dy + dy * dz + dz * dx;
}

template <typename T>
void put(std::vector<uint8_t>& out, const T* p, size_t n) {
    out.resize(n * sizeof(T));
    if (n) std::memcpy(out.data(), p, n * sizeof(T));
}

}  // namespace

void BuildLeafTable(const float* nodes, uint32_t nodeCount, std::vector<uint32_t>& leaves) {
    leaves.clear();
    for (uint32_t i = 0; i < nodeCount; ++i) {
        for (int s = 0; s < 2; ++s) {
            const uint32_t ref = refOf(nodes, i, s);
            if (ref != ptrk::kRefEmpty && (ref & ptrk::kRefLeafBit)) leaves.push_back(ref);
        }
    }
    std::sort(leaves.begin(), leaves.end(), [](uint32_t a, uint32_t b) { return (a & kLeafTableKeyMask) < (b & kLeafTableKeyMask); });
}

std::string RebuildDepthProblem(uint32_t levels, bool useWide, uint32_t wideDepth) {
    if (levels >= ptrk::kMaxTreeDepth) {
        return "the rebuilt tree would have " + std::to_string(levels) + " levels or more; the traversal stacks hold fewer than " +
               std::to_string(ptrk::kMaxTreeDepth);
    }
    if (useWide && 3u * wideDepth + 4u > ptrk::kTraversalStackDepth) {
        return "the rebuilt four-wide tree would have " + std::to_string(wideDepth) + " levels, more than the traversal stack holds";
    }
    return "";
}

RebuildInstall PlanRebuildInstall(uint32_t levels, uint32_t wideCount, uint32_t wideDepth) {
    RebuildInstall p;
    p.maxDepth = levels + 1u;
    const uint32_t wideLevels = wideCount > 0u ? wideDepth : 0u;
    const uint32_t stackNeed = std::min<uint32_t>(ptrk::kTraversalStackDepth, std::max(3u * wideLevels, p.maxDepth) + 4u);
    p.stackLimit = std::max(stackNeed, ptrk::kLdsStackLevels);
    p.spillLevels = p.stackLimit - ptrk::kLdsStackLevels;
    p.wideBytes = static_cast<uint64_t>(wideCount) * 64u;
    return p;
}

bool RootBoxOfNode(const float* node0, float lo[3], float hi[3]) {
    bool any = false;
    for (int c = 0; c < 2; ++c) {
        if (refOf(node0, 0, c) == ptrk::kRefEmpty) continue;
        const float* cl = node0 + c * 8;
        const float* ch = node0 + c * 8 + 4;
        for (int a = 0; a < 3; ++a) {
            lo[a] = any ? std::min(lo[a], cl[a]) : cl[a];
            hi[a] = any ? std::max(hi[a], ch[a]) : ch[a];
        }
        any = true;
    }
    return any;
}

bool TreeCostOfNode0(const float* node0, uint32_t nodeCount, double& cost, double& rootHalfArea) {
    cost = 0.0;
    rootHalfArea = 0.0;
    if (nodeCount == 0u) return true;
    float lo[3], hi[3];
    if (!RootBoxOfNode(node0, lo, hi)) return true;
    rootHalfArea = halfArea(lo, hi);
    const uint32_t r0 = refOf(node0, 0, 0), r1 = refOf(node0, 0, 1);
    if (nodeCount == 1u && r1 == ptrk::kRefEmpty && (r0 & ptrk::kRefLeafBit)) {
        cost = static_cast<double>(((r0 >> ptrk::kRefCountShift) & 0xFu) + 1u);
        return true;
    }
    return false;
}

double TreeCost(const float* nodes, uint32_t nodeCount) {
    double cost = 0.0, rootHalf = 0.0;
    if (TreeCostOfNode0(nodes, nodeCount, cost, rootHalf)) return cost;
    const double rootArea = std::max(rootHalf, 1e-30);
    cost = rootHalf / rootArea;
    for (uint32_t i = 0; i < nodeCount; ++i) {
        for (int s = 0; s < 2; ++s) {
            const uint32_t ref = refOf(nodes, i, s);
            if (ref == ptrk::kRefEmpty) continue;
            const float* b = nodes + static_cast<size_t>(i) * 16u + s * 8;
            const double weight = (ref & ptrk::kRefLeafBit) ? static_cast<double>(((ref >> ptrk::kRefCountShift) & 0xFu) + 1u) : 1.0;
            cost += halfArea(b, b + 4) / rootArea * weight;
        }
    }
    return cost;
}

std::string NodeArrayProblem(const float* nodes, uint32_t nodeCount) {
    for (uint32_t i = 0; i < nodeCount; ++i) {
        for (int s = 0; s < 2; ++s) {
            const uint32_t ref = refOf(nodes, i, s);
            if (ref == ptrk::kRefEmpty || (ref & ptrk::kRefLeafBit)) continue;
            if (ref <= i || ref >= nodeCount) {
                return "slot " + std::to_string(s) + " of node " + std::to_string(i) + " names node " + std::to_string(ref) + ", which is no later node of the array";
            }
        }
    }
    return "";
}

std::string RebuildTable(const float* nodes, uint32_t nodeCount, uint32_t which, std::vector<uint8_t>& out) {
    out.clear();
    if (which > PTR_REBUILD_TABLE_DEPTH_CHECK) return "no such table";
    const std::string problem = NodeArrayProblem(nodes, nodeCount);
    if (!problem.empty()) return problem;
    if (which == PTR_REBUILD_TABLE_SAH) {
        const double cost = TreeCost(nodes, nodeCount);
        put(out, &cost, 1);
        return "";
    }
    if (which == PTR_REBUILD_TABLE_LEAF_TABLE) {
        std::vector<uint32_t> leaves;
        BuildLeafTable(nodes, nodeCount, leaves);
        put(out, leaves.data(), leaves.size());
        return "";
    }
    FlatBvh bvh;
    bvh.nodeCount = nodeCount;
    bvh.nodes.assign(nodes, nodes + static_cast<size_t>(nodeCount) * 16u);
    std::vector<uint32_t> schedule, levelOffsets;
    BuildRefitSchedule(bvh, schedule, levelOffsets);
    if (which == PTR_REBUILD_TABLE_SCHEDULE) return put(out, schedule.data(), schedule.size()), "";
    if (which == PTR_REBUILD_TABLE_LEVEL_OFFSETS) return put(out, levelOffsets.data(), levelOffsets.size()), "";
    if (which == PTR_REBUILD_TABLE_DEPTH_CHECK) {
        const uint32_t levels = static_cast<uint32_t>(levelOffsets.size()) - 1u;
        put(out, &levels, 1);
        return RebuildDepthProblem(levels, false, 0u);
    }
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (nodeCount > 0u && RootBoxOfNode(nodes, lo, hi)) {
        for (int a = 0; a < 3; ++a) ptrk::gridAxis(lo[a], hi[a], bvh.gridOrigin[a], bvh.gridCell[a]);
    }
    if (which == PTR_REBUILD_TABLE_GRID) {
        float grid[6];
        std::memcpy(grid, bvh.gridOrigin, 12);
        std::memcpy(grid + 3, bvh.gridCell, 12);
        return put(out, grid, 6), "";
    }
    bvh.qnodes.assign(static_cast<size_t>(nodeCount) * 8u, 0u);
    for (uint32_t i = 0; i < nodeCount; ++i) QuantiseNode(nodes + static_cast<size_t>(i) * 16u, bvh.gridOrigin, bvh.gridCell, bvh.qnodes.data() + static_cast<size_t>(i) * 8u);
    if (which == PTR_REBUILD_TABLE_QNODES) return put(out, bvh.qnodes.data(), bvh.qnodes.size()), "";
    std::unique_ptr<uint32_t[]> wide;
    std::vector<uint32_t> source;
    uint32_t depth = 0;
    const uint32_t wideCount = BuildWideNodes(bvh, WideCollapse::ByArea, wide, &depth, &source);
    if (which == PTR_REBUILD_TABLE_WNODES) return put(out, wide.get(), static_cast<size_t>(wideCount) * 16u), "";
    if (which == PTR_REBUILD_TABLE_WIDE_SOURCE) return put(out, source.data(), wideCount > 0u ? source.size() : 0u), "";
    return put(out, &depth, 1), "";   // PTR_REBUILD_TABLE_WIDE_DEPTH
}

}  // namespace ptr
