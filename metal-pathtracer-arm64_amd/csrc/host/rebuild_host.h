// The host half of include/ptr_rebuild.h that needs no device: the leaf table of a tree, the decisions of step 8, the figures an install
// changes, the SAH figure in float64 and the probe's tables.  Plain C++ (g++), so tools/rebuild_host_check.cpp runs it under sanitizers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bvh_builder.h"

namespace ptr {

// Step 1: the leaf references of `nodeCount` float nodes, ascending by (reference & kLeafTableKeyMask).
constexpr uint32_t kLeafTableKeyMask = 0x43FFFFFFu;
void BuildLeafTable(const float* nodes, uint32_t nodeCount, std::vector<uint32_t>& leaves);

// Step 8: what is wrong with a rebuilt tree of `levels` binary levels (and, with four-wide nodes, `wideDepth` wide levels), or "".
std::string RebuildDepthProblem(uint32_t levels, bool useWide, uint32_t wideDepth);

// Step 11: the figures of the scene that follow a tree of that shape, by the upload's own rules.
struct RebuildInstall {
    uint32_t maxDepth = 0;     // FlatBvh::maxDepth of such a tree: levels + 1
    uint32_t stackLimit = 0;   // SceneView::stackLimit
    uint32_t spillLevels = 0;  // stack levels beyond the LDS part
    uint64_t wideBytes = 0;
};
RebuildInstall PlanRebuildInstall(uint32_t levels, uint32_t wideCount, uint32_t wideDepth);

// the root box of the tree from node 0 (16 floats): the union of its children that exist
bool RootBoxOfNode(const float* node0, float lo[3], float hi[3]);

// the SAH figure of include/ptr_rebuild.h on the host, terms in node order
double TreeCost(const float* nodes, uint32_t nodeCount);
// the special cases the kernel does not see: true when `cost` is settled by node 0 alone (no nodes; a root whose only child is a leaf)
bool TreeCostOfNode0(const float* node0, uint32_t nodeCount, double& cost, double& rootHalfArea);

// "" or why `nodes` is no preorder array the builder's functions may walk
std::string NodeArrayProblem(const float* nodes, uint32_t nodeCount);

// ptr_debug_rebuild_tables: table `which` of include/ptr_rebuild.h as bytes; "" or the refusal
std::string RebuildTable(const float* nodes, uint32_t nodeCount, uint32_t which, std::vector<uint8_t>& out);

}  // namespace ptr
