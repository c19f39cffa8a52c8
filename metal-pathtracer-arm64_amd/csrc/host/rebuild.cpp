// include/ptr_rebuild.h on the device: ptr_scene_tree_cost, ptr_scene_rebuild_tree and their probes.  The kernels are in
// kernels/rebuild.hip (fit, quantiser and wide copy: kernels/dynamic.hip); what needs no device is in rebuild_host.cpp.  Compiled with
// hipcc (host code only), like dynamic.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "../kernels/bvh_grid.h"
#include "../kernels/dynamic.h"
#include "../kernels/rebuild.h"
#include "device_scene.h"
#include "dynamic_host.h"
#include "ptr_rebuild.h"
#include "rebuild_host.h"

using namespace ptrk;
using namespace ptrhost;

namespace {

float4* floatBoxes(PtrDeviceScene& ds) { return ds.view.useQuantized ? ds.dynamic->boxes.ptr : ds.nodes.ptr; }

RebuildState& stateOf(DynamicScene& dyn) {
    if (!dyn.rebuild) {
        auto st = std::make_unique<RebuildState>();
        for (hipEvent_t& e : st->events) HIP_CHECK(hipEventCreate(&e));
        dyn.rebuild = std::move(st);
    }
    return *dyn.rebuild;
}

template <typename T>
void swapBuffers(DeviceBuffer<T>& a, DeviceBuffer<T>& b) {
    std::swap(a.ptr, b.ptr);
    std::swap(a.count, b.count);
}

uint32_t costBlocks(uint32_t nodeCount) { return (nodeCount + kRebuildBlock - 1u) / kRebuildBlock; }

double sumInBlockOrder(const double* partials, uint32_t blocks) {
    double sum = 0.0;
    for (uint32_t b = 0; b < blocks; ++b) sum += partials[b];
    return sum;
}

// The cost of the tree in `boxes`: node 0 comes to the host first (the root area is a kernel argument), then the block sums.
double treeCostOf(DynamicScene& dyn, RebuildState& st, const float4* boxes, uint32_t nodeCount, hipStream_t stream) {
    if (nodeCount == 0u) return 0.0;
    const uint32_t blocks = costBlocks(nodeCount);
    char* pinned = static_cast<char*>(dyn.pinned.pinnedFor(64u + static_cast<size_t>(blocks) * sizeof(double)));
    HIP_CHECK(hipMemcpyAsync(pinned, boxes, 64u, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    double cost = 0.0, rootHalf = 0.0;
    if (ptr::TreeCostOfNode0(reinterpret_cast<const float*>(pinned), nodeCount, cost, rootHalf)) return cost;
    st.partials.ensure(static_cast<size_t>(blocks) * 2u);
    launchTreeCost(boxes, nodeCount, rootHalf, std::max(rootHalf, 1e-30), st.partials.ptr, stream);
    HIP_CHECK(hipMemcpyAsync(pinned + 64, st.partials.ptr, static_cast<size_t>(blocks) * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return sumInBlockOrder(reinterpret_cast<const double*>(pinned + 64), blocks);
}

void fillInfo(const PtrDeviceScene& ds, PtrRebuildInfo& info) {
    const DynamicScene& dyn = *ds.dynamic;
    info.nodes = dyn.nodeCount;
    info.levels = dyn.levelOffsets.size() - 1u;
    info.wideNodes = dyn.wideCount;
    info.wideDepth = ds.view.useWide ? ds.wideDepth : 0u;
    info.leaves = dyn.leafTable.size();
}

}  // namespace

namespace ptrhost {

std::string rebuildFlagsProblem(uint32_t flags) { return flags & ~static_cast<uint32_t>(PTR_REBUILD_KEEP_IF_BETTER) ? "unknown flag bits" : ""; }

std::string checkTreeCall(const PtrDeviceScene* scene, uint32_t flags) {
    if (!scene->dynamic) return "the scene is not dynamic (upload it with ptr_scene_upload_dynamic)";
    return rebuildFlagsProblem(flags);
}

double treeCost(PtrDeviceScene& ds, hipStream_t st) {
    DynamicScene& dyn = *ds.dynamic;
    return treeCostOf(dyn, stateOf(dyn), floatBoxes(ds), dyn.nodeCount, st);
}

void rebuildTree(const char* who, PtrDeviceScene& ds, uint32_t flags, hipStream_t stream, PtrRebuildInfo& info) {
    const auto t0 = std::chrono::steady_clock::now();
    DynamicScene& dyn = *ds.dynamic;
    SceneView& v = ds.view;
    RebuildState& st = stateOf(dyn);
    std::memset(&info, 0, sizeof(info));
    const uint32_t nodeCount = dyn.nodeCount;
    const uint32_t leafCount = static_cast<uint32_t>(dyn.leafTable.size());
    auto finish = [&] {
        fillInfo(ds, info);
        info.totalSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    info.costBefore = info.costAfter = treeCostOf(dyn, st, floatBoxes(ds), nodeCount, stream);
    if (nodeCount == 0u || leafCount < 2u) return finish();   // nothing above the leaves to rebuild
    if (leafCount != nodeCount + 1u) throw HipError{std::string(who) + ": the scene's tree is not a full binary tree over its leaves"};

    // the second set of arrays and the scratch, once
    const size_t n = nodeCount;
    st.boxes.ensure(n * 4u);
    st.schedule.ensure(n);
    if (v.useQuantized) st.qnodes.ensure(n * 2u);
    if (st.leaves.count < leafCount) st.leaves.upload(dyn.leafTable.data(), leafCount);
    st.keys.ensure(leafCount), st.sortedKeys.ensure(leafCount);
    st.first.ensure(n), st.parent.ensure(n), st.pre.ensure(n), st.iota.ensure(n), st.kids.ensure(n);
    st.heights.ensure(n), st.sortedHeights.ensure(n);
    st.small.ensure(128u);
    st.partials.ensure(static_cast<size_t>(costBlocks(nodeCount)) * 2u);
    const size_t keyScratch = rebuildSortKeysScratch(leafCount), scheduleScratch = rebuildSortScheduleScratch(nodeCount);
    size_t scanScratch = 0;
    if (v.useWide) {
        st.depth.ensure(n), st.marks.ensure(n), st.wideIndex.ensure(n);
        scanScratch = rebuildScanScratch(nodeCount);
    }
    const size_t scratchBytes = std::max(std::max(keyScratch, scheduleScratch), scanScratch);
    st.sortScratch.ensure(std::max<size_t>(scratchBytes, 16u));

    // steps 2-4: the root box of the current tree is in the pinned buffer (treeCostOf read node 0)
    float rootLo[3] = {0, 0, 0}, rootHi[3] = {0, 0, 0};
    ptr::RootBoxOfNode(static_cast<const float*>(dyn.pinned.ptr), rootLo, rootHi);
    HIP_CHECK(hipEventRecord(st.events[0], stream));
    launchRebuildKeys(st.leaves.ptr, leafCount, dyn.triBounds.ptr, dyn.sphereBounds.ptr, rootLo, rootHi, st.keys.ptr, stream);
    launchRebuildSortKeys(st.sortScratch.ptr, keyScratch, st.keys.ptr, st.sortedKeys.ptr, leafCount, stream);
    HIP_CHECK(hipEventRecord(st.events[1], stream));
    // steps 5-6
    launchRebuildTopology(st.sortedKeys.ptr, leafCount, st.first.ptr, st.kids.ptr, st.parent.ptr, stream);
    launchRebuildNumber(st.first.ptr, st.parent.ptr, nodeCount, st.pre.ptr, stream);
    launchRebuildNodes(st.sortedKeys.ptr, st.leaves.ptr, st.kids.ptr, st.pre.ptr, nodeCount, st.boxes.ptr, stream);
    HIP_CHECK(hipEventRecord(st.events[2], stream));
    // steps 7-8: launch k settles height k; a root still unknown after kMaxTreeDepth - 1 launches is too deep
    HIP_CHECK(hipMemsetAsync(st.heights.ptr, kHeightUnknown, n, stream));
    HIP_CHECK(hipMemsetAsync(st.small.ptr, 0, 128u * sizeof(uint32_t), stream));
    for (uint32_t k = 0; k + 1u < kMaxTreeDepth; ++k) launchRebuildHeights(st.boxes.ptr, nodeCount, k, st.heights.ptr, st.iota.ptr, stream);
    uint8_t* pinnedBytes = static_cast<uint8_t*>(dyn.pinned.pinnedFor(64u + static_cast<size_t>(costBlocks(nodeCount)) * sizeof(double) + 1024u));
    HIP_CHECK(hipMemcpyAsync(pinnedBytes, st.heights.ptr, 1u, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint32_t levels = pinnedBytes[0] == kHeightUnknown ? kMaxTreeDepth : pinnedBytes[0] + 1u;
    std::string problem = ptr::RebuildDepthProblem(levels, false, 0u);
    if (!problem.empty()) throw Refused{std::string(who) + ": " + problem};
    launchRebuildSchedule(st.sortScratch.ptr, scheduleScratch, st.heights.ptr, st.sortedHeights.ptr, st.iota.ptr, st.schedule.ptr, nodeCount, st.small.ptr, stream);
    uint32_t* pinnedWords = reinterpret_cast<uint32_t*>(pinnedBytes);
    HIP_CHECK(hipMemcpyAsync(pinnedWords, st.small.ptr, levels * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    st.levelOffsets.assign(pinnedWords, pinnedWords + levels);
    st.levelOffsets.push_back(nodeCount);
    for (uint32_t l = 0; l < levels; ++l) {
        launchDynRefitLevel(st.boxes.ptr, st.schedule.ptr + st.levelOffsets[l], st.levelOffsets[l + 1u] - st.levelOffsets[l], dyn.triBounds.ptr,
                            dyn.sphereBounds.ptr, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[3], stream));
    info.costAfter = treeCostOf(dyn, st, st.boxes.ptr, nodeCount, stream);   // (leaves node 0 of the new tree in the pinned buffer)
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, st.events[0], st.events[1]));
    info.keysSortMs = ms;
    HIP_CHECK(hipEventElapsedTime(&ms, st.events[1], st.events[2]));
    info.topologyMs = ms;
    HIP_CHECK(hipEventElapsedTime(&ms, st.events[2], st.events[3]));
    info.fitMs = ms;
    if ((flags & PTR_REBUILD_KEEP_IF_BETTER) && !(info.costAfter < info.costBefore)) return finish();

    // step 9: the grid of the new root box (the same box: min and max do not depend on the order of the union)
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, origin[3], cell[3];
    ptr::RootBoxOfNode(static_cast<const float*>(dyn.pinned.ptr), lo, hi);
    for (int a = 0; a < 3; ++a) gridAxis(lo[a], hi[a], origin[a], cell[a]);
    if (v.useQuantized) launchDynQuantise(st.boxes.ptr, st.qnodes.ptr, nodeCount, origin, cell, stream);
    HIP_CHECK(hipEventRecord(st.events[4], stream));
    // step 10
    uint32_t wideCount = 0, wideDepth = 0;
    if (v.useWide) {
        uint32_t* reached = st.small.ptr + 64;
        HIP_CHECK(hipMemsetAsync(st.depth.ptr, 0, n, stream));
        HIP_CHECK(hipMemsetAsync(st.depth.ptr, 1, 1u, stream));
        HIP_CHECK(hipMemsetAsync(st.marks.ptr, 0, n * sizeof(uint32_t), stream));
        for (uint32_t d = 1; d <= levels; ++d) launchRebuildWideMark(st.qnodes.ptr, nodeCount, cell, d, st.depth.ptr, st.marks.ptr, reached, stream);
        launchRebuildWideScan(st.sortScratch.ptr, scanScratch, st.marks.ptr, st.wideIndex.ptr, nodeCount, stream);
        pinnedWords = static_cast<uint32_t*>(dyn.pinned.pinnedFor(1024u));
        HIP_CHECK(hipMemcpyAsync(pinnedWords, reached, 64u * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(pinnedWords + 64, st.wideIndex.ptr + (n - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(pinnedWords + 65, st.marks.ptr + (n - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        wideCount = pinnedWords[64] + pinnedWords[65];
        wideDepth = 1u;
        for (uint32_t d = 2; d < 64u; ++d) {
            if (pinnedWords[d]) wideDepth = d;
        }
        problem = ptr::RebuildDepthProblem(levels, true, wideDepth);
        if (!problem.empty()) throw Refused{std::string(who) + ": " + problem};
        if (static_cast<uint64_t>(wideCount) * 64u > 0xFFFFFFFFull) throw HipError{std::string(who) + ": the four-wide nodes exceed the 4 GiB node array limit"};
        st.wnodes.ensure(static_cast<size_t>(wideCount) * 4u);
        st.wideSource.ensure(static_cast<size_t>(wideCount) * 4u);
        launchRebuildWideWrite(st.qnodes.ptr, nodeCount, cell, st.marks.ptr, st.wideIndex.ptr, st.wnodes.ptr, st.wideSource.ptr, stream);
        launchDynWide(st.qnodes.ptr, st.wnodes.ptr, st.wideSource.ptr, wideCount * 4u, stream);
    }
    HIP_CHECK(hipEventRecord(st.events[5], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipEventElapsedTime(&ms, st.events[3], st.events[4]));
    info.quantiseMs = ms;
    HIP_CHECK(hipEventElapsedTime(&ms, st.events[4], st.events[5]));
    info.wideMs = ms;

    // step 11: the sets change places; what described the old tree now describes the new one
    const ptr::RebuildInstall plan = ptr::PlanRebuildInstall(levels, wideCount, wideDepth);
    const uint32_t oldSpillLevels = ds.spillLevels;
    ds.spillLevels = plan.spillLevels;
    if (plan.spillLevels > oldSpillLevels) {
        ds.spill.ensure(std::max<size_t>(static_cast<size_t>(ds.spillLevels) * ds.traceGrid * kTraceGridUnit * ds.maxPoolGroups() * 2u, 1u));
    }
    if (v.useQuantized) {
        swapBuffers(dyn.boxes, st.boxes);
        swapBuffers(ds.qnodes, st.qnodes);
        v.qnodes = ds.qnodes.ptr;
    } else {
        swapBuffers(ds.nodes, st.boxes);
        v.nodes = ds.nodes.ptr;
    }
    if (v.useWide) {
        swapBuffers(ds.wnodes, st.wnodes);
        swapBuffers(dyn.wideSource, st.wideSource);
        v.wnodes = ds.wnodes.ptr;
        v.wideBytes = static_cast<uint32_t>(plan.wideBytes);
        dyn.wideCount = wideCount;
        ds.wideDepth = wideDepth;
    }
    swapBuffers(dyn.schedule, st.schedule);
    dyn.levelOffsets.swap(st.levelOffsets);
    for (int a = 0; a < 3; ++a) {
        v.gridOrigin[a] = origin[a], v.gridCell[a] = cell[a];
        v.gridInvCell[a] = 1.0f / cell[a];
    }
    v.stackLimit = plan.stackLimit;
    ds.info[4] = plan.maxDepth;
    ds.info[6] = static_cast<uint64_t>(info.costAfter * 1000.0);
    info.installed = 1u;
    finish();
}

}  // namespace ptrhost

extern "C" {

int ptr_scene_tree_cost(PtrDeviceScene* scene, void* stream, double* cost, char* err, size_t err_cap) {
    const char* who = "ptr_scene_tree_cost";
    if (!scene || !cost) return nullArgument(who, err, err_cap);
    const std::string problem = checkTreeCall(scene, 0u);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    return deviceCall(who, scene, true, err, err_cap, [&] { *cost = treeCost(*scene, static_cast<hipStream_t>(stream)); });
}

int ptr_scene_rebuild_tree(PtrDeviceScene* scene, uint32_t flags, void* stream, PtrRebuildInfo* info, char* err, size_t err_cap) {
    const char* who = "ptr_scene_rebuild_tree";
    if (!scene) return nullArgument(who, err, err_cap);
    const std::string problem = checkTreeCall(scene, flags);
    if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
    return deviceCall(who, scene, true, err, err_cap, [&] {
        PtrRebuildInfo local;
        rebuildTree(who, *scene, flags, static_cast<hipStream_t>(stream), local);
        if (info) *info = local;
    });
}

int ptr_debug_rebuild_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out) {
    if (!scene || !size_out || !scene->dynamic) return 1;
    const PtrDeviceScene& ds = *scene;
    const DynamicScene& dyn = *ds.dynamic;
    const uint32_t levels = static_cast<uint32_t>(dyn.levelOffsets.size()) - 1u;
    const uint32_t infoWords[6] = {dyn.nodeCount, levels, dyn.wideCount, ds.view.useWide ? ds.wideDepth : 0u, ds.view.stackLimit,
                                   static_cast<uint32_t>(dyn.leafTable.size())};
    const uint64_t pointers[3] = {reinterpret_cast<uintptr_t>(ds.view.nodes), reinterpret_cast<uintptr_t>(ds.view.qnodes), reinterpret_cast<uintptr_t>(ds.view.wnodes)};
    const void* host = nullptr;
    const void* device = nullptr;
    uint64_t bytes = 0;
    switch (which) {
        case PTR_REBUILD_ARRAY_SCHEDULE: device = dyn.schedule.ptr, bytes = static_cast<uint64_t>(dyn.nodeCount) * 4u; break;
        case PTR_REBUILD_ARRAY_LEVEL_OFFSETS: host = dyn.levelOffsets.data(), bytes = dyn.levelOffsets.size() * 4u; break;
        case PTR_REBUILD_ARRAY_WIDE_SOURCE: device = dyn.wideSource.ptr, bytes = ds.view.useWide ? static_cast<uint64_t>(dyn.wideCount) * 16u : 0u; break;
        case PTR_REBUILD_ARRAY_INFO: host = infoWords, bytes = sizeof(infoWords); break;
        case PTR_REBUILD_ARRAY_LEAF_TABLE: host = dyn.leafTable.data(), bytes = dyn.leafTable.size() * 4u; break;
        case PTR_REBUILD_ARRAY_POINTERS: host = pointers, bytes = sizeof(pointers); break;
        default: return 1;
    }
    return probeArrayTail(ds.device, host ? host : device, host != nullptr, bytes, out, cap_bytes, size_out);
}

int ptr_debug_rebuild_tables(const float* nodes, uint32_t nodeCount, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err,
                             size_t err_cap) {
    const char* who = "ptr_debug_rebuild_tables";
    if (!size_out || (!nodes && nodeCount > 0u)) return nullArgument(who, err, err_cap);
    try {
        std::vector<uint8_t> bytes;
        const std::string problem = ptr::RebuildTable(nodes, nodeCount, which, bytes);
        *size_out = bytes.size();
        if (!problem.empty()) return refuse(err, err_cap, std::string(who) + ": " + problem);
        if (!out) return 0;
        if (cap_bytes < bytes.size()) return refuse(err, err_cap, std::string(who) + ": the buffer is too small");
        if (!bytes.empty()) std::memcpy(out, bytes.data(), bytes.size());
        return 0;
    }
    PTR_CATCH_ALL(err, err_cap)
}

}  // extern "C"
