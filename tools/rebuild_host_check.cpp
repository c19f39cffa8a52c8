// Host check of the rebuild above the leaves (include/ptr_rebuild.h): the leaf table of the upload's tree, every table of the probe
// (ptr::RebuildTable: schedule, level offsets, grid, QuantiseNode, BuildWideNodes(ByArea) with its source table and depth, the SAH figure,
// the depth decision) and the figures an install changes (ptr::PlanRebuildInstall), on scenes of 0 .. 20,000 random triangles beside a
// sphere and a rectangle, so that an address or undefined-behaviour sanitizer sees any step outside an array.  The device calls of a
// rebuild are left out: what is checked is everything the host decides about array sizes.  Also holds the probe's schedule and wide
// nodes to the builder's own, the leaf table to the tree (every leaf once, in key order), and a node array with a reference out of
// range to its refusal.  Build and run on the host only:
//   H=metal-pathtracer-arm64_amd/csrc/host; g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       -Iinclude -I$H -I$H/../kernels tools/rebuild_host_check.cpp $H/rebuild_host.cpp $H/scene_geometry.cpp $H/bvh_builder.cpp $H/knobs.cpp \
//       -o /tmp/rebuild_host_check && /tmp/rebuild_host_check
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "bvh_builder.h"
#include "bvh_layout.h"
#include "ptr_rebuild.h"
#include "rebuild_host.h"
#include "scene_geometry.h"
static int fail(const char* what) { std::printf("fail: %s\n", what); return 1; }
int main() {
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (int tris : {0, 1, 9, 500, 20000}) {
        std::vector<float> pos, nrm; std::vector<uint32_t> idx;
        for (int t = 0; t < tris; ++t) {
            float cx = u(rng) * 5, cy = u(rng) * 5, cz = u(rng) * 5;
            for (int c = 0; c < 3; ++c) {
                pos.insert(pos.end(), {cx + 0.1f * u(rng), cy + 0.1f * u(rng), cz + 0.1f * u(rng)});
                nrm.insert(nrm.end(), {0.f, 1.f, 0.f}); idx.push_back(3 * t + c);
            }
        }
        PtrMeshDesc mesh; std::memset(&mesh, 0, sizeof(mesh));
        mesh.positions = pos.data(); mesh.normals = nrm.data(); mesh.indices = idx.data();
        mesh.vertexCount = (uint32_t)pos.size() / 3; mesh.indexCount = (uint32_t)idx.size();
        for (int i = 0; i < 4; ++i) mesh.localToWorld[i * 5] = 1.f;
        PtrSphere sph; std::memset(&sph, 0, sizeof(sph)); sph.centerRadius[3] = 0.5f;
        PtrRect rect; std::memset(&rect, 0, sizeof(rect)); rect.edgeU[0] = 1; rect.edgeV[2] = 1; rect.normalAndPlane[1] = 1;
        PtrSceneDesc d; std::memset(&d, 0, sizeof(d));
        d.meshes = &mesh; d.meshCount = 1; d.spheres = &sph; d.sphereCount = 1; d.rects = &rect; d.rectCount = 1;
        ptr::SceneGeometry g; ptr::DynamicTables t; std::string err;
        if (!ptr::BuildSceneGeometry(d, 0, g, err, &t)) return fail(err.c_str());
        const ptr::FlatBvh& bvh = g.bvh;
        // step 1: every leaf of the tree once, ascending by key
        std::vector<uint32_t> leaves;
        ptr::BuildLeafTable(bvh.nodes.data(), bvh.nodeCount, leaves);
        if (leaves.size() != bvh.leafCount) return fail("leaf count");
        for (size_t i = 1; i < leaves.size(); ++i) {
            if ((leaves[i - 1] & ptr::kLeafTableKeyMask) >= (leaves[i] & ptr::kLeafTableKeyMask)) return fail("leaf order");
        }
        if (bvh.leafCount >= 2 && bvh.leafCount != bvh.nodeCount + 1) return fail("not a full binary tree");
        // the probe, every table, on the upload's own tree
        std::vector<uint8_t> bytes, schedule, wnodes, source;
        for (uint32_t which = 0; which <= PTR_REBUILD_TABLE_DEPTH_CHECK; ++which) {
            const std::string problem = ptr::RebuildTable(bvh.nodes.data(), bvh.nodeCount, which, bytes);
            if (!problem.empty()) return fail(problem.c_str());
            if (which == PTR_REBUILD_TABLE_SCHEDULE) schedule = bytes;
            if (which == PTR_REBUILD_TABLE_WNODES) wnodes = bytes;
            if (which == PTR_REBUILD_TABLE_WIDE_SOURCE) source = bytes;
            if (which == PTR_REBUILD_TABLE_QNODES && (bytes.size() != bvh.qnodes.size() * 4 || std::memcmp(bytes.data(), bvh.qnodes.data(), bytes.size()) != 0)) return fail("qnodes");
        }
        if (schedule.size() != t.schedule.size() * 4 || (schedule.size() && std::memcmp(schedule.data(), t.schedule.data(), schedule.size()) != 0)) return fail("schedule");
        std::unique_ptr<uint32_t[]> wide; uint32_t depth = 0; std::vector<uint32_t> src;
        const uint32_t wc = ptr::BuildWideNodes(bvh, ptr::WideCollapse::ByArea, wide, &depth, &src);
        if (wnodes.size() != (size_t)wc * 64 || (wc && std::memcmp(wnodes.data(), wide.get(), wnodes.size()) != 0)) return fail("wnodes");
        if (source.size() != (size_t)wc * 16 || (wc && std::memcmp(source.data(), src.data(), source.size()) != 0)) return fail("wide source");
        if (ptr::RebuildTable(bvh.nodes.data(), bvh.nodeCount, 99, bytes).empty()) return fail("table 99 accepted");
        // a reference past the array and one to an earlier node are refused, not walked
        if (bvh.nodeCount >= 3) {
            std::vector<float> bad(bvh.nodes);
            for (uint32_t ref : {bvh.nodeCount + 7u, 0u}) {
                std::memcpy(&bad[(size_t)(bvh.nodeCount - 1) * 16 + 3], &ref, 4);
                if (ptr::RebuildTable(bad.data(), bvh.nodeCount, PTR_REBUILD_TABLE_WNODES, bytes).empty()) return fail("bad reference accepted");
            }
        }
        // steps 8 and 11 for every shape a rebuild could report
        for (uint32_t levels = 1; levels < 64; ++levels) {
            for (uint32_t wideDepth : {0u, 1u, levels / 2 + 1, levels, 24u, 25u}) {
                const bool refused = !ptr::RebuildDepthProblem(levels, wideDepth > 0, wideDepth).empty();
                if (refused != (levels >= ptrk::kMaxTreeDepth || (wideDepth > 0 && 3 * wideDepth + 4 > ptrk::kTraversalStackDepth))) return fail("depth decision");
                if (refused) continue;
                const ptr::RebuildInstall p = ptr::PlanRebuildInstall(levels, wideDepth ? wc : 0, wideDepth);
                if (p.stackLimit > ptrk::kTraversalStackDepth || p.stackLimit < ptrk::kLdsStackLevels || p.spillLevels != p.stackLimit - ptrk::kLdsStackLevels) return fail("stack limit");
                if (p.stackLimit < std::min(ptrk::kTraversalStackDepth, levels + 1) || (wideDepth && p.stackLimit < 3 * wideDepth + 4)) return fail("stack need");
            }
        }
        std::printf("tris %d: nodes %u leaves %zu levels %zu wide %u cost %.6f ok\n", tris, bvh.nodeCount, leaves.size(), t.levelOffsets.size() - 1, wc,
                    ptr::TreeCost(bvh.nodes.data(), bvh.nodeCount));
    }
    return 0;
}
