// Host check of the dynamic-scene preparation (include/ptr_dynamic.h): BuildSceneGeometry with its dynamic tables, the wide-source table
// of BuildWideNodes under both collapses, the refit schedule and QuantiseNode, on scenes of 0 .. 20,000 random triangles beside a sphere, a
// rectangle and a mesh without triangles, so that an address or undefined-behaviour sanitizer sees any step outside an array.  Also
// holds every wide place to its source record and QuantiseNode to the builder's qnodes.  Build and run on the host only:
//   H=metal-pathtracer-arm64_amd/csrc/host; g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       -Iinclude -I$H -I$H/../kernels tools/dynamic_host_check.cpp $H/scene_geometry.cpp $H/bvh_builder.cpp $H/knobs.cpp \
//       -o /tmp/dynamic_host_check && /tmp/dynamic_host_check
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "scene_geometry.h"
#include "bvh_builder.h"
int main() {
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (int tris : {0, 1, 9, 500, 20000}) {
        std::vector<float> pos, nrm; std::vector<uint32_t> idx;
        for (int t = 0; t < tris; ++t) for (int c = 0; c < 3; ++c) {
            float cx = u(rng) * 5, cy = u(rng) * 5, cz = u(rng) * 5;
            pos.insert(pos.end(), {cx + 0.1f * u(rng), cy + 0.1f * u(rng), cz + 0.1f * u(rng)});
            nrm.insert(nrm.end(), {0.f, 1.f, 0.f}); idx.push_back(3 * t + c);
        }
        PtrMeshDesc mesh[2]; std::memset(mesh, 0, sizeof(mesh));
        for (int m = 0; m < 2; ++m) {
            mesh[m].positions = pos.data(); mesh[m].normals = nrm.data(); mesh[m].indices = idx.data();
            mesh[m].vertexCount = m == 0 ? (uint32_t)pos.size() / 3 : 0; mesh[m].indexCount = m == 0 ? (uint32_t)idx.size() : 0;
            for (int i = 0; i < 4; ++i) mesh[m].localToWorld[i * 5] = 1.f;
        }
        PtrSphere sph; std::memset(&sph, 0, sizeof(sph)); sph.centerRadius[3] = 0.5f;
        PtrRect rect; std::memset(&rect, 0, sizeof(rect)); rect.edgeU[0] = 1; rect.edgeV[2] = 1; rect.normalAndPlane[1] = 1;
        PtrSceneDesc d; std::memset(&d, 0, sizeof(d));
        d.meshes = mesh; d.meshCount = 2; d.spheres = &sph; d.sphereCount = 1; d.rects = &rect; d.rectCount = 1;
        ptr::SceneGeometry g; ptr::DynamicTables t; std::string err;
        if (!ptr::BuildSceneGeometry(d, 0, g, err, &t)) { std::printf("fail %s\n", err.c_str()); return 1; }
        std::unique_ptr<uint32_t[]> wide; uint32_t depth = 0;
        for (auto how : {ptr::WideCollapse::ByArea, ptr::WideCollapse::ByLevel}) {
            uint32_t wc = ptr::BuildWideNodes(g.bvh, how, wide, &depth, &t.wideSource);
            for (size_t i = 0; i < t.wideSource.size(); ++i) {
                uint32_t s = t.wideSource[i];
                if (s != ptr::kNoWideSource && (s >= g.bvh.nodeCount * 2 || std::memcmp(&wide[i * 4], &g.bvh.qnodes[(size_t)s * 4], 12) != 0)) { std::printf("bad source\n"); return 1; }
            }
            if (t.wideSource.size() != (size_t)wc * 4) return 1;
        }
        std::vector<uint32_t> q(8);
        for (uint32_t i = 0; i < g.bvh.nodeCount; ++i) {
            ptr::QuantiseNode(&g.bvh.nodes[(size_t)i * 16], g.bvh.gridOrigin, g.bvh.gridCell, q.data());
            if (std::memcmp(q.data(), &g.bvh.qnodes[(size_t)i * 8], 32) != 0) return 1;
        }
        std::printf("tris %d: nodes %u levels %zu meshTris %zu ok\n", tris, g.bvh.nodeCount, t.levelOffsets.size() - 1, t.meshTris.size());
    }
    return 0;
}
