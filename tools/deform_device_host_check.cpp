// A stand-alone check of the host side of include/ptr_deform_device.h, meant to be built with sanitizers and run on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -pthread -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host \
//       -Imetal-pathtracer-arm64_amd/csrc/kernels tools/deform_device_host_check.cpp metal-pathtracer-arm64_amd/csrc/host/scene_geometry.cpp \
//       metal-pathtracer-arm64_amd/csrc/host/bvh_builder.cpp metal-pathtracer-arm64_amd/csrc/host/knobs.cpp -o /tmp/deform_device_host_check
//
// For scenes of 0 to 20,000 mesh triangles in two meshes, and a third mesh that has vertices and no triangle, it runs the preparation of a
// dynamic scene with PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS (BuildSceneGeometry) and checks every
// entry of every mesh's vertex adjacency against the description: the row offsets, that a vertex's entries are triangles in ascending
// order, and that each triangle is there once per corner that names the vertex.  The last vertex of every mesh is named by no triangle;
// the first triangle of the second mesh names one vertex three times, its second names one twice.  Prints one line per scene; exits 1 on
// the first difference.  No GPU, no HIP.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "scene_geometry.h"

namespace {

struct Scene {
    std::vector<float> pos[3], nrm[3];
    std::vector<uint32_t> idx[3];
    std::vector<PtrMeshDesc> meshes;
    std::vector<PtrMaterial> materials;
    PtrSceneDesc desc;
};

void makeScene(uint32_t triangles, Scene& s) {
    std::mt19937 rng(triangles * 2654435761u + 29u);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const uint32_t split[3] = {triangles / 3u, triangles - triangles / 3u, 0u};
    s.meshes.assign(3, PtrMeshDesc{});
    for (int m = 0; m < 3; ++m) {
        const uint32_t verts = m == 2 ? 5u : (split[m] ? split[m] / 2u + 3u : 0u);   // shared vertices; the last one stays unreferenced
        s.pos[m].resize(static_cast<size_t>(verts) * 3u), s.nrm[m].resize(static_cast<size_t>(verts) * 3u);
        for (float& f : s.pos[m]) f = uni(rng) * 5.0f;
        for (float& f : s.nrm[m]) f = uni(rng);
        s.idx[m].resize(static_cast<size_t>(split[m]) * 3u);
        for (uint32_t& i : s.idx[m]) i = rng() % (verts - 1u);
        if (m == 1 && split[m] >= 1u) s.idx[m][0] = s.idx[m][1] = s.idx[m][2] = 1u;
        if (m == 1 && split[m] >= 2u) s.idx[m][3] = s.idx[m][5] = 0u;
        PtrMeshDesc& d = s.meshes[m];
        d.positions = s.pos[m].data(), d.normals = s.nrm[m].data(), d.indices = s.idx[m].data();
        d.vertexCount = verts, d.indexCount = split[m] * 3u;
        const float l2w[16] = {1.1f, 0.1f, 0, 0, -0.2f, 0.9f, 0.1f, 0, 0, 0.3f, m ? -1.2f : 1.2f, 0, 3.0f * m, 0.5f, -1, 1};
        std::memcpy(d.localToWorld, l2w, sizeof(l2w));
        d.materialIndex = 0;
    }
    s.materials.assign(1, PtrMaterial{});
    s.desc = PtrSceneDesc{};
    s.desc.meshes = s.meshes.data(), s.desc.meshCount = 3;
    s.desc.materials = s.materials.data(), s.desc.materialCount = 1;
}

bool fail(uint32_t triangles, const char* what) {
    std::printf("%u triangles: %s\n", triangles, what);
    return false;
}

// one mesh's adjacency against its index array
bool checkMesh(uint32_t triangles, const uint32_t* offsets, size_t offsetCount, const uint32_t* entries, size_t entryCount, const std::vector<uint32_t>& idx,
               uint32_t verts) {
    if (offsetCount != static_cast<size_t>(verts) + 1u || entryCount != idx.size()) return fail(triangles, "adjacency size");
    if (offsets[0] != 0u || offsets[verts] != entryCount) return fail(triangles, "first or last row offset");
    std::vector<uint32_t> seen(idx.size() / 3u, 0u);   // corners of each triangle found in the rows
    for (uint32_t v = 0; v < verts; ++v) {
        if (offsets[v + 1u] < offsets[v]) return fail(triangles, "row offsets decrease");
        for (uint32_t e = offsets[v]; e < offsets[v + 1u]; ++e) {
            const uint32_t t = entries[e];
            if (t >= seen.size()) return fail(triangles, "entry names no triangle");
            if (e > offsets[v] && entries[e - 1u] > t) return fail(triangles, "entries of a vertex not in ascending triangle order");
            uint32_t named = 0, before = 0;
            for (int c = 0; c < 3; ++c) named += idx[static_cast<size_t>(t) * 3u + c] == v ? 1u : 0u;
            for (uint32_t b = offsets[v]; b < e; ++b) before += entries[b] == t ? 1u : 0u;
            if (before >= named) return fail(triangles, "a triangle is in the row of a vertex more often than it names it");
            ++seen[t];
        }
    }
    for (uint32_t n : seen) {
        if (n != 3u) return fail(triangles, "a corner is missing from the rows");
    }
    if (verts > 0u && offsets[verts] != offsets[verts - 1u]) return fail(triangles, "the unreferenced vertex has entries");
    return true;
}

bool check(uint32_t triangles, const Scene& s) {
    ptr::SceneGeometry geo;
    ptr::DynamicTables t;
    t.flags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES | PTR_DYNAMIC_VERTEX_NORMALS;
    std::string error;
    if (!ptr::BuildSceneGeometry(s.desc, 0, geo, error, &t)) return fail(triangles, error.c_str());
    if (t.adjBase.size() != 4u || t.adjBase[0] != 0u || t.adjBase[3] != t.adjOffsets.size() || t.adjEntries.size() != t.meshCorners.size()) {
        return fail(triangles, "adjacency bases");
    }
    for (uint32_t m = 0; m < 3; ++m) {
        const size_t first = static_cast<size_t>(t.meshTriOffsets[m]) * 3u, count = static_cast<size_t>(t.meshTriOffsets[m + 1u]) * 3u - first;
        if (!checkMesh(triangles, t.adjOffsets.data() + t.adjBase[m], static_cast<size_t>(t.adjBase[m + 1u] - t.adjBase[m]), t.adjEntries.data() + first, count,
                       s.idx[m], s.meshes[m].vertexCount)) {
            return false;
        }
        // an entry reaches its triangle's indices through the corner table, which is in the description's order
        if (count && std::memcmp(&t.meshCorners[first], s.idx[m].data(), count * 4u) != 0) return fail(triangles, "corner table order");
    }
    // without the flag the tables stay empty and the others are what they were
    ptr::SceneGeometry geo3;
    ptr::DynamicTables t3;
    t3.flags = PTR_DYNAMIC_DEFORMABLE | PTR_DYNAMIC_PRIMITIVES;
    if (!ptr::BuildSceneGeometry(s.desc, 0, geo3, error, &t3)) return fail(triangles, error.c_str());
    if (!t3.adjOffsets.empty() || !t3.adjEntries.empty() || !t3.adjBase.empty()) return fail(triangles, "adjacency without its flag");
    if (t3.meshCorners != t.meshCorners || t3.meshTris != t.meshTris || t3.objPos != t.objPos || t3.objNrm != t.objNrm || t3.triBounds != t.triBounds ||
        t3.schedule != t.schedule || geo3.triData != geo.triData) {
        return fail(triangles, "the flag changed another table");
    }
    return true;
}

}  // namespace

int main() {
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 9u, 255u, 256u, 257u, 1000u, 4097u, 20000u};
    for (uint32_t triangles : sizes) {
        Scene s;
        makeScene(triangles, s);
        if (!check(triangles, s)) return 1;
        std::printf("%u triangles: ok\n", triangles);
    }
    // the function alone, on the smallest inputs: no vertex, one vertex named three times
    std::vector<uint32_t> offsets, entries;
    ptr::BuildVertexAdjacency(nullptr, 0, 0, offsets, entries);
    if (offsets.size() != 1u || offsets[0] != 0u || !entries.empty()) return fail(0, "empty mesh") ? 0 : 1;
    const uint32_t one[3] = {0u, 0u, 0u};
    ptr::BuildVertexAdjacency(one, 1, 1, offsets, entries);
    if (offsets != std::vector<uint32_t>{0u, 3u} || entries != std::vector<uint32_t>{0u, 0u, 0u}) return fail(1, "one vertex named three times") ? 0 : 1;
    std::printf("single calls: ok\n");
    return 0;
}
