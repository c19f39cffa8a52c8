// A stand-alone check of the host side of include/ptr_deform.h, meant to be built with sanitizers and run on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -Iinclude -Imetal-pathtracer-arm64_amd/csrc/host \
//       -Imetal-pathtracer-arm64_amd/csrc/kernels tools/dynamic_deform_host_check.cpp metal-pathtracer-arm64_amd/csrc/host/scene_geometry.cpp \
//       metal-pathtracer-arm64_amd/csrc/host/bvh_builder.cpp metal-pathtracer-arm64_amd/csrc/host/knobs.cpp -o /tmp/dynamic_deform_host_check
//
// For scenes of 0 to 20,000 mesh triangles in two meshes, three rectangles and two spheres it runs the preparation of a dynamic scene with
// both flags (BuildSceneGeometry), checks the tables the flags add against the description (the corner table, the sphere map, the
// rectangle map) and holds the row writers the update calls share with the upload against the preparation's own rows, before and after
// moving every rectangle and sphere.  Prints one line per scene; exits 1 on the first difference.  No GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "scene_geometry.h"

namespace {

struct Scene {
    std::vector<float> pos[2], nrm[2];
    std::vector<uint32_t> idx[2];
    std::vector<PtrMeshDesc> meshes;
    std::vector<PtrRect> rects;
    std::vector<PtrSphere> spheres;
    std::vector<PtrMaterial> materials;
    PtrSceneDesc desc;
};

void setRect(PtrRect& r, float cx, float cy, float cz, float ux, float uy, float uz, float vx, float vy, float vz, float nx, float ny, float nz) {
    const float c[4] = {cx, cy, cz, 0.0f}, u[4] = {ux, uy, uz, 1.0f / (ux * ux + uy * uy + uz * uz)}, v[4] = {vx, vy, vz, 1.0f / (vx * vx + vy * vy + vz * vz)};
    const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
    const float n[4] = {nx / len, ny / len, nz / len, (nx * cx + ny * cy + nz * cz) / len};
    std::memcpy(r.corner, c, 16), std::memcpy(r.edgeU, u, 16), std::memcpy(r.edgeV, v, 16), std::memcpy(r.normalAndPlane, n, 16);
}

void makeScene(uint32_t triangles, Scene& s) {
    std::mt19937 rng(triangles * 2654435761u + 17u);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const uint32_t split[2] = {triangles / 3u, triangles - triangles / 3u};
    s.meshes.assign(2, PtrMeshDesc{});
    for (int m = 0; m < 2; ++m) {
        const uint32_t verts = split[m] ? split[m] / 2u + 3u : 0u;   // shared vertices
        s.pos[m].resize(static_cast<size_t>(verts) * 3u), s.nrm[m].resize(static_cast<size_t>(verts) * 3u);
        for (float& f : s.pos[m]) f = uni(rng) * 5.0f;
        for (float& f : s.nrm[m]) f = uni(rng);
        s.idx[m].resize(static_cast<size_t>(split[m]) * 3u);
        for (uint32_t& i : s.idx[m]) i = verts ? rng() % verts : 0u;
        PtrMeshDesc& d = s.meshes[m];
        d.positions = s.pos[m].data(), d.normals = s.nrm[m].data(), d.indices = s.idx[m].data();
        d.vertexCount = verts, d.indexCount = split[m] * 3u;
        const float l2w[16] = {1.1f, 0.1f, 0, 0, -0.2f, 0.9f, 0.1f, 0, 0, 0.3f, m ? -1.2f : 1.2f, 0, 3.0f * m, 0.5f, -1, 1};
        std::memcpy(d.localToWorld, l2w, sizeof(l2w));
        d.materialIndex = 0;
    }
    s.materials.assign(2, PtrMaterial{});
    s.materials[1].typeEta[0] = static_cast<float>(PTR_MAT_DIFFUSE_LIGHT);
    s.materials[1].emission[0] = 5.0f, s.materials[1].emission[1] = 4.0f, s.materials[1].emission[2] = 3.0f;
    s.rects.assign(3, PtrRect{});
    setRect(s.rects[0], -8, -6, -8, 16, 0, 0, 0, 0, 16, 0, 1, 0);
    setRect(s.rects[1], -1, 7, -1, 2, 0, 0, 0, 0, 2, 0, -1, 0);   // cross(U, V) = -y: same winding as the normal
    setRect(s.rects[2], 6, -2, 0, 0, 3, 0, 0, 0, 3, -1, 0, 0);   // cross(U, V) = +x against a -x normal: flipped
    s.rects[1].materialTwoSided[0] = 1;
    s.rects[2].materialTwoSided[0] = 1, s.rects[2].materialTwoSided[1] = 1;
    s.spheres.assign(2, PtrSphere{});
    const float a[4] = {2, 1, -3, 0.7f}, b[4] = {-4, 0, 2, -1.5f};
    std::memcpy(s.spheres[0].centerRadius, a, 16), std::memcpy(s.spheres[1].centerRadius, b, 16);
    s.desc = PtrSceneDesc{};
    s.desc.meshes = s.meshes.data(), s.desc.meshCount = 2;
    s.desc.rects = s.rects.data(), s.desc.rectCount = 3;
    s.desc.spheres = s.spheres.data(), s.desc.sphereCount = 2;
    s.desc.materials = s.materials.data(), s.desc.materialCount = 2;
}

bool fail(uint32_t triangles, const char* what) {
    std::printf("%u triangles: %s\n", triangles, what);
    return false;
}

// the preparation's rows of every rectangle and sphere equal the row writers', and the new tables name what they should
bool check(uint32_t triangles, const Scene& s) {
    ptr::SceneGeometry geo;
    ptr::DynamicTables t;
    t.flags = 3u;
    std::string error;
    if (!ptr::BuildSceneGeometry(s.desc, 0, geo, error, &t)) return fail(triangles, error.c_str());
    if (t.meshCorners.size() != t.meshTris.size() * 3u || t.meshTris.size() != triangles) return fail(triangles, "corner table size");
    for (uint32_t m = 0; m < 2; ++m) {
        if (t.meshVertexCount[m] != s.meshes[m].vertexCount) return fail(triangles, "vertex count");
        for (uint32_t e = t.meshTriOffsets[m]; e < t.meshTriOffsets[m + 1]; ++e) {
            uint32_t meta[2];
            std::memcpy(&meta[0], &geo.triData[static_cast<size_t>(t.meshTris[e]) * 12u + 7u], 4);
            std::memcpy(&meta[1], &geo.triData[static_cast<size_t>(t.meshTris[e]) * 12u + 11u], 4);
            if ((meta[0] >> 30) != 0u || (meta[0] & 0x3FFFFFFu) != m) return fail(triangles, "mesh list names another mesh's triangle");
            if (std::memcmp(&t.meshCorners[static_cast<size_t>(e) * 3u], &s.idx[m][static_cast<size_t>(meta[1]) * 3u], 12) != 0) return fail(triangles, "corner table");
        }
    }
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t slot = t.sphereLeaf[i];
        float row[4];
        ptr::BuildPrim prim{};
        ptr::WriteSphere(s.spheres[i], row, prim);
        if (slot >= 2u || geo.sphereInfo[slot * 2u] != i || std::memcmp(row, &geo.sphereData[slot * 4u], 16) != 0) return fail(triangles, "sphere row");
        if (std::memcmp(prim.lo, &t.sphereBounds[slot * 8u], 12) != 0 || std::memcmp(prim.hi, &t.sphereBounds[slot * 8u + 4u], 12) != 0) return fail(triangles, "sphere bounds");
    }
    for (uint32_t i = 0; i < 3; ++i) {
        float tri[2][12], nrm[2][12], row[20], light[ptr::kRectLightFloats];
        ptr::BuildPrim half[2];
        ptr::WriteRectTriangles(s.rects[i], i, t.rectShadeKey[i], tri, nrm, half);
        for (int h = 0; h < 2; ++h) {
            const size_t k = geo.rectTriLeaf[i * 2u + h];
            if (k >= geo.triCount) return fail(triangles, "rectangle map");
            if (std::memcmp(tri[h], &geo.triData[k * 12u], 48) != 0 || std::memcmp(nrm[h], &geo.triNormals[k * 12u], 48) != 0) return fail(triangles, "rectangle triangle rows");
            if (std::memcmp(half[h].lo, &t.triBounds[k * 8u], 12) != 0 || std::memcmp(half[h].hi, &t.triBounds[k * 8u + 4u], 12) != 0) return fail(triangles, "rectangle bounds");
        }
        ptr::WriteRectRow(s.rects[i], row);
        if (std::memcmp(row, &s.rects[i], 80) != 0) return fail(triangles, "rects row");
        ptr::WriteRectLightRow(s.rects[i], i, s.materials[1].emission, tri[0], tri[1], light);
        uint32_t index;
        std::memcpy(&index, &light[11], 4);
        if (index != i || light[15] != 1.0f || std::memcmp(&light[20], tri[0], 48) != 0 || std::memcmp(&light[32], tri[1], 48) != 0) return fail(triangles, "light row");
        ptr::WriteRectLightRow(s.rects[i], i, s.materials[1].emission, nullptr, nullptr, light);
        if (light[15] != 0.0f || light[20] != 0.0f || light[43] != 0.0f) return fail(triangles, "light row without triangles");
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
        // every rectangle and sphere moved, the second rectangle so that its winding flips, the first sphere to a negative radius
        setRect(s.rects[0], -9, -7, -8, 17, 1, 0, 0, 0, 15, 0.1f, 1, 0);
        setRect(s.rects[1], 1, 6, -2, 0, 0, 2, 2, 0.5f, 0, 0, -1, 0.2f);
        setRect(s.rects[2], 5, -1, 1, 0, 0, 3, 0, 3, 0, -1, 0.1f, 0);
        s.spheres[0].centerRadius[0] = 30.0f, s.spheres[0].centerRadius[3] = -0.25f;
        s.spheres[1].centerRadius[1] = -12.0f, s.spheres[1].centerRadius[3] = 2.0f;
        if (!check(triangles, s)) return 1;
        std::printf("%u triangles: ok\n", triangles);
    }
    return 0;
}
