// Host-side geometry preparation for the device scene: bake meshes to world space, split rectangles into two
// triangles, build the BVH and lay triangles / spheres out in leaf order.  Plain C++ (no HIP), so the CPU test
// suite can build and validate the exact arrays the GPU traverses.
//
// Reference counterparts: the Embree backend's scene assembly (src/headless/EmbreeHeadlessRenderer.mm:2100-2166
// meshes, 2184-2196 spheres, 2211-2293 rectangles) and SceneResources::rebuildAccelerationStructures
// (src/renderer/SceneResources.mm:2055-2259).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bvh_builder.h"
#include "ptr_abi.h"
#include "ptr_deform_device.h"

namespace ptr {

struct SceneGeometry {
    FlatBvh bvh;
    std::vector<float> triData;      // 12 floats per triangle in leaf order: v0|material, v0-v1|kind<<30|geom, v2-v0|primIndex
    std::vector<float> triNormals;   // 12 floats per triangle in leaf order: world-space vertex normals
    std::vector<float> sphereData;   // 4 floats per sphere in leaf order: centre, radius
    std::vector<uint32_t> sphereInfo;  // 2 words per sphere in leaf order: original index, material
    // textured scenes only (desc.textureCount > 0 and some mesh carries texture coordinates); leaf order:
    std::vector<float> triUv;        // 16 floats per triangle: (uv0, uv1) of the three vertices, then (uvPerWorld0, uvPerWorld1, sign of det(localToWorld), 0)
    std::vector<float> triTangent;   // 12 floats per triangle: world-space vertex tangents, w = handedness x sign of det (0: no tangent)
    std::vector<uint32_t> rectTriLeaf;   // 2 per rectangle: leaf-order indices of its two triangles
    uint32_t triCount = 0, sphereCount = 0;
    double gatherSeconds = 0.0, buildSeconds = 0.0, flattenSeconds = 0.0;
};

// What the bake of one mesh derives from its localToWorld, by the functions BuildSceneGeometry itself uses: the three columns the normals
// go through (rows of the cofactor inverse) and the sign of the 3x3 determinant.  det3 is that determinant.
struct MeshBake {
    float localToWorld[16];
    float nc0[3], nc1[3], nc2[3];
    float detSign, det3;
};
void ComputeMeshBake(const float localToWorld[16], MeshBake& out);

// What a dynamic scene (include/ptr_dynamic.h) keeps beside the arrays above so that a mesh can be moved and the tree refitted on the
// device.  Triangle arrays are in leaf order, like triData.
struct DynamicTables {
    std::vector<float> triBounds;      // 8 floats per triangle: the padded box the builder was given (lo xyz, 0, hi xyz, 0)
    std::vector<float> sphereBounds;   // 8 floats per sphere, likewise
    // object-space corners of every mesh triangle, 12 floats each (zeros for rectangle halves): position | the w word of the triData row,
    // normal | 0, and in textured scenes tangent | handedness as the mesh gives it
    std::vector<float> objPos, objNrm, objTan;
    std::vector<uint32_t> meshTriOffsets;   // meshCount + 1: mesh m owns meshTris[meshTriOffsets[m] .. meshTriOffsets[m + 1])
    std::vector<uint32_t> meshTris;         // leaf-order triangle indices, grouped by mesh
    std::vector<uint8_t> meshHasTangents;   // per mesh: it carries tangents (textured scenes)
    std::vector<uint32_t> schedule, levelOffsets;   // BuildRefitSchedule
    std::vector<uint32_t> wideSource;       // BuildWideNodes' source table (empty without four-wide nodes)
    bool textured = false;
    // Set by the caller before BuildSceneGeometry (PTR_DYNAMIC_DEFORMABLE / PTR_DYNAMIC_PRIMITIVES of include/ptr_deform.h,
    // PTR_DYNAMIC_VERTEX_NORMALS of include/ptr_deform_device.h): which of the tables below to fill.  The rest of this struct does not depend on it.
    uint32_t flags = 0;
    std::vector<MeshBake> meshBakes;           // per mesh: what its localToWorld bakes to (a mesh without triangles: zeros)
    // deformable scenes
    std::vector<uint32_t> meshCorners;         // 3 per entry of meshTris, in its order: the vertex indices of that triangle
    std::vector<uint32_t> meshVertexCount;     // per mesh, as the description gave it
    std::vector<uint8_t> meshTangentsGiven;    // per mesh: the description carried tangents (kept or not)
    // scenes that compute vertex normals: BuildVertexAdjacency of every mesh, one after the other.  Mesh m owns the row offsets
    // adjOffsets[adjBase[m] .. adjBase[m + 1]) (its vertex count + 1 of them, counted from 0) and the entries adjEntries[3 meshTriOffsets[m] ..)
    std::vector<uint32_t> adjOffsets, adjEntries;
    std::vector<uint64_t> adjBase;             // meshCount + 1
    // scenes whose spheres and rectangles move
    std::vector<uint32_t> sphereLeaf;          // original sphere index -> leaf slot (the inverse of SceneGeometry::sphereInfo)
    std::vector<uint32_t> rectShadeKey;        // per rectangle: the shade key of its material, which the meta word of its triangles carries
};

// The vertex adjacency of one mesh, CSR by a counting sort over its index array: vertex v owns entries[offsets[v] .. offsets[v + 1]), one
// per corner that names it, in ascending triangle order (a triangle that names v twice is there twice); an entry is the triangle's number.
// This order is the order k_dyn_vertex_normals sums in (include/ptr_deform_device.h); it depends on the index array alone.  Indices must
// be below vertexCount.
void BuildVertexAdjacency(const uint32_t* indices, size_t triangleCount, uint32_t vertexCount, std::vector<uint32_t>& offsets, std::vector<uint32_t>& entries);

// The rows of one rectangle and of one sphere, written by the upload (BuildSceneGeometry, the light table) and by ptr_scene_set_rects /
// ptr_scene_set_spheres alike: one statement of their arithmetic.
// the two triangles of rectangle `rectIndex`, winding chosen to agree with the stored normal: tris / triNormals rows and padded bounds
void WriteRectTriangles(const PtrRect& r, uint32_t rectIndex, uint32_t shadeKey, float tri[2][12], float nrm[2][12], BuildPrim prim[2]);
// the `rects` row: the description's record as it stands (5 float4)
void WriteRectRow(const PtrRect& r, float row[20]);
// one `rectLights` row (kRectLightVec4 float4): corner|area, edgeU|two-sided, edgeV|rectangle index, normal|has-triangles, emission|0, and
// the light's own two triangles as the traversal reads them (null: the geometry does not hold them)
constexpr uint32_t kRectLightFloats = 44u;
void WriteRectLightRow(const PtrRect& r, uint32_t rectIndex, const float emission[3], const float* tri0, const float* tri1, float row[kRectLightFloats]);
// the `spheres` row and the sphere's padded bounds
void WriteSphere(const PtrSphere& s, float row[4], BuildPrim& prim);

// leafMax = 0 picks the default (4).  Returns false with a message on malformed input.  dyn (nullable): also fill the tables of a dynamic
// scene (everything but wideSource, which comes with the four-wide nodes).
bool BuildSceneGeometry(const PtrSceneDesc& desc, uint32_t leafMax, SceneGeometry& out, std::string& error, DynamicTables* dyn = nullptr);

struct GeometryCheck {
    uint64_t nodes = 0, leaves = 0, trianglesReferenced = 0, spheresReferenced = 0;
    uint64_t maxDepth = 0, maxLeafSize = 0;
    uint64_t unreferenced = 0;        // primitives no leaf points at
    uint64_t multiplyReferenced = 0;  // primitives in more than one leaf
    uint64_t boxViolations = 0;       // primitives sticking out of an ancestor's child box (float nodes)
    uint64_t quantViolations = 0;     // float child boxes sticking out of their quantised twin
    uint64_t badRefs = 0;             // child references pointing outside the arrays / cycles
    uint64_t oversize = 0;            // triangles kept out of the tree (FlatBvh::oversizeRef)
    uint64_t wideNodes = 0;           // four-wide nodes (BuildWideNodes, by area)
    uint64_t wideDepth = 0;           // levels of that wide tree
    uint64_t wideProblems = 0;        // bad references in them + primitives not reached exactly once through them
};

// Walks the flattened tree from the root and checks the invariants the device traversal relies on.
void ValidateSceneGeometry(const SceneGeometry& g, GeometryCheck& out);

}  // namespace ptr
