// Launchers of the dynamic-scene kernels (dynamic.hip; include/ptr_dynamic.h): re-bake the triangles of a moved mesh, refit the float
// child boxes level by level, requantise the binary nodes and refill the four-wide ones; and, for include/ptr_deform.h, gather new vertex
// data into the corner rows the bake reads and scatter the host-computed rows of moved spheres and rectangles; and, for
// include/ptr_deform_device.h, check a caller's device arrays for non-finite components and compute vertex normals.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptrk {

// One row of the per-call mesh table: what the host bake derives from localToWorld, computed by the host's own functions
// (ptr::ComputeMeshBake), so the device multiplies by the host's bits.
constexpr uint32_t kDynMeshVec4 = 8u;
struct alignas(16) DynMeshRow {
    float l2w[16];        // column-major
    float nc0[3], detSign;
    float nc1[3], hasTangents;   // 1: the mesh carries tangents
    float nc2[3], pad0;
    float pad1[4];
};
static_assert(sizeof(DynMeshRow) == kDynMeshVec4 * 16u, "mesh table row layout");

// The arrays a bake writes (leaf order) and the object-space corners it reads.  triUv / triTangent / objTan are null in untextured scenes.
struct DynBakeArrays {
    const float4* objPos;
    const float4* objNrm;
    const float4* objTan;
    float4* tris;
    float4* triNormals;
    float4* triBounds;
    float4* triUv;
    float4* triTangent;
};

// New per-vertex data of one mesh in device scratch (include/ptr_deform.h): float3 positions and normals, float4 tangents (null: the mesh
// carries none, or the scene is untextured).  Packed as the caller gave them, so only 4 B aligned.
struct DynVertexArrays {
    const float* positions;
    const float* normals;
    const float* tangents;
};
// triangles list[0 .. count) of one mesh: corners[3 i ..] are the vertex indices of list[i]; writes its object-space corner rows
void launchDynGatherCorners(float4* dObjPos, float4* dObjNrm, float4* dObjTan, const DynVertexArrays& v, const uint32_t* dList, const uint32_t* dCorners,
                            uint32_t count, hipStream_t stream);

// include/ptr_deform_device.h: the caller's arrays are read where they are, so their components are looked at on the device.  One row per
// array, behind the mesh rows of the per-call mesh table: `count` floats at `data`; row r of a launch owns bit r of the flag words.
struct alignas(16) DynCheckRow {
    const float* data;
    uint64_t count;
};
static_assert(sizeof(DynCheckRow) == 16u, "check row layout");
// ORs bit r into dFlags (32 rows per word; cleared by the caller) when row r holds a non-finite float.  largest: the longest row.
void launchDynCheckFinite(const DynCheckRow* dRows, uint32_t rows, uint64_t largest, uint32_t* dFlags, hipStream_t stream);
// Area-weighted vertex normals of one mesh, one vertex per lane, by the rule of include/ptr_deform_device.h: offsets / entries are the
// mesh's vertex adjacency (ptr::BuildVertexAdjacency), corners its corner table in the description's triangle order; packed float3 out.
void launchDynVertexNormals(const float* dPositions, const uint32_t* dOffsets, const uint32_t* dEntries, const uint32_t* dCorners, float* dNormals,
                            uint32_t vertexCount, hipStream_t stream);

// The arrays ptr_scene_set_spheres / ptr_scene_set_rects scatter rows into, indexed by PTR_SCATTER_*: a destination word is
// (array << kScatterArrayShift) | row, the row counted in float4.
constexpr uint32_t kScatterArrays = 7u, kScatterArrayShift = 28u, kScatterRowMask = (1u << kScatterArrayShift) - 1u;
struct DynScatterTargets {
    float4* base[kScatterArrays];
    uint32_t rows[kScatterArrays];   // float4 in each: a destination past it is skipped
};
// dst[dest[i]] = rows[i], i < count
void launchDynScatterRows(const DynScatterTargets& t, const float4* dRows, const uint32_t* dDest, uint32_t count, hipStream_t stream);

// triangles list[0 .. count) through row `mesh` of the table
void launchDynBake(const DynBakeArrays& a, const float4* dMeshTable, uint32_t mesh, const uint32_t* dList, uint32_t count, hipStream_t stream);
// one height level: nodes dSchedule[0 .. count), both child boxes each; children of internal children were written by earlier launches
void launchDynRefitLevel(float4* dBoxes, const uint32_t* dSchedule, uint32_t count, const float4* dTriBounds, const float4* dSphereBounds,
                         hipStream_t stream);
void launchDynQuantise(const float4* dBoxes, uint4* dQnodes, uint32_t nodeCount, const float origin[3], const float cell[3], hipStream_t stream);
// every place of every wide node takes the three box words of its source record; the reference word stays
void launchDynWide(const uint4* dQnodes, uint4* dWnodes, const uint32_t* dWideSource, uint32_t places, hipStream_t stream);

}  // namespace ptrk
