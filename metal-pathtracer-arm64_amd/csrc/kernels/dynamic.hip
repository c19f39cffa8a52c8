// The kernels of a dynamic scene (include/ptr_dynamic.h; launchers in dynamic.h).  Compiled like the rest of the tree, unfused
// (-ffp-contract=off) with correctly rounded division and square root: every value written here is bit for bit what the host bake
// (host/scene_geometry.cpp) and the host builder (host/bvh_builder.cpp) write for the same input, because the operations and their
// order are the host's.
//
// k_dyn_bake          one moved triangle per lane, through the per-mesh list of leaf-order indices.
// k_dyn_refit_level   one launch per height level, lowest first; a lane owns one node and writes both child boxes.  A leaf child is the
//                     union of its primitives' padded bounds, an internal child the union of that node's two child boxes, which an
//                     EARLIER launch wrote: the launch boundary is the only hand-off between workgroups.
// k_dyn_quantise      one node per lane: both 16 B records from the float boxes through kernels/bvh_grid.h.
// k_dyn_wide          one wide place per lane: the three box words of its source record.
// Every access of these is one 16 B load or store.  include/ptr_deform.h adds two kernels that compute nothing:
// k_dyn_gather_corners  one triangle of a deformed mesh per lane: its three vertices, through the corner table, to the object-space rows
//                       k_dyn_bake reads (4 B gather loads - packed float3 is only 4 B aligned - and 16 B stores).
// k_dyn_scatter_rows    one 16 B row of a moved sphere or rectangle per lane, computed on the host, to the array it belongs to.
// include/ptr_deform_device.h adds two that write nothing the renderer reads:
// k_dyn_check_finite    a grid-stride pass over the caller's device arrays; a bit per array with a non-finite float, by atomic OR.
// k_dyn_vertex_normals  one vertex per lane: area-weighted normals through the vertex adjacency, into scratch the gather then reads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bvh_grid.h"
#include "bvh_layout.h"
#include "dynamic.h"

namespace ptrk {

namespace {

constexpr uint32_t kBlock = 256u;

struct V3 {
    float x, y, z;
};

// std::min / std::max as the host uses them (the second argument wins only when strictly smaller / larger)
__device__ inline float minOf(float a, float b) { return b < a ? b : a; }
__device__ inline float maxOf(float a, float b) { return a < b ? b : a; }

__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ inline float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline float length3(V3 a) { return sqrtf(dot3(a, a)); }

// transformPoint of the host bake: ((m00 x + m10 y) + m20 z) + m30
__device__ inline V3 xfPoint(const float* m, float4 p) {
    return {((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12], ((m[1] * p.x + m[5] * p.y) + m[9] * p.z) + m[13],
            ((m[2] * p.x + m[6] * p.y) + m[10] * p.z) + m[14]};
}
// the linear part alone (tangents)
__device__ inline V3 xfVector(const float* m, float4 p) {
    return {(m[0] * p.x + m[4] * p.y) + m[8] * p.z, (m[1] * p.x + m[5] * p.y) + m[9] * p.z, (m[2] * p.x + m[6] * p.y) + m[10] * p.z};
}

__device__ inline float4 bakeNormal(const DynMeshRow& r, float4 n) {
    // (nc0 n.x + nc1 n.y) + nc2 n.z, then length > 0 ? v * (1 / sqrt(dot)) : v
    const V3 wn{(r.nc0[0] * n.x + r.nc1[0] * n.y) + r.nc2[0] * n.z, (r.nc0[1] * n.x + r.nc1[1] * n.y) + r.nc2[1] * n.z,
                (r.nc0[2] * n.x + r.nc1[2] * n.y) + r.nc2[2] * n.z};
    const float d = dot3(wn, wn);
    const V3 out = sqrtf(d) > 0.0f ? scale(wn, 1.0f / sqrtf(d)) : wn;
    return make_float4(out.x, out.y, out.z, 0.0f);
}

// uv-per-world of one uv set (host/scene_geometry.cpp, the same branches and thresholds)
__device__ inline float uvPerWorld(V3 edge1, V3 edge2, float u0, float v0, float u1, float v1, float u2, float v2) {
    const float du1 = u1 - u0, dv1 = v1 - v0;
    const float du2 = u2 - u0, dv2 = v2 - v0;
    const float det = du1 * dv2 - dv1 * du2;
    float perWorld = 0.0f;
    bool done = false;
    if (fabsf(det) > 1.0e-9f) {
        const float inv = 1.0f / det;
        const V3 dPdu = scale(sub(scale(edge1, dv2), scale(edge2, dv1)), inv), dPdv = scale(sub(scale(edge2, du1), scale(edge1, du2)), inv);
        const float lenU = length3(dPdu), lenV = length3(dPdv);
        if (lenU > 1.0e-8f && lenV > 1.0e-8f) {
            perWorld = maxOf(1.0f / lenU, 1.0f / lenV);
            done = isfinite(perWorld) && perWorld > 0.0f;
        }
    }
    if (!done) {
        const float worldArea = length3(cross3(edge1, edge2)), uvArea = fabsf(det);
        perWorld = (worldArea > 1.0e-12f && uvArea > 1.0e-12f) ? sqrtf(uvArea / worldArea) : 0.0f;
        if (!isfinite(perWorld)) perWorld = 0.0f;
    }
    return perWorld;
}

__global__ void __launch_bounds__(kBlock) k_dyn_bake(DynBakeArrays a, const float4* __restrict__ meshTable, uint32_t mesh,
                                                     const uint32_t* __restrict__ list, uint32_t count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const size_t k = list[i];
    DynMeshRow r;
    {
        float4* dst = reinterpret_cast<float4*>(&r);
#pragma unroll
        for (uint32_t q = 0; q < kDynMeshVec4 - 1u; ++q) dst[q] = meshTable[static_cast<size_t>(mesh) * kDynMeshVec4 + q];
    }
    const float4 p0 = a.objPos[k * 3 + 0], p1 = a.objPos[k * 3 + 1], p2 = a.objPos[k * 3 + 2];
    const V3 v0 = xfPoint(r.l2w, p0), v1 = xfPoint(r.l2w, p1), v2 = xfPoint(r.l2w, p2);
    const V3 e1 = sub(v0, v1), e2 = sub(v2, v0);
    // the w words of the three rows (material, meta word, primitive index) travel with the object-space corners
    a.tris[k * 3 + 0] = make_float4(v0.x, v0.y, v0.z, p0.w);
    a.tris[k * 3 + 1] = make_float4(e1.x, e1.y, e1.z, p1.w);
    a.tris[k * 3 + 2] = make_float4(e2.x, e2.y, e2.z, p2.w);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.triNormals[k * 3 + c] = bakeNormal(r, a.objNrm[k * 3 + c]);
    // padded bounds (storeTri + padBounds)
    float lo[3], hi[3];
    const float x[3][3] = {{v0.x, v1.x, v2.x}, {v0.y, v1.y, v2.y}, {v0.z, v1.z, v2.z}};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = minOf(minOf(x[ax][0], x[ax][1]), x[ax][2]);
        hi[ax] = maxOf(maxOf(x[ax][0], x[ax][1]), x[ax][2]);
        const float pad = 1e-5f * maxOf(maxOf(fabsf(lo[ax]), fabsf(hi[ax])), 1.0f);
        lo[ax] -= pad;
        hi[ax] += pad;
    }
    a.triBounds[k * 2 + 0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    a.triBounds[k * 2 + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    if (a.triUv) {
        if (r.hasTangents != 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 tl = a.objTan[k * 3 + c];
                const V3 t = xfVector(r.l2w, tl);
                const float w = tl.w == 0.0f ? 0.0f : (tl.w < 0.0f ? -1.0f : 1.0f) * r.detSign;
                a.triTangent[k * 3 + c] = make_float4(t.x, t.y, t.z, w);
            }
        }
        const float4 uv0 = a.triUv[k * 4 + 0], uv1 = a.triUv[k * 4 + 1], uv2 = a.triUv[k * 4 + 2];
        const V3 edge1 = sub(v1, v0), edge2 = sub(v2, v0);
        const float pw0 = uvPerWorld(edge1, edge2, uv0.x, uv0.y, uv1.x, uv1.y, uv2.x, uv2.y);
        const float pw1 = uvPerWorld(edge1, edge2, uv0.z, uv0.w, uv1.z, uv1.w, uv2.z, uv2.w);
        a.triUv[k * 4 + 3] = make_float4(pw0, pw1, r.detSign, 0.0f);
    }
}

// One triangle of a deformed mesh per lane: its three vertices through the corner table into the object-space corner rows k_dyn_bake
// reads.  The vertex arrays are packed float3 (4 B aligned), so the gather loads are 4 B; every store is 16 B.  The w words of objPos
// carry the w words of the triangle's tris row and stay.
__global__ void __launch_bounds__(kBlock) k_dyn_gather_corners(float4* __restrict__ objPos, float4* __restrict__ objNrm, float4* __restrict__ objTan,
                                                               DynVertexArrays v, const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ corners, uint32_t count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const size_t k = list[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t vi = corners[static_cast<size_t>(i) * 3 + c];
        const float* p = v.positions + vi * 3;
        const float* n = v.normals + vi * 3;
        const float w = objPos[k * 3 + c].w;
        objPos[k * 3 + c] = make_float4(p[0], p[1], p[2], w);
        objNrm[k * 3 + c] = make_float4(n[0], n[1], n[2], 0.0f);
        if (v.tangents) {
            const float* t = v.tangents + vi * 4;
            objTan[k * 3 + c] = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
}

// include/ptr_deform_device.h.  One grid-stride pass over every array an update from device pointers will read: blockIdx.y names the row
// of the table (an array: pointer and float count), the blocks of a row stride over its floats with coalesced 4 B loads (packed float3 is
// only 4 B aligned).  Reads the caller's arrays, writes the flag words alone: at most one atomic OR per wave, and none on finite data.
__global__ void __launch_bounds__(kBlock) k_dyn_check_finite(const DynCheckRow* __restrict__ rows, uint32_t rowBase, uint32_t* __restrict__ flags) {
    const uint32_t r = rowBase + blockIdx.y;
    const DynCheckRow row = rows[r];
    bool bad = false;
    const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < row.count; i += stride) {
        bad = bad || (__float_as_uint(row.data[i]) & 0x7F800000u) == 0x7F800000u;   // exponent all ones: infinite or NaN
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&flags[r >> 5], 1u << (r & 31u));
}

// One vertex per lane: the sum of the cross products of the triangles that name it, in the adjacency's order (ascending triangle of the
// description, so the sum does not depend on the tree), normalised by the bake's rule.  Unfused like everything here: the values are
// tests/deform_device_ref.py's bit for bit.  Per vertex 8 B of row offsets read (4 B fresh) and 12 B written; per incident corner one 4 B
// entry, three 4 B indices and nine 4 B position gathers - scattered, but a mesh's vertices and triangles that are close in the arrays
// are close in space more often than not, and the arrays of one mesh stay in L2.
__global__ void __launch_bounds__(kBlock) k_dyn_vertex_normals(const float* __restrict__ positions, const uint32_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ entries, const uint32_t* __restrict__ corners,
                                                               float* __restrict__ normals, uint32_t vertexCount) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= vertexCount) return;
    V3 s{0.0f, 0.0f, 0.0f};
    const uint32_t end = offsets[v + 1u];
    for (uint32_t e = offsets[v]; e < end; ++e) {
        const size_t t = entries[e];
        V3 p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = positions + static_cast<size_t>(corners[t * 3 + c]) * 3;
            p[c] = {q[0], q[1], q[2]};
        }
        const V3 n = cross3(sub(p[1], p[0]), sub(p[2], p[0]));
        s = {s.x + n.x, s.y + n.y, s.z + n.z};
    }
    const float d = dot3(s, s);
    const V3 out = d > 0.0f ? scale(s, 1.0f / sqrtf(d)) : s;
    float* dst = normals + static_cast<size_t>(v) * 3;
    dst[0] = out.x, dst[1] = out.y, dst[2] = out.z;
}

// One 16 B row per lane: the rows of moved spheres and rectangles, computed on the host, to the arrays they belong to.
__global__ void __launch_bounds__(kBlock) k_dyn_scatter_rows(DynScatterTargets t, const float4* __restrict__ rows, const uint32_t* __restrict__ dest,
                                                             uint32_t count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t d = dest[i], array = d >> kScatterArrayShift, row = d & kScatterRowMask;
    float4* base = nullptr;
    uint32_t limit = 0u;
#pragma unroll
    for (uint32_t a = 0; a < kScatterArrays; ++a) {
        if (array == a) base = t.base[a], limit = t.rows[a];
    }
    if (row < limit) base[row] = rows[i];
}

struct Box {
    float lo[3], hi[3];
};
__device__ inline void growBox(Box& b, float4 lo, float4 hi) {
    b.lo[0] = minOf(b.lo[0], lo.x), b.lo[1] = minOf(b.lo[1], lo.y), b.lo[2] = minOf(b.lo[2], lo.z);
    b.hi[0] = maxOf(b.hi[0], hi.x), b.hi[1] = maxOf(b.hi[1], hi.y), b.hi[2] = maxOf(b.hi[2], hi.z);
}

__global__ void __launch_bounds__(kBlock) k_dyn_refit_level(float4* __restrict__ boxes, const uint32_t* __restrict__ schedule, uint32_t count,
                                                            const float4* __restrict__ triBounds, const float4* __restrict__ sphereBounds) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const size_t node = schedule[i];
    float4 row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = boxes[node * 4 + q];
    const uint32_t refs[2] = {__float_as_uint(row[0].w), __float_as_uint(row[1].w)};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint32_t ref = refs[c];
        if (ref == kRefEmpty) continue;   // an empty child keeps its record
        Box b;
        const float inf = __uint_as_float(0x7F800000u);
        b.lo[0] = b.lo[1] = b.lo[2] = inf;
        b.hi[0] = b.hi[1] = b.hi[2] = -inf;
        if (ref & kRefLeafBit) {
            const float4* bounds = (ref & kRefSphereBit) ? sphereBounds : triBounds;
            const size_t first = ref & kRefOffsetMask;
            const uint32_t prims = ((ref >> kRefCountShift) & 0xFu) + 1u;
            for (uint32_t p = 0; p < prims; ++p) growBox(b, bounds[(first + p) * 2], bounds[(first + p) * 2 + 1]);
        } else {
            const size_t child = ref;
            const float4 c0 = boxes[child * 4 + 0], c1 = boxes[child * 4 + 1];
            if (__float_as_uint(c0.w) != kRefEmpty) growBox(b, c0, c1);
            if (__float_as_uint(c1.w) != kRefEmpty) growBox(b, boxes[child * 4 + 2], boxes[child * 4 + 3]);
        }
        row[c * 2 + 0] = make_float4(b.lo[0], b.lo[1], b.lo[2], row[c * 2 + 0].w);
        row[c * 2 + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], row[c * 2 + 1].w);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) boxes[node * 4 + q] = row[q];
}

struct GridArgs {
    float origin[3], cell[3];
};

__global__ void __launch_bounds__(kBlock) k_dyn_quantise(const float4* __restrict__ boxes, uint4* __restrict__ qnodes, uint32_t nodeCount, GridArgs g) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    const size_t node = i;
    float4 row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = boxes[node * 4 + q];
    const uint32_t refs[2] = {__float_as_uint(row[0].w), __float_as_uint(row[1].w)};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float lo[3] = {row[c * 2].x, row[c * 2].y, row[c * 2].z}, hi[3] = {row[c * 2 + 1].x, row[c * 2 + 1].y, row[c * 2 + 1].z};
        uint32_t w[4];
        quantiseChild(lo, hi, refs[c], g.origin, g.cell, w);
        qnodes[node * 2 + c] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ void __launch_bounds__(kBlock) k_dyn_wide(const uint4* __restrict__ qnodes, uint4* __restrict__ wnodes, const uint32_t* __restrict__ source,
                                                     uint32_t places) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= places) return;
    const uint32_t src = source[i];
    if (src == 0xFFFFFFFFu) return;   // an unused place stays an inverted box
    const uint4 rec = qnodes[src];
    uint4 w = wnodes[i];
    w.x = rec.x, w.y = rec.y, w.z = rec.z;   // the reference word, renumbered to wide indices at upload, stays
    wnodes[i] = w;
}

uint32_t blocksFor(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

}  // namespace

void launchDynBake(const DynBakeArrays& a, const float4* dMeshTable, uint32_t mesh, const uint32_t* dList, uint32_t count, hipStream_t stream) {
    if (count > 0u) hipLaunchKernelGGL(k_dyn_bake, dim3(blocksFor(count)), dim3(kBlock), 0, stream, a, dMeshTable, mesh, dList, count);
}

void launchDynGatherCorners(float4* dObjPos, float4* dObjNrm, float4* dObjTan, const DynVertexArrays& v, const uint32_t* dList, const uint32_t* dCorners,
                            uint32_t count, hipStream_t stream) {
    if (count > 0u) hipLaunchKernelGGL(k_dyn_gather_corners, dim3(blocksFor(count)), dim3(kBlock), 0, stream, dObjPos, dObjNrm, dObjTan, v, dList, dCorners, count);
}

void launchDynCheckFinite(const DynCheckRow* dRows, uint32_t rows, uint64_t largest, uint32_t* dFlags, hipStream_t stream) {
    // enough blocks per row for the longest one at a few floats per lane, and no more than fill the device a few times over
    const uint32_t perRow = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>((largest + kBlock * 4u - 1u) / (kBlock * 4u), 1u), 2048u));
    constexpr uint32_t kMaxGridY = 65535u;
    for (uint32_t base = 0; base < rows; base += kMaxGridY) {
        hipLaunchKernelGGL(k_dyn_check_finite, dim3(perRow, std::min(rows - base, kMaxGridY)), dim3(kBlock), 0, stream, dRows, base, dFlags);
    }
}

void launchDynVertexNormals(const float* dPositions, const uint32_t* dOffsets, const uint32_t* dEntries, const uint32_t* dCorners, float* dNormals,
                            uint32_t vertexCount, hipStream_t stream) {
    if (vertexCount > 0u) {
        hipLaunchKernelGGL(k_dyn_vertex_normals, dim3(blocksFor(vertexCount)), dim3(kBlock), 0, stream, dPositions, dOffsets, dEntries, dCorners, dNormals, vertexCount);
    }
}

void launchDynScatterRows(const DynScatterTargets& t, const float4* dRows, const uint32_t* dDest, uint32_t count, hipStream_t stream) {
    if (count > 0u) hipLaunchKernelGGL(k_dyn_scatter_rows, dim3(blocksFor(count)), dim3(kBlock), 0, stream, t, dRows, dDest, count);
}

void launchDynRefitLevel(float4* dBoxes, const uint32_t* dSchedule, uint32_t count, const float4* dTriBounds, const float4* dSphereBounds,
                         hipStream_t stream) {
    if (count > 0u) hipLaunchKernelGGL(k_dyn_refit_level, dim3(blocksFor(count)), dim3(kBlock), 0, stream, dBoxes, dSchedule, count, dTriBounds, dSphereBounds);
}

void launchDynQuantise(const float4* dBoxes, uint4* dQnodes, uint32_t nodeCount, const float origin[3], const float cell[3], hipStream_t stream) {
    GridArgs g;
    for (int a = 0; a < 3; ++a) g.origin[a] = origin[a], g.cell[a] = cell[a];
    if (nodeCount > 0u) hipLaunchKernelGGL(k_dyn_quantise, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, dBoxes, dQnodes, nodeCount, g);
}

void launchDynWide(const uint4* dQnodes, uint4* dWnodes, const uint32_t* dWideSource, uint32_t places, hipStream_t stream) {
    if (places > 0u) hipLaunchKernelGGL(k_dyn_wide, dim3(blocksFor(places)), dim3(kBlock), 0, stream, dQnodes, dWnodes, dWideSource, places);
}

}  // namespace ptrk
