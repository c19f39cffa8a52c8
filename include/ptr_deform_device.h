/*
 * ptr_deform_device.h — ptr_scene_set_mesh_vertices (ptr_deform.h) for callers whose vertex data is resident on the device: skinning,
 * cloth, a simulation written in torch.  The arrays are read where they are; no component passes through the host.
 *
 * ptr_scene_set_mesh_vertices_device takes DEVICE pointers.  The host checks the pointers alone (alignment, kind of memory, device, and
 * where the runtime knows it the size of the allocation); k_dyn_check_finite looks at every component on the device and ORs one bit per
 * (mesh, array) into flag words the scene owns, which come back before anything the renderer reads is written: a non-finite component is
 * refused as ptr_scene_set_mesh_vertices refuses it, with every array of the scene as it was.  Then k_dyn_gather_corners reads straight
 * from the caller's arrays, and k_dyn_bake and the refit run as they do for every update call.  The result is bit for bit that of
 * ptr_scene_set_mesh_vertices with the same data.
 *
 * A scene uploaded with PTR_DYNAMIC_VERTEX_NORMALS (ptr_scene_upload_deformable) also keeps, per mesh, a vertex-adjacency table: per
 * vertex the corners that name it, in ascending order of the description's triangles (4 B per vertex + 4 B, and 12 B per triangle).  A
 * mesh given without normals then has them computed on the device (k_dyn_vertex_normals, one vertex per lane), area-weighted, in float32:
 *
 *     s = (+0, +0, +0)
 *     for each corner naming the vertex, in that order:  p0, p1, p2 = positions of that triangle's indices 0, 1, 2
 *         e1 = p1 - p0;  e2 = p2 - p0
 *         s += (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x)        one add per component
 *     d = (s.x s.x + s.y s.y) + s.z s.z
 *     n = d > 0 ? s * (1 / sqrt(d)) : s
 *
 * unfused, with correctly rounded division and square root, so the values are those of tests/deform_device_ref.py bit for bit and do not
 * depend on the tree.  A triangle that names a vertex twice is added twice; a vertex no triangle names gets (0, 0, 0).  The normals go to
 * scratch the scene owns and are checked like given ones: a sum that overflows is refused.  Tangents are never computed.
 *
 * The contract of the arrays: they are read on `stream`; whatever produces them must be ordered before the call on that stream, or have
 * finished; they are free again when the call returns (it ends with a stream synchronisation); they must not overlap the scene's own
 * buffers.  Plain device memory only: host, registered-host and managed memory and another device's memory are refused by name.
 */
#ifndef PTR_DEFORM_DEVICE_H
#define PTR_DEFORM_DEVICE_H

#include "ptr_deform.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PTR_DYNAMIC_VERTEX_NORMALS = 4 }; /* needs PTR_DYNAMIC_DEFORMABLE: normals may be left to ptr_scene_set_mesh_vertices_device */

/* ptr_scene_upload_dynamic_ex, which also knows PTR_DYNAMIC_VERTEX_NORMALS.  1 for an unknown flag and for PTR_DYNAMIC_VERTEX_NORMALS
 * without PTR_DYNAMIC_DEFORMABLE; 2 without a HIP device. */
int ptr_scene_upload_deformable(const PtrSceneDesc* scene, int device, uint32_t flags, PtrDeviceScene** out_scene, char* err, size_t err_cap);

typedef struct PtrMeshVerticesDevice {
    uint32_t meshIndex, vertexCount; /* vertexCount: as at upload */
    const float* positions;          /* DEVICE, vertexCount * 3 packed, 4 B aligned */
    const float* normals;            /* DEVICE, vertexCount * 3, or NULL: compute them (the scene needs PTR_DYNAMIC_VERTEX_NORMALS) */
    const float* tangents;           /* DEVICE, vertexCount * 4, or NULL: given exactly when the upload's mesh carried tangents */
} PtrMeshVerticesDevice;

/* ptr_scene_set_mesh_vertices from device-resident arrays.  Stream, synchronisation and info as there; bakeMs covers everything from the
 * first kernel of the call (the normals, the finiteness check) to the end of the bake, the read-back of the flag words included.
 * Refused before any device work, on top of everything ptr_scene_set_mesh_vertices refuses: a pointer that is not 4 B aligned; memory
 * that is not plain device memory of the scene's device, or an allocation that ends before the array does; null normals on a scene
 * without PTR_DYNAMIC_VERTEX_NORMALS.  Refused after kernels that only read the caller's arrays and write scene-owned scratch, with
 * every array the renderer reads unchanged: a non-finite position, normal (given or computed) or tangent component - the first named
 * mesh that has one, positions ahead of normals ahead of tangents. */
int ptr_scene_set_mesh_vertices_device(PtrDeviceScene* scene, const PtrMeshVerticesDevice* meshes, uint32_t count, void* stream, PtrUpdateInfo* info,
                                       char* err, size_t err_cap);

/* ---- test-only probe, host side (no GPU) ----
 * The vertex-adjacency table PTR_DYNAMIC_VERTEX_NORMALS keeps for mesh `mesh` of the preparation of `scene`: vertexCount + 1 row offsets,
 * then one word per corner of the mesh: the number, within the mesh, of the description's triangle that corner belongs to (its three
 * vertex indices are entries 3 t .. 3 t + 2 of the corner table, PTR_DYNAMIC_TABLE_MESH_CORNERS, of that mesh).  *size_out in bytes;
 * out may be NULL (size only). */
int ptr_debug_vertex_adjacency(const PtrSceneDesc* scene, uint32_t mesh, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DEFORM_DEVICE_H */
