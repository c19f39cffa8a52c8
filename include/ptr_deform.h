/*
 * ptr_deform.h — what a dynamic scene (ptr_dynamic.h) can do beyond rigid motion of whole meshes: deform a mesh (new vertex positions,
 * normals and tangents under the same indices) and move spheres and rectangles, the emissive ones - the lights - included.
 *
 * A scene uploaded with ptr_scene_upload_dynamic_ex keeps, on request, what these calls need beside the tables of ptr_dynamic.h:
 *   PTR_DYNAMIC_DEFORMABLE  the corner table: per mesh triangle, in the order of the per-mesh triangle lists, its three vertex indices
 *                           (12 B per triangle on top of the 132 B a dynamic scene pays), because the description's index arrays need not
 *                           outlive the upload; and per mesh the vertex count, on the host.
 *   PTR_DYNAMIC_PRIMITIVES  where the two triangles of every rectangle ended up in leaf order, the leaf slot of every sphere, and on the
 *                           host the PtrRect and PtrSphere records the scene currently holds.
 *
 * ptr_scene_set_mesh_vertices stages the new per-vertex arrays into device scratch the scene owns, gathers them through the corner table
 * into the object-space corner rows (k_dyn_gather_corners, one triangle per lane) and then runs what ptr_scene_set_mesh_transforms runs:
 * the bake of that mesh under the matrix it currently has, the refit, the requantisation and the wide copy.  ptr_scene_set_spheres and
 * ptr_scene_set_rects compute the few rows of a moved primitive on the host with the functions the upload itself uses (a rectangle: its
 * two triangles and their normals and padded bounds, winding flip included, its `rects` row and, if it is a light, its `rectLights` row; a
 * sphere: its row and padded bounds), scatter them with one kernel (k_dyn_scatter_rows, one 16 B row per lane) and refit likewise.
 * Every array is bit for bit what a fresh upload of the changed description produces for the topology the tree has.
 *
 * Material index, the two-sided flag and emission of a primitive stay; so do topology, uv coordinates and indices.  Normals and tangents
 * are the caller's: nothing here computes them.  All pointers are host pointers.
 */
#ifndef PTR_DEFORM_H
#define PTR_DEFORM_H

#include "ptr_dynamic.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PTR_DYNAMIC_DEFORMABLE = 1, /* ptr_scene_set_mesh_vertices */
    PTR_DYNAMIC_PRIMITIVES = 2  /* ptr_scene_set_spheres, ptr_scene_set_rects */
};

typedef struct PtrMeshVertices {
    uint32_t meshIndex, vertexCount; /* vertexCount: as at upload */
    const float* positions;          /* vertexCount * 3, object space */
    const float* normals;            /* vertexCount * 3 */
    const float* tangents;           /* vertexCount * 4, or NULL: given exactly when the upload's mesh carried tangents */
} PtrMeshVertices;

typedef struct PtrSphereUpdate {
    uint32_t sphereIndex, pad[3];
    float centerRadius[4];
} PtrSphereUpdate;

typedef struct PtrRectUpdate {
    uint32_t rectIndex, pad[3];
    float corner[4], edgeU[4], edgeV[4], normalAndPlane[4]; /* as PtrRect, the w words included */
} PtrRectUpdate;

/* ptr_scene_upload_dynamic with flags == 0; otherwise the scene also keeps what the flags name.  1 for an unknown flag. */
int ptr_scene_upload_dynamic_ex(const PtrSceneDesc* scene, int device, uint32_t flags, PtrDeviceScene** out_scene, char* err, size_t err_cap);
/* The flags a scene was uploaded with; 0 for any other scene (or NULL). */
uint32_t ptr_scene_dynamic_flags(const PtrDeviceScene* scene);

/* New vertex data for the `count` named meshes.  Stream, synchronisation and info as ptr_scene_set_mesh_transforms; bakeMs covers the
 * gather and the bake (the staging copy runs before the first event and shows in totalSeconds alone).  Refused with a message naming the
 * cause, before any device work and with the scene unchanged: a scene that is not deformable; a null list or count == 0; a mesh index out
 * of range or named twice; a vertexCount other than the upload's; null positions or normals; tangents for a mesh uploaded without them, or
 * none for a mesh uploaded with them; a non-finite component.  A mesh without triangles is accepted and changes nothing. */
int ptr_scene_set_mesh_vertices(PtrDeviceScene* scene, const PtrMeshVertices* meshes, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                                size_t err_cap);
/* New centre and radius for the named spheres / new corner, edges and normal for the named rectangles.  Refused likewise: a scene
 * without PTR_DYNAMIC_PRIMITIVES; a null list or count == 0; an index out of range or named twice; a non-finite entry; for a rectangle
 * cross(edgeU, edgeV) or the normal of length zero.  trianglesMoved counts the triangles of moved rectangles. */
int ptr_scene_set_spheres(PtrDeviceScene* scene, const PtrSphereUpdate* spheres, uint32_t count, void* stream, PtrUpdateInfo* info, char* err,
                          size_t err_cap);
int ptr_scene_set_rects(PtrDeviceScene* scene, const PtrRectUpdate* rects, uint32_t count, void* stream, PtrUpdateInfo* info, char* err, size_t err_cap);

/* ---- test-only probe, host side (no GPU) ----
 * The host half of ptr_scene_set_spheres (kind 0, update: one PtrSphereUpdate) or ptr_scene_set_rects (kind 1, one PtrRectUpdate) on the
 * preparation of `scene` with both flags: the staging buffer the call would copy to the device - n rows of 16 B, then n destination words,
 * (array << 28) | row, array one of PTR_SCATTER_*.  *rows_out = n.  Refusals as the calls'. */
enum {
    PTR_SCATTER_TRIS = 0,
    PTR_SCATTER_TRI_NORMALS = 1,
    PTR_SCATTER_TRI_BOUNDS = 2,
    PTR_SCATTER_SPHERES = 3,
    PTR_SCATTER_SPHERE_BOUNDS = 4,
    PTR_SCATTER_RECTS = 5,
    PTR_SCATTER_RECT_LIGHTS = 6
};
int ptr_debug_dynamic_update_rows(const PtrSceneDesc* scene, uint32_t kind, const void* update, void* out, uint64_t cap_bytes, uint64_t* rows_out,
                                  char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DEFORM_H */
