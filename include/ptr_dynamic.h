/*
 * ptr_dynamic.h — dynamic scenes of libptr_hip.so: a scene whose meshes can be moved while it stays resident on the device.
 *
 * ptr_scene_upload bakes every mesh to world space on the host and builds one SAH tree over everything; moving one object means doing
 * all of that again.  A scene uploaded with ptr_scene_upload_dynamic keeps, beside the arrays the kernels render from, the object-space
 * corners of its mesh triangles, the padded primitive bounds the builder was given, the float child boxes of every node, a refit
 * schedule (the nodes grouped by height) and, with four-wide nodes, the table of records each wide place copies.
 * ptr_scene_set_mesh_transforms then re-bakes the triangles of the named meshes on the device with the host bake's own operations in
 * the host's order, refits the boxes level by level (one launch per level; no data passes between workgroups inside a launch), reads
 * the root box back, derives the 16-bit grid from it by the builder's rule, and requantises the binary and four-wide nodes.  The
 * topology of the tree stays what the upload built; every array is bit for bit what the host builder would produce for that topology
 * and the moved description.
 *
 * The node format (float, quantised binary, four-wide; PTR_QUANTIZED_NODES and PTR_WIDE_NODES) is decided once, at upload, and kept:
 * PtrUpdateInfo::cellOverExtent tells when a fresh upload would have chosen otherwise.  A refit does not rebuild: when boxes overlap
 * much more than a fresh tree's would, ptr_rebuild.h measures it (ptr_scene_tree_cost) and rebuilds the tree above the leaves on the device.
 *
 * This header moves whole meshes rigidly.  ptr_deform.h adds, for scenes uploaded with its flags, new vertex data for a mesh and new
 * places for spheres and rectangles, the lights among them.  Materials, emission, textures, uv coordinates and topology stay;
 * the one-shot ptr_render_multi* calls and the geometry cache (ptr_scene_upload_prepared) do not take part.  A frame on several devices
 * (ptr_multi_frame.h) is created over dynamic scenes and updated in place on all of them through ptr_multi_dynamic.h.
 *
 * Resumable frames (ptr_frame.h) on a dynamic scene keep working.  The samples a frame holds belong to the pose they were taken in:
 * after an update call ptr_frame_reset before accumulating again.  Nothing here tracks that.
 */
#ifndef PTR_DYNAMIC_H
#define PTR_DYNAMIC_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrMeshTransform {
    uint32_t meshIndex;        /* index into PtrSceneDesc::meshes of the upload */
    uint32_t pad;
    float localToWorld[16];    /* column-major, as PtrMeshDesc */
} PtrMeshTransform;

typedef struct PtrUpdateInfo {
    double totalSeconds;                        /* host wall time of the call, the final synchronisation included */
    double bakeMs, refitMs, quantiseMs, wideMs; /* HIP-event times of the kernel groups */
    uint64_t trianglesMoved, nodes, levels, wideNodes;
    float sceneLo[3], sceneHi[3];               /* root box after the refit */
    float gridOrigin[3], gridCell[3];
    float cellOverExtent;                       /* largest grid cell / mean primitive extent at upload; above 1/8 a fresh upload would have chosen float nodes */
    uint32_t pad;
} PtrUpdateInfo;

/* ptr_scene_upload plus the extra device data of a dynamic scene.  The host arrays of the description need not outlive the call.
 * Released with ptr_scene_release like any scene.  2 without a HIP device. */
int ptr_scene_upload_dynamic(const PtrSceneDesc* scene, int device, PtrDeviceScene** out_scene, char* err, size_t err_cap);

/* Replaces localToWorld of the `count` named meshes and brings every array of the scene to the new pose; other meshes, rectangles,
 * spheres, lights, materials and textures stay.  Runs on `stream` and ends with a stream synchronisation (the grid of the quantised
 * nodes travels to the kernels as arguments and comes from the root box).  Renders of this scene on other streams must have finished.
 * Refused with a message naming the cause, before any device work and with the scene unchanged: a scene that is not dynamic; a null
 * list or count == 0; a mesh index out of range; an index named twice; a matrix with a non-finite entry; a matrix whose 3x3 determinant
 * is zero or whose cofactor inverse is not finite.  A mesh without triangles is accepted and changes nothing.  info may be NULL. */
int ptr_scene_set_mesh_transforms(PtrDeviceScene* scene, const PtrMeshTransform* transforms, uint32_t count, void* stream, PtrUpdateInfo* info,
                                  char* err, size_t err_cap);

/* 1 for a scene uploaded with ptr_scene_upload_dynamic, 0 otherwise (or NULL). */
int ptr_scene_is_dynamic(const PtrDeviceScene* scene);

/* ---- test-only probes (they live here, not in ptr_debug.h, because they speak of this header's tables) ----
 * The arrays of a device scene, dynamic or not, downloaded: *size_out = the array's size in bytes (0: the scene
 * has no such array); out may be NULL (size only).  tris, triNormals (48 B per triangle), triUv (64 B), triTangent (48 B), in leaf order;
 * the padded primitive bounds of a dynamic scene (32 B per triangle / sphere: lo xyz, 0, hi xyz, 0); the 64 B float nodes (a dynamic
 * scene, or a static one that renders from them); qnodes (32 B per node); wnodes (64 B per wide node); the grid (origin xyz, cell xyz);
 * the rects rows (80 B per rectangle), the rectLights rows (176 B per light) and the spheres rows (16 B, leaf order); the object-space
 * corner rows of a dynamic scene (48 B per triangle each; objTan in textured scenes).
 * 1: bad argument, 2: cap_bytes too small, 3: the copy failed. */
enum {
    PTR_SCENE_ARRAY_TRIS = 0,
    PTR_SCENE_ARRAY_TRI_NORMALS = 1,
    PTR_SCENE_ARRAY_TRI_UV = 2,
    PTR_SCENE_ARRAY_TRI_TANGENT = 3,
    PTR_SCENE_ARRAY_TRI_BOUNDS = 4,
    PTR_SCENE_ARRAY_SPHERE_BOUNDS = 5,
    PTR_SCENE_ARRAY_BOXES = 6,
    PTR_SCENE_ARRAY_QNODES = 7,
    PTR_SCENE_ARRAY_WNODES = 8,
    PTR_SCENE_ARRAY_GRID = 9,
    PTR_SCENE_ARRAY_RECTS = 10,
    PTR_SCENE_ARRAY_RECT_LIGHTS = 11,
    PTR_SCENE_ARRAY_SPHERES = 12,
    PTR_SCENE_ARRAY_OBJ_POS = 13,
    PTR_SCENE_ARRAY_OBJ_NRM = 14,
    PTR_SCENE_ARRAY_OBJ_TAN = 15
};
int ptr_debug_scene_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out);
/* Host-side (no GPU): the preparation ptr_scene_upload_dynamic performs on a description, one table per call, with the same outputs
 * as above: the float nodes, qnodes and four-wide nodes of the builder (the node-format knobs apply as at upload); the leaf-order padded
 * bounds; the refit schedule (node indices grouped by height) and its level offsets (levels + 1 words); the wide-source table (per wide
 * place node * 2 + side, 0xFFFFFFFF: unused); the grid; the shared quantiser (csrc/kernels/bvh_grid.h) applied to the float nodes with
 * the grid the shared rule derives from node 0; the per-mesh triangle lists and their offsets; and info = {nodes, levels, wide nodes,
 * quantised nodes in use, triangles, spheres, tree depth, root reference, oversize reference, wide depth}.  The tables of ptr_deform.h:
 * the corner table (3 vertex indices per entry of the per-mesh lists), the leaf-order indices of every rectangle's two triangles, the
 * leaf slot of every sphere; and the leaf-order arrays an upload copies to the device as they stand (tris, triNormals, spheres, rects,
 * rectLights), which the row writers of ptr_deform.h are held against. */
enum {
    PTR_DYNAMIC_TABLE_NODES = 0,
    PTR_DYNAMIC_TABLE_QNODES = 1,
    PTR_DYNAMIC_TABLE_WNODES = 2,
    PTR_DYNAMIC_TABLE_TRI_BOUNDS = 3,
    PTR_DYNAMIC_TABLE_SPHERE_BOUNDS = 4,
    PTR_DYNAMIC_TABLE_SCHEDULE = 5,
    PTR_DYNAMIC_TABLE_LEVEL_OFFSETS = 6,
    PTR_DYNAMIC_TABLE_WIDE_SOURCE = 7,
    PTR_DYNAMIC_TABLE_GRID = 8,
    PTR_DYNAMIC_TABLE_REQUANTISED = 9,
    PTR_DYNAMIC_TABLE_MESH_TRI_OFFSETS = 10,
    PTR_DYNAMIC_TABLE_MESH_TRIS = 11,
    PTR_DYNAMIC_TABLE_INFO = 12,
    PTR_DYNAMIC_TABLE_MESH_CORNERS = 13,
    PTR_DYNAMIC_TABLE_RECT_TRI_LEAF = 14,
    PTR_DYNAMIC_TABLE_SPHERE_LEAF = 15,
    PTR_DYNAMIC_TABLE_TRIS = 16,
    PTR_DYNAMIC_TABLE_TRI_NORMALS = 17,
    PTR_DYNAMIC_TABLE_SPHERES = 18,
    PTR_DYNAMIC_TABLE_RECTS = 19,
    PTR_DYNAMIC_TABLE_RECT_LIGHTS = 20
};
int ptr_debug_dynamic_tables(const PtrSceneDesc* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_DYNAMIC_H */
