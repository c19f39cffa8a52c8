/* Dynamic scenes on several devices: a PtrMultiFrame (ptr_multi_frame.h) created over dynamic scenes and updated in place on all its
 * devices.  A sequence of poses rendered on P devices costs one scene preparation and P uploads for the whole sequence, and one update
 * per pose: no ptr_multi_frame_create per pose.
 * Kernels: none of its own.  The per-device work of an update is csrc/kernels/dynamic.hip / rebuild.hip as ptr_dynamic.h, ptr_deform.h,
 * ptr_deform_device.h and ptr_rebuild.h run them, on each partition's own stream.  Host: csrc/host/multi_dynamic.cpp, over the partition
 * driver of multi_frame.cpp (csrc/host/multi_frame_host.h) and the two halves of every single-device update (csrc/host/dynamic_host.h).
 *
 * ---- The specification (host code and tests are written from this text) ------------------------------------------------------------
 *
 * Creation.  ptr_multi_frame_create_dynamic is ptr_multi_frame_create with one difference: the scene is prepared once as a dynamic scene
 * and uploaded to every device as ptr_scene_upload_dynamic_ex / ptr_scene_upload_deformable upload it, with dynamic_flags (PTR_DYNAMIC_*
 * of ptr_deform.h / ptr_deform_device.h; 0 is ptr_scene_upload_dynamic).  Each partition has its own scene, also when one device holds
 * several partitions.  Flag combinations those uploads refuse are refused here with the same words.  A frame made by
 * ptr_multi_frame_create is static: it allocates and behaves as before, and refuses every call below.
 *
 * The two laws.
 *   arrays   after any sequence of the calls below, every array of every partition's scene (ptr_debug_scene_arrays,
 *            ptr_debug_rebuild_arrays but the device pointers) is bit for bit that of ONE single-device dynamic scene given the same calls;
 *   frames   every frame is bit for bit the single-device PtrFrame on that scene: state, resolved outputs and every PtrAdaptiveInfo.
 * They hold because an update is a function of the scene's arrays and the call's arguments alone, every partition starts from the same
 * upload, and every partition is given every call.
 *
 * An update call is
 *   1 checked once on the host, before any device work, against partition 0's records (all partitions hold the same): the rules and the
 *     words are those of the single-device call, behind this function's name.  A refusal leaves all partitions and the frame as they were;
 *   2 distributed: what the call's kernels read reaches every partition (below);
 *   3 run on every partition concurrently, each on its own stream: the single-device call's device work, unchanged;
 *   4 joined: every partition's stream is synchronised before the call returns.
 *
 * Distribution.
 *   matrices, sphere and rectangle rows   a few hundred bytes; each partition copies them from the host itself.
 *   host vertex data (set_mesh_vertices)  staged ONCE in portable pinned memory, each component looked at on the way (a non-finite one
 *            refuses the call); each partition copies it from there on its own stream.  It is not staged per partition.
 *   device vertex data (set_mesh_vertices_device)  the arrays live on src_device, any visible device, in the frame or not, and are ordered
 *            after `stream`, a stream of src_device.
 *              check    k_dyn_check_finite over the given arrays runs once, on src_device and `stream`, before anything is distributed;
 *                       its flag words are the one thing the host waits for on `stream` before the final join.  A set bit refuses the
 *                       call, every partition unchanged.
 *              order    an event recorded on `stream` behind the check (and behind the copies of the staged path); every partition's stream
 *                       waits on the event, the host does not.
 *              in place a partition on src_device (not forced) reads the arrays where they are.
 *              peer     a partition on a device that can address src_device pulls them with hipMemcpyPeerAsync on its own stream into a
 *                       buffer it keeps for the frame's life; the pulls of different partitions run side by side.
 *              staged   without peer access, or forced (below), the arrays go through the pinned memory ONCE for all such partitions, each
 *                       of which copies them from there; each is counted in stagedParts and a line goes to stderr, as for a resolve's gather.
 *            With PTR_DYNAMIC_VERTEX_NORMALS and null normals only positions (and tangents) travel; every partition computes the normals
 *            itself from its own adjacency and looks at them itself - every partition finds what partition 0 finds.
 *
 * Refusals after device work began.  A non-finite computed normal and the depth bounds of a rebuild (ptr_rebuild.h, step 8) are found on
 * the device, by every partition alike, before it changes anything the renderer reads: the call returns 1 with the single-device words,
 * all partitions unchanged, the frame usable.
 *
 * Rebuild.  The rebuild is a function of the leaf table and the current bounds, and the cost has a fixed summation order: every partition
 * reaches the same costBefore / costAfter, the same PTR_REBUILD_KEEP_IF_BETTER decision and the same tree.  ptr_multi_frame_rebuild_tree
 * checks that: partitions that disagree on the bits of either cost, on `installed`, on nodes, levels, wideNodes, wideDepth or leaves, or
 * of which one refuses and another does not, fail the frame with a message naming both devices.  ptr_multi_frame_tree_cost returns
 * partition 0's value.
 *
 * PtrMultiUpdateInfo.  The counts and boxes of an update are the same on all partitions by the first law, so `first` is partition 0's
 * PtrUpdateInfo; its times are partition 0's run half alone (step 3), as the single-device call reports them.  totalSeconds is the wall
 * time of the whole call, from its entry - steps 1 to 4, the staging of host vertex data in step 1 included - to the join.
 * distributeSeconds runs from the entry of the call to the moment the last partition has ENQUEUED the copies that bring it its inputs:
 * the checks, the staging of host data, the device-side check, the event and the staging copy all lie inside it; the copies themselves
 * run inside partSeconds[p], which is partition p's thread from its start to its stream joined.
 *
 * Sample state.  The law of ptr_dynamic.h: an update touches neither the sample state, nor the published halo rows, nor the count
 * classes.  The caller calls ptr_multi_frame_reset before accumulating the new pose; accumulating across poses without it is allowed and
 * gives what a single-device PtrFrame gives for the same calls, a blur over the poses.  Export / import do not carry the pose.
 *
 * Errors.  1 and a message that starts with the function's name: a null frame (or other null argument that is not named nullable), a
 * list that is null or empty, unknown flag bits, a negative src_device - these before the frame is looked at; a frame that is broken
 * or was not created dynamic (or without the flag the call needs: the single-device words); src_device at or past the visible count;
 * every rule of the single-device call.  2 and "no CPU fallback" from the create calls without a HIP device.  A device failure in one
 * partition ends the call on all, names that device and breaks the frame as in ptr_multi_frame.h; the partitions may then differ, so
 * only release is left.  Step 1 can be run alone, without a device, through ptr_multi_frame_debug_check_update.
 */
#ifndef PTR_MULTI_DYNAMIC_H
#define PTR_MULTI_DYNAMIC_H

#include "ptr_deform_device.h"
#include "ptr_multi_frame.h"
#include "ptr_rebuild.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrMultiUpdateInfo {
    uint32_t parts;                                /* partitions the update ran on */
    uint32_t stagedParts;                          /* partitions whose device vertex data came through pinned host memory */
    double totalSeconds;                           /* wall time of the call from its entry, checks, staging and join included */
    double distributeSeconds;                      /* from the entry of the call to the last partition having its inputs enqueued */
    double partSeconds[PTR_MULTI_MAX_PARTS];       /* partition p's thread, from its start to its stream joined */
    PtrUpdateInfo first;                           /* partition 0's */
} PtrMultiUpdateInfo;

int ptr_multi_frame_create_dynamic(const PtrSceneDesc* scene, const PtrSettings* settings, int n_devices, uint32_t dynamic_flags,
                                   PtrMultiFrame** out_frame, char* err, size_t err_cap);
/* Test only: the id-list semantics of ptr_multi_frame_debug_create_on.  An id given as -(id + 1) also forces that partition's device
 * vertex data through the pinned memory. */
int ptr_multi_frame_debug_create_dynamic_on(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t dynamic_flags, const int* device_ids,
                                            int n, PtrMultiFrame** out_frame, char* err, size_t err_cap);
int ptr_multi_frame_is_dynamic(const PtrMultiFrame* frame);
uint32_t ptr_multi_frame_dynamic_flags(const PtrMultiFrame* frame);

/* The update calls: the argument lists of ptr_scene_set_mesh_transforms, ptr_scene_set_mesh_vertices, ptr_scene_set_spheres and
 * ptr_scene_set_rects without the stream.  info is nullable. */
int ptr_multi_frame_set_mesh_transforms(PtrMultiFrame* frame, const PtrMeshTransform* transforms, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                        size_t err_cap);
int ptr_multi_frame_set_mesh_vertices(PtrMultiFrame* frame, const PtrMeshVertices* meshes, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                      size_t err_cap);
int ptr_multi_frame_set_spheres(PtrMultiFrame* frame, const PtrSphereUpdate* spheres, uint32_t count, PtrMultiUpdateInfo* info, char* err,
                                size_t err_cap);
int ptr_multi_frame_set_rects(PtrMultiFrame* frame, const PtrRectUpdate* rects, uint32_t count, PtrMultiUpdateInfo* info, char* err, size_t err_cap);
/* The arrays of `meshes` live on src_device and are ordered after `stream`, a stream of that device (Distribution). */
int ptr_multi_frame_set_mesh_vertices_device(PtrMultiFrame* frame, const PtrMeshVerticesDevice* meshes, uint32_t count, int src_device, void* stream,
                                             PtrMultiUpdateInfo* info, char* err, size_t err_cap);

int ptr_multi_frame_tree_cost(PtrMultiFrame* frame, double* cost, char* err, size_t err_cap);
/* flags: 0 or PTR_REBUILD_KEEP_IF_BETTER; info (nullable) is the one every partition reached, its times partition 0's. */
int ptr_multi_frame_rebuild_tree(PtrMultiFrame* frame, uint32_t flags, PtrRebuildInfo* info, char* err, size_t err_cap);

/* Partition p's scene, BORROWED: it lives as long as the frame and is never released by the caller.  The caller never passes it to an
 * update or rebuild call (ptr_scene_set_*, ptr_scene_rebuild_tree): that would desynchronise the partitions.  Rendering,
 * ptr_temporal_create / ptr_temporal_create_cov and the ptr_debug_scene_arrays / ptr_debug_rebuild_arrays probes may use it.  With p = 0
 * the whole pipeline runs on the frame's first device without a host round trip: update, reset, accumulate,
 * ptr_multi_frame_resolve_device, ptr_temporal_step_cov_device on this scene, ptr_denoise_cov_device.
 * NULL: a null frame, p past the partitions, a frame without scenes.  Works on static frames too. */
PtrDeviceScene* ptr_multi_frame_part_scene(PtrMultiFrame* frame, uint32_t p);

/* Test only, host only (no GPU): step 1 of an update call alone.  What ptr_multi_frame_set_mesh_transforms (kind 0),
 * _set_mesh_vertices (1, the look at every component included), _set_spheres (2) or _set_rects (3) says about `list` on a frame created
 * from `scene` with dynamic_flags: 0 when the call would go on to the devices, 1 and the call's own message when it is refused.  The
 * records it is checked against are made from the description as an upload makes them. */
int ptr_multi_frame_debug_check_update(const PtrSceneDesc* scene, uint32_t dynamic_flags, uint32_t kind, const void* list, uint32_t count, char* err,
                                       size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_MULTI_DYNAMIC_H */
