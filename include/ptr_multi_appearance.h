/* Appearance updates for frames on several devices: the calls of ptr_appearance.h - whole materials (and with them emission and the
 * rectangle-light table), the pixels of material textures, the pixels of the environment map - on a PtrMultiFrame (ptr_multi_frame.h),
 * on all its devices in place.  A relit or re-textured pose rendered on P devices costs one call, not a ptr_multi_frame_create of the
 * edited description.
 * Kernels: none of its own.  The per-device work of a call is csrc/kernels/appearance.hip (and k_dyn_check_finite of dynamic.hip) as
 * ptr_appearance.h runs them, on each partition's own stream.  Host: csrc/host/multi_appearance.cpp, over the partition driver of
 * multi_frame.cpp (csrc/host/multi_frame_host.h), the steps it shares with multi_dynamic.cpp (csrc/host/multi_update_host.h) and the two
 * halves of every single-device call (csrc/host/dynamic_host.h, appearance.cpp).
 *
 * ---- The specification (host code and tests are written from this text) ------------------------------------------------------------
 *
 * The two laws.  Those of ptr_multi_dynamic.h, extended.
 *   arrays   after any sequence of the calls below and of the calls of ptr_multi_dynamic.h, every array of every partition's scene -
 *            every selector of ptr_debug_appearance_arrays with its PTR_APPEARANCE_SCALARS, ptr_debug_scene_arrays,
 *            ptr_debug_rebuild_arrays but the device pointers - is bit for bit that of ONE single-device scene given the same calls.  By
 *            the law of ptr_appearance.h they are then also those of a fresh upload of the edited description;
 *   frames   every frame accumulated after ptr_multi_frame_reset is bit for bit the single-device PtrFrame on that scene: state,
 *            resolved outputs and every PtrAdaptiveInfo.
 * They hold because a call is a function of the scene's arrays, its host-side records and the call's arguments alone, every partition
 * starts from the same upload, and every partition is given every call.
 *
 * Which frames.  The single-device calls work on static scenes, so these work on a frame made by ptr_multi_frame_create as well as on
 * one made by ptr_multi_frame_create_dynamic.  The single-device exception carries over with the single-device words: when a rectangle
 * uses a named material the frame must have been created dynamic with PTR_DYNAMIC_PRIMITIVES.  What the calls distribute through (the
 * portable pinned memory, the per-source-device scratch and event) is made by the first call that needs it: a static frame that never
 * receives a call here allocates nothing new, and it refuses every call of ptr_multi_dynamic.h exactly as before.
 *
 * A call is the four steps of ptr_multi_dynamic.h:
 *   1 checked once on the host, before any device work that writes what a renderer reads, against partition 0's records (all
 *     partitions hold the same): the rules, their order and their words are those of the single-device call (ptr_appearance.h), behind
 *     this function's name.  A refusal leaves all partitions and the frame as they were;
 *   2 distributed: what the call's kernels read reaches every partition (below);
 *   3 run on every partition concurrently, each on its own stream: the single-device call's device work, unchanged;
 *   4 joined: every partition's stream is synchronised before the call returns.
 *
 * Distribution.
 *   materials     the rows, the key table and the light table are a few KB; each partition copies them from the host itself.
 *   host pixels   (set_textures, set_environment) staged ONCE in the frame's portable pinned memory, each component looked at on the way
 *            (a non-finite one refuses the call in step 1); each partition copies them from there on its own stream.  They are not
 *            staged per partition: hostStagedBytes is the payload once, whatever the number of partitions.
 *   device pixels (set_textures_device, set_environment_device) the arrays live on src_device, any visible device, in the frame or not,
 *            and are ordered after `stream`, a stream of src_device.  The pointer checks of the single-device call are made against
 *            src_device.  Then, as for the vertex arrays of ptr_multi_frame_set_mesh_vertices_device:
 *              check    k_dyn_check_finite over the given arrays runs once, on src_device and `stream`, before anything is distributed;
 *                       a set bit refuses the call with the single-device words, every partition unchanged.  No partition repeats it.
 *              order    an event recorded on `stream` behind the check (and behind the copies of the staged path); every partition's
 *                       stream waits on the event, the host does not.
 *              in place a partition on src_device (not forced) reads the arrays where they are.
 *              peer     a partition on a device that can address src_device pulls them with hipMemcpyPeerAsync on its own stream into
 *                       the buffer it keeps for the frame's life.
 *              staged   without peer access, or forced (an id given as -(id + 1) to the test-only create calls), the arrays go through
 *                       the pinned memory ONCE for all such partitions, each of which copies them from there; each is counted in
 *                       stagedParts and a line goes to stderr.
 *
 * Environment.  Every partition runs the whole rebuild of ptr_appearance.h itself - weights, the sequential total, alias tables, pdf -
 * and reads its own total: the total is a function of the pixels alone, in a fixed order, so every partition reaches the same decision
 * about sampling.  After the join the partitions' envSampling and lightsAfter are compared, as ptr_multi_frame_rebuild_tree compares its
 * infos (every call here does so): partitions that disagree fail the frame with a message naming both devices.  The mip chain a render
 * with PTR_METAL_ENV_LOD builds lazily is rebuilt on each partition that has one.
 *
 * PtrMultiAppearanceInfo.  `first` is partition 0's PtrAppearanceInfo: its counts are those of every partition by the first law, its
 * times partition 0's run half alone, as the single-device call reports them (its clock starts at the check of step 1).  totalSeconds,
 * distributeSeconds and partSeconds are those of PtrMultiUpdateInfo: the wall time of the whole call from its entry to the join; from
 * the entry to the moment the last partition has ENQUEUED the copies that bring it its inputs (for materials: to the moment the last
 * partition's run half begins, whose own copies bring the rows); partition p's thread from its start to its stream joined.
 *
 * Sample state.  The law of ptr_appearance.h: nothing tells the frame about an edit.  A call touches neither the sample state, nor the
 * published halo rows, nor the count classes; the caller calls ptr_multi_frame_reset before accumulating the edited scene.
 *
 * Errors.  As ptr_multi_dynamic.h: 1 and a message that starts with the function's name.  A null frame, a null or empty list (null
 * pixels for the environment), a negative src_device ("no such HIP device") - these before the frame is looked at; a frame that is
 * broken or has no scene; src_device at or past the visible count ("no such HIP device"); every rule of the single-device call.  A
 * device failure in one partition ends the call on all, names that device and breaks the frame as in ptr_multi_frame.h; the partitions
 * may then differ, so only release is left.  Step 1 can be run alone, without a device, through ptr_multi_frame_debug_check_appearance.
 */
#ifndef PTR_MULTI_APPEARANCE_H
#define PTR_MULTI_APPEARANCE_H

#include "ptr_appearance.h"
#include "ptr_multi_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrMultiAppearanceInfo {
    uint32_t parts;                                /* partitions the call ran on */
    uint32_t stagedParts;                          /* partitions whose DEVICE pixels came through pinned host memory */
    uint64_t hostStagedBytes;                      /* bytes of caller pixels written into pinned memory on the host by this call: the
                                                      payload once, whatever `parts` is; 0 for materials and the device forms */
    double totalSeconds;                           /* wall time of the call from its entry, checks, staging and join included */
    double distributeSeconds;                      /* from the entry of the call to the last partition having its inputs enqueued */
    double partSeconds[PTR_MULTI_MAX_PARTS];       /* partition p's thread, from its start to its stream joined */
    PtrAppearanceInfo first;                       /* partition 0's */
} PtrMultiAppearanceInfo;

/* The argument lists of ptr_scene_set_materials, ptr_scene_set_textures and ptr_scene_set_environment without the stream.  info is
 * nullable. */
int ptr_multi_frame_set_materials(PtrMultiFrame* frame, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, PtrMultiAppearanceInfo* info,
                                  char* err, size_t err_cap);
int ptr_multi_frame_set_textures(PtrMultiFrame* frame, const PtrTextureUpdate* textures, uint32_t count, PtrMultiAppearanceInfo* info, char* err,
                                 size_t err_cap);
int ptr_multi_frame_set_environment(PtrMultiFrame* frame, const float* rgba, uint32_t width, uint32_t height, PtrMultiAppearanceInfo* info, char* err,
                                    size_t err_cap);
/* The pixel arrays live on src_device and are ordered after `stream`, a stream of that device (Distribution). */
int ptr_multi_frame_set_textures_device(PtrMultiFrame* frame, const PtrTextureUpdate* textures, uint32_t count, int src_device, void* stream,
                                        PtrMultiAppearanceInfo* info, char* err, size_t err_cap);
int ptr_multi_frame_set_environment_device(PtrMultiFrame* frame, const float* rgba, uint32_t width, uint32_t height, int src_device, void* stream,
                                           PtrMultiAppearanceInfo* info, char* err, size_t err_cap);

/* Test only, host only (no GPU): step 1 of a call alone.  What ptr_multi_frame_set_materials (kind 0: list = the indices, materials,
 * count), ptr_multi_frame_set_textures (kind 1: list = the PtrTextureUpdate list, count; the look at every component included) or
 * ptr_multi_frame_set_environment (kind 2: list = the pixels, width, height; the look at every component included) says on a frame
 * created from `scene` - static when dynamic_flags is 0, else dynamic with these flags: 0 when the call would go on to the devices, 1 and
 * the call's own message when it is refused.  Arguments a kind does not use are ignored.  The records it is checked against are made
 * from the description as an upload makes them. */
int ptr_multi_frame_debug_check_appearance(const PtrSceneDesc* scene, uint32_t dynamic_flags, uint32_t kind, const void* list, const PtrMaterial* materials,
                                           uint32_t count, uint32_t width, uint32_t height, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif /* PTR_MULTI_APPEARANCE_H */
