/*
 * ptr_rebuild.h — dynamic scenes of libptr_hip.so: the quality of a refitted tree, measured on the device, and a rebuild of the tree
 * above its leaves that runs where the data is and keeps every handle valid.
 *
 * The update calls of ptr_dynamic.h, ptr_deform.h and ptr_deform_device.h refit: the topology stays the upload's, and boxes that moved
 * far overlap more than a fresh tree's would.  ptr_scene_tree_cost says how much; ptr_scene_rebuild_tree builds a new topology over the
 * LEAVES of the upload's tree.  A leaf (a run of at most 8 primitives in leaf order) is one unit: leaf order does not change, so hit words,
 * tris / triNormals / triUv / triTangent, the bounds and object-space corner rows, the per-mesh lists, the sphere and rectangle tables, a
 * Temporal handle's pose snapshot and a Frame's state are all untouched, and no traversal or shading kernel changes - they read the
 * same SceneView with other node pointers.  A closest hit does not depend on the tree: on a scene without ties the image after a rebuild
 * is bit for bit the image before it.  What a rebuild cannot mend: leaf contents are never regrouped, so a deformation that tears a
 * leaf's own triangles apart still needs an upload.
 *
 * ---- tree cost ----
 * The builder's SAH figure (FlatBvh::sahCost) of the current float child boxes, in float64:
 *     halfArea(lo, hi) = dx dy + dy dz + dz dx with d = (double)hi - (double)lo
 *     rootBox  = union of the children of node 0 that exist;  rootArea = max(halfArea(rootBox), 1e-30)
 *     cost     = halfArea(rootBox) / rootArea                                              (node 0 itself)
 *              + sum over nodes, per child that exists, of halfArea(child box) / rootArea * (leaf child: primitive count; internal: 1)
 * An internal node's box is the one its parent stores.  The oversize leaf lies in no box and is left out.  Special cases, as in the
 * builder: a tree without nodes costs 0; a root whose only child is a leaf costs that leaf's primitive count.
 * One kernel, one node per lane; a block of 256 lanes sums its terms in index order, the host adds the block sums in block order: the
 * value is the same on every run.
 *
 * ---- rebuild ---- (N leaves; every step is restated in numpy by tests/rebuild_ref.py)
 *  1 leaf table   the leaf references of the upload's tree, ascending by (reference & 0x43FFFFFF): triangle leaves by first primitive,
 *                 then sphere leaves by first sphere.  Made once at upload; leaf index = position in this table.  A rebuild is a function
 *                 of the table and the current bounds, never of earlier rebuilds.
 *  2 leaf boxes   float32 min / max union of the leaf's padded primitive bounds (k_dyn_refit_level's leaf case).
 *  3 keys         rootLo / rootHi = the root box of the current tree (a rebuild does not change it).  Per axis, float64:
 *                 m = ((double)lo + (double)hi) * 0.5;  u = extent > 0 ? (m - rootLo) / (rootHi - rootLo) : 0;  q = min(1023, max(0, floor(u * 1024))).
 *                 30-bit Morton code: bit k of qx at 3k + 2, of qy at 3k + 1, of qz at 3k.  key = code << 32 | leaf index (unique).
 *  4 sort         keys ascending (rocprim radix sort).
 *  5 topology     the binary radix tree over the sorted keys with delta(i, j) = clz64(key_i ^ key_j), -1 for j outside 0 .. N - 1; one
 *                 internal node per lane (N - 1 of them), no communication between lanes.  The node of lane i covers a range of sorted
 *                 positions and splits it after position s: slot 0 is [first, s], slot 1 is [s + 1, last]; a range of one position is
 *                 that leaf's reference word, unchanged.
 *  6 numbering    preorder: node 0 is the root (the whole range), the left subtree follows its parent, the right one follows the left.
 *                 index = first + (number of left turns on the path from the root to the node), which a lane finds by walking up
 *                 to the root through parent words an earlier launch wrote (at most one step per key bit).
 *  7 heights, schedule, fit   height = 0 with only leaf children, else 1 + the largest height of the internal children.  Launch k
 *                 settles the nodes of height k from heights earlier launches wrote (kMaxTreeDepth - 1 launches); the schedule is the
 *                 stable sort of the node indices by height, the level offsets are where the height changes; the boxes are fitted by
 *                 k_dyn_refit_level, one launch per level.  No data is handed between workgroups inside a launch.
 *  8 depth bound  levels = height of node 0 + 1.  levels >= kMaxTreeDepth (48; the traversal stacks are sized by it) is refused with a
 *                 message, the scene unchanged; so is a four-wide tree with 3 x wideDepth + 4 > 76 stack entries.
 *  9 quantise     the grid rule on the new root box (the same box, so the same grid) and k_dyn_quantise.
 * 10 four-wide    WideCollapse::ByArea on the quantised records: the root is a wide root; one launch per wide level marks every
 *                 internal child a wide node of that level keeps; wide index = exclusive scan of the marks in binary-index order; per
 *                 wide root the reference words (internal ones renumbered), the unused places (inverted box, 0xFFFFFFFF) and the
 *                 wide-source table; box words by k_dyn_wide.
 * 11 install      everything above is built into a second set of arrays (allocated at the first call); the sets are swapped and
 *                 SceneView, the stack limit and the counts PtrUpdateInfo reports follow.  With PTR_REBUILD_KEEP_IF_BETTER only when
 *                 costAfter < costBefore: a radix tree over leaves can be worse than a lightly refitted SAH tree.
 * The node format (float, quantised binary, four-wide) stays the upload's.  A tree without nodes, a root that is a single leaf and a scene
 * of one leaf succeed with installed = 0.  After an installed rebuild every update call, Frame and Temporal handles and
 * ptr_debug_scene_arrays go on working, on the new topology.
 */
#ifndef PTR_REBUILD_H
#define PTR_REBUILD_H

#include "ptr_dynamic.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PTR_REBUILD_KEEP_IF_BETTER = 1 };

typedef struct PtrRebuildInfo {
    double totalSeconds;          /* host wall time of the call, the final synchronisation included */
    double costBefore, costAfter; /* ptr_scene_tree_cost of the tree the call found and of the one it built (equal for a no-op) */
    double keysSortMs, topologyMs, fitMs, quantiseMs, wideMs;   /* HIP-event times: steps 2-4, 5-6, 7, 9, 10 */
    uint64_t nodes, levels, wideNodes, wideDepth, leaves;       /* of the tree the scene has when the call returns; leaves = N */
    uint32_t installed;           /* 1: the new tree was swapped in */
    uint32_t pad;
} PtrRebuildInfo;

/* The SAH figure of the scene's current tree (above).  Runs on `stream` and ends with a stream synchronisation.  Refused before any
 * device work: a null scene or cost, a scene that is not dynamic. */
int ptr_scene_tree_cost(PtrDeviceScene* scene, void* stream, double* cost, char* err, size_t err_cap);

/* Rebuilds the tree above the leaves (above).  flags: 0 or PTR_REBUILD_KEEP_IF_BETTER.  Runs on `stream` and ends with a stream
 * synchronisation; renders of this scene on other streams must have finished.  Refused before any device work, the scene unchanged:
 * a null scene, a scene that is not dynamic, unknown flag bits.  Refused after device work, the scene unchanged: the depth bounds of
 * step 8.  info may be NULL. */
int ptr_scene_rebuild_tree(PtrDeviceScene* scene, uint32_t flags, void* stream, PtrRebuildInfo* info, char* err, size_t err_cap);

/* ---- test-only probes ----
 * The refit schedule (node indices grouped by height) and its level offsets of the scene as it is now, downloaded (what
 * ptr_debug_scene_arrays does for the other arrays); the wide-source table; {nodes, levels, wide nodes, wide depth, stack limit,
 * leaves} as uint32.  *size_out = bytes; out may be NULL.  1: bad argument, 2: cap_bytes too small, 3: the copy failed. */
enum {
    PTR_REBUILD_ARRAY_SCHEDULE = 0,
    PTR_REBUILD_ARRAY_LEVEL_OFFSETS = 1,
    PTR_REBUILD_ARRAY_WIDE_SOURCE = 2,
    PTR_REBUILD_ARRAY_INFO = 3,
    PTR_REBUILD_ARRAY_LEAF_TABLE = 4,
    PTR_REBUILD_ARRAY_POINTERS = 5   /* uint64: SceneView's nodes, qnodes, wnodes pointers */
};
int ptr_debug_rebuild_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out);

/* Host only (no GPU): the builder's own functions on a preorder array of `nodeCount` 64 B float nodes - the exact reference for what
 * steps 7-10 produce.  The schedule and level offsets of BuildRefitSchedule; the grid the shared rule derives from node 0 (origin xyz,
 * cell xyz); QuantiseNode's nodes on that grid; BuildWideNodes(ByArea) on them, its source table and its depth (one uint32); the SAH
 * figure above (one double); the leaf table of step 1; and the decision of step 8: {levels} as one uint32, refused when the rebuild
 * would refuse a tree of that depth.  Refused: null arguments, a reference that is neither empty, a leaf nor the index of a later node. */
enum {
    PTR_REBUILD_TABLE_SCHEDULE = 0,
    PTR_REBUILD_TABLE_LEVEL_OFFSETS = 1,
    PTR_REBUILD_TABLE_GRID = 2,
    PTR_REBUILD_TABLE_QNODES = 3,
    PTR_REBUILD_TABLE_WNODES = 4,
    PTR_REBUILD_TABLE_WIDE_SOURCE = 5,
    PTR_REBUILD_TABLE_WIDE_DEPTH = 6,
    PTR_REBUILD_TABLE_SAH = 7,
    PTR_REBUILD_TABLE_LEAF_TABLE = 8,
    PTR_REBUILD_TABLE_DEPTH_CHECK = 9
};
int ptr_debug_rebuild_tables(const float* nodes, uint32_t nodeCount, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out, char* err,
                             size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_REBUILD_H */
