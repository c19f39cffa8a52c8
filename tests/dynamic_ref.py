"""numpy restatement of what a dynamic scene's update computes after the bake (include/ptr_dynamic.h): the refit of the float child boxes
by height level in float32 min / max, the grid rule and the quantiser in float64, and the copy into the four-wide nodes.  Inputs are the
arrays ptr_debug_dynamic_tables / ptr_debug_scene_arrays return; every result is compared bit for bit.

Node layout (64 B, 16 words): lo0 xyz, ref0, hi0 xyz, ref1, lo1 xyz, -, hi1 xyz, -.  A reference: 0xFFFFFFFF empty; bit 31 leaf, bit 30
sphere leaf, bits 26..29 primitive count - 1, bits 0..25 first primitive; otherwise the index of an internal node."""
import numpy as np

EMPTY = 0xFFFFFFFF
LEAF = 0x80000000
SPHERE = 0x40000000
OFFSET_MASK = 0x03FFFFFF
NO_SOURCE = 0xFFFFFFFF


def refs_of(nodes):
    w = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16).view(np.uint32)
    return w[:, [3, 7]].copy()


def heights(nodes):
    """Height of every node: 0 with only leaf children, else 1 + the largest height of its internal children (children follow parents)."""
    refs = refs_of(nodes)
    h = np.zeros(len(refs), np.int64)
    for i in range(len(refs) - 1, -1, -1):
        for r in refs[i]:
            if r != EMPTY and not (r & LEAF):
                h[i] = max(h[i], 1 + h[int(r)])
    return h


def refit(nodes, schedule, level_offsets, tri_bounds, sphere_bounds):
    """The float nodes with both child boxes of every node recomputed, level by level in the schedule's order."""
    out = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16).copy()
    refs = refs_of(out)
    tb = np.asarray(tri_bounds, np.float32).reshape(-1, 2, 4)
    sb = np.asarray(sphere_bounds, np.float32).reshape(-1, 2, 4)
    for level in range(len(level_offsets) - 1):
        for node in schedule[level_offsets[level]:level_offsets[level + 1]]:
            for c in range(2):
                r = int(refs[node, c])
                if r == EMPTY:
                    continue
                if r & LEAF:
                    first, count = r & OFFSET_MASK, ((r >> 26) & 0xF) + 1
                    b = (sb if r & SPHERE else tb)[first:first + count]
                    lo, hi = b[:, 0, :3].min(axis=0), b[:, 1, :3].max(axis=0)
                else:
                    kid, kid_refs = out[r], refs[r]
                    los = [kid[s * 8:s * 8 + 3] for s in range(2) if kid_refs[s] != EMPTY]
                    his = [kid[s * 8 + 4:s * 8 + 7] for s in range(2) if kid_refs[s] != EMPTY]
                    lo, hi = np.min(los, axis=0), np.max(his, axis=0)
                out[node, c * 8:c * 8 + 3] = lo
                out[node, c * 8 + 4:c * 8 + 7] = hi
    return out.reshape(-1, 4, 4)


def root_box(nodes):
    """Union of the children of node 0 that exist (None for a tree without nodes)."""
    n = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    if len(n) == 0:
        return None
    refs = refs_of(n)[0]
    los = [n[0, s * 8:s * 8 + 3] for s in range(2) if refs[s] != EMPTY]
    his = [n[0, s * 8 + 4:s * 8 + 7] for s in range(2) if refs[s] != EMPTY]
    return np.min(los, axis=0).astype(np.float32), np.max(his, axis=0).astype(np.float32)


def grid_of(lo, hi):
    """cell = extent / 65531 (1 without extent), origin = lo - 2 cell, in float64, stored as float32: [origin, cell]."""
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    ext = hi - lo
    cell = np.where(ext > 0, ext / 65531.0, 1.0)
    return np.stack([(lo - 2.0 * cell).astype(np.float32), cell.astype(np.float32)])


def quantise(nodes, grid):
    """The 32 B quantised nodes of the float nodes on `grid` ([origin, cell] float32): floor - 1 / ceil + 1 in float64, clamped to 0..65535."""
    n = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    refs = refs_of(n)
    origin, cell = np.asarray(grid, np.float32).astype(np.float64)
    q = np.zeros((len(n), 2, 4), np.uint32)
    for c in range(2):
        lo = (n[:, c * 8:c * 8 + 3].astype(np.float64) - origin) / cell
        hi = (n[:, c * 8 + 4:c * 8 + 7].astype(np.float64) - origin) / cell
        with np.errstate(invalid="ignore"):
            ql = np.clip(np.floor(lo) - 1.0, 0.0, 65535.0).astype(np.uint32)
            qh = np.clip(np.ceil(hi) + 1.0, 0.0, 65535.0).astype(np.uint32)
        words = np.stack([ql[:, 0] | (ql[:, 1] << 16), ql[:, 2] | (qh[:, 0] << 16), qh[:, 1] | (qh[:, 2] << 16)], axis=1)
        words[refs[:, c] == EMPTY] = 0
        q[:, c, :3] = words
        q[:, c, 3] = refs[:, c]
    return q


def wide_copy(wnodes, qnodes, wide_source):
    """The four-wide nodes with the three box words of every used place taken from its source record; reference words and unused places stay."""
    w = np.ascontiguousarray(wnodes, np.uint32).reshape(-1, 4).copy()
    src = np.asarray(wide_source, np.uint32).reshape(-1)
    used = src != NO_SOURCE
    recs = np.ascontiguousarray(qnodes, np.uint32).reshape(-1, 4)
    w[used, :3] = recs[src[used], :3]
    return w.reshape(-1, 4, 4)
