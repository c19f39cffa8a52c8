"""numpy restatement of steps 1-6 of include/ptr_rebuild.h, written from the header's text: the leaf table of a tree, the leaf boxes, the
Morton keys, the binary radix tree over the sorted keys and its preorder numbering.  Fit, grid, quantiser and wide copy are dynamic_ref's.
Inputs are the arrays ptr_debug_dynamic_tables / ptr_debug_scene_arrays return; every result is compared bit for bit."""
import numpy as np

import dynamic_ref as dr

KEY_MASK = 0x43FFFFFF


def leaf_table(nodes):
    """Step 1: the leaf references of the tree, ascending by (reference & 0x43FFFFFF)."""
    refs = dr.refs_of(nodes).reshape(-1)
    leaves = refs[(refs != dr.EMPTY) & ((refs & dr.LEAF) != 0)]
    return leaves[np.argsort(leaves & KEY_MASK, kind="stable")].astype(np.uint32)


def leaf_boxes(leaves, tri_bounds, sphere_bounds):
    """Step 2: float32 min / max union of the padded bounds of every leaf's primitives."""
    tb = np.asarray(tri_bounds, np.float32).reshape(-1, 2, 4)
    sb = np.asarray(sphere_bounds, np.float32).reshape(-1, 2, 4)
    lo, hi = np.zeros((len(leaves), 3), np.float32), np.zeros((len(leaves), 3), np.float32)
    for i, r in enumerate(int(x) for x in leaves):
        first, count = r & dr.OFFSET_MASK, ((r >> 26) & 0xF) + 1
        b = (sb if r & dr.SPHERE else tb)[first:first + count]
        lo[i], hi[i] = b[:, 0, :3].min(axis=0), b[:, 1, :3].max(axis=0)
    return lo, hi


def _spread(q):
    """bit k of a 10-bit value to bit 3k"""
    out = np.zeros(len(q), np.uint64)
    for k in range(10):
        out |= ((q >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def keys_of(lo, hi, root_lo, root_hi):
    """Step 3: code << 32 | leaf index, the code from the box centres in the root box, float64."""
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    rl, rh = np.asarray(root_lo, np.float32).astype(np.float64), np.asarray(root_hi, np.float32).astype(np.float64)
    m = (lo + hi) * 0.5
    ext = rh - rl
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(ext > 0, (m - rl) / np.where(ext > 0, ext, 1.0), 0.0)
    q = np.minimum(1023.0, np.maximum(0.0, np.floor(u * 1024.0))).astype(np.uint64)
    code = (_spread(q[:, 0]) << np.uint64(2)) | (_spread(q[:, 1]) << np.uint64(1)) | _spread(q[:, 2])
    return (code << np.uint64(32)) | np.arange(len(lo), dtype=np.uint64)


def _clz64(x):
    return 64 - x.bit_length()


def radix_tree(sorted_keys, leaves):
    """Steps 5-6: the [N - 1, 2] reference words of the binary radix tree over the sorted keys, nodes numbered in preorder.  The node of a
    range [first, last] splits it after the last position whose key shares more leading bits with key[first] than key[last] does."""
    keys = [int(k) for k in sorted_keys]
    n = len(keys)
    refs = np.full((max(n - 1, 0), 2), dr.EMPTY, np.uint32)
    if n < 2:
        return refs

    def leaf_ref(pos):
        return int(leaves[keys[pos] & 0xFFFFFFFF])

    def split(first, last):
        common = _clz64(keys[first] ^ keys[last])
        lo, hi = first, last - 1   # the largest s in [first, last - 1] with clz(key[first] ^ key[s]) > common (s = first always qualifies)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if mid == first or _clz64(keys[first] ^ keys[mid]) > common:
                lo = mid
            else:
                hi = mid - 1
        return lo

    next_index = 0
    stack = [(0, n - 1, -1, 0)]   # (first, last, parent, slot): preorder = parent, whole left subtree, then the right one
    while stack:
        first, last, parent, slot = stack.pop()
        if first == last:
            refs[parent, slot] = leaf_ref(first)
            continue
        index = next_index
        next_index += 1
        if parent >= 0:
            refs[parent, slot] = index
        s = split(first, last)
        stack.append((s + 1, last, index, 1))
        stack.append((first, s, index, 0))
    assert next_index == n - 1
    return refs


def nodes_of(refs):
    """64 B float nodes with these reference words and zero boxes (what the fit then fills)."""
    out = np.zeros((len(refs), 16), np.uint32)
    out[:, 3], out[:, 7] = refs[:, 0], refs[:, 1]
    return out.view(np.float32)


def rebuild(leaves, tri_bounds, sphere_bounds, root_lo, root_hi):
    """Steps 2-6 on a leaf table and the current bounds: the reference words of the new tree [N - 1, 2], and the sorted keys."""
    lo, hi = leaf_boxes(leaves, tri_bounds, sphere_bounds)
    keys = np.sort(keys_of(lo, hi, root_lo, root_hi))
    return radix_tree(keys, leaves), keys


def fitted(refs, tri_bounds, sphere_bounds):
    """The new tree's float nodes: dynamic_ref's heights, schedule and refit on the reference words.  Returns (nodes [n, 4, 4], schedule, level offsets)."""
    nodes = nodes_of(refs)
    h = dr.heights(nodes)
    levels = int(h.max()) + 1 if len(h) else 0
    schedule = np.concatenate([np.flatnonzero(h == l) for l in range(levels)]).astype(np.uint32) if levels else np.zeros(0, np.uint32)
    offsets = np.concatenate([[0], np.cumsum([int((h == l).sum()) for l in range(levels)])]).astype(np.uint32)
    return dr.refit(nodes, schedule, offsets, tri_bounds, sphere_bounds), schedule, offsets


def tree_cost(nodes):
    """The SAH figure of the header in float64 (any order of the sum: compared within a relative 1e-9)."""
    n = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    if len(n) == 0:
        return 0.0
    refs = dr.refs_of(n)
    if len(n) == 1 and refs[0, 1] == dr.EMPTY and refs[0, 0] & dr.LEAF:
        return float(((int(refs[0, 0]) >> 26) & 0xF) + 1)

    def half(lo, hi):
        d = hi.astype(np.float64) - lo.astype(np.float64)
        return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]

    rlo, rhi = dr.root_box(n)
    root_half = float(half(rlo, rhi))
    root_area = max(root_half, 1e-30)
    total = root_half / root_area
    for c in range(2):
        r = refs[:, c]
        weight = np.where((r & dr.LEAF) != 0, ((r >> 26) & 0xF) + 1, 1).astype(np.float64)
        weight[r == dr.EMPTY] = 0.0
        total += float(np.sum(half(n[:, c * 8:c * 8 + 3], n[:, c * 8 + 4:c * 8 + 7]) / root_area * weight))
    return total
