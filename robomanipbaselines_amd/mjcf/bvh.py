"""Bounding volume hierarchies of the render meshes, for the renderer's shadow rays.

The render triangles (mjcf/rmesh.py) are rigid in their body's frame, so each mesh slot gets one
static hierarchy over its triangles there, shared by every env and camera.  The shadow query
(csrc/rmbx_render.hip, include/rmbx.h rmbx_scene_tables) is an any-hit walk without a stack:

* the slot's triangles are ordered along a Morton curve of their centroids (through an index array:
  `rmesh_tri` itself keeps its order, which the visibility pass's triangle indices depend on) and cut
  into leaves of at most LEAF consecutive triangles;
* the tree over the leaves halves each range of leaves down to one; its nodes are numbered in
  depth-first order, so an inner node's first child is the next node and a subtree of m leaves holds
  2 m - 1 consecutive nodes;
* every node carries a skip link: the node to visit after a miss, or after a leaf's triangles -- the
  node after its subtree, -1 where that ends the slot's walk.

Tables: nodes f32 [nnode, 8] = (box min xyz, skip link, box max xyz, leaf word) with the two words
int32 bits (leaf word 0: an inner node; else (first entry of `tri` << 3) | number of triangles);
tri i32 [ntri]: triangle indices into rmesh_tri, leaf by leaf; root i32 [nslot]: each slot's root
node (-1 for a slot without triangles).  The boxes are padded by PAD metres and rounded outwards to
f32, so they contain their triangles whatever the rounding of the kernel's slab test.
"""

import numpy as np

LEAF = 4
PAD = 1e-5


def _morton(cen):
    """30-bit Morton keys of points [n, 3] within their bounding box."""
    lo, hi = cen.min(0), cen.max(0)
    q = ((cen - lo) / np.maximum(hi - lo, 1e-30) * 1023.0).astype(np.uint64)
    key = np.zeros(len(cen), np.uint64)
    for b in range(10):
        for a in range(3):
            key |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return key


def build_slot(verts):
    """One slot: verts [n, 3, 3] (f64, the triangles' corners in the body frame) -> (nodes [m, 8] f32
    with slot-relative links, tri [n] the slot-relative triangle order)."""
    n = len(verts)
    order = np.argsort(_morton(verts.mean(1)), kind="stable")
    nleaf = -(-n // LEAF)
    first = np.arange(nleaf) * LEAF
    count = np.minimum(first + LEAF, n) - first
    v = verts[order]
    llo = np.minimum.reduceat(v.min(1), first)
    lhi = np.maximum.reduceat(v.max(1), first)
    total = 2 * nleaf - 1
    blo, bhi = np.zeros((total, 3)), np.zeros((total, 3))
    skip, word = np.zeros(total, np.int32), np.zeros(total, np.int32)
    # top-down, one level at a time: (node, its range of leaves [a, b), its skip link)
    node, a, b, sk = np.zeros(1, np.int64), np.zeros(1, np.int64), np.array([nleaf], np.int64), np.array([total], np.int64)
    levels = []
    while len(node):
        skip[node] = np.where(sk == total, -1, sk)
        leaf = b - a == 1
        la = a[leaf]
        word[node[leaf]] = (first[la] << 3) | count[la]
        blo[node[leaf]], bhi[node[leaf]] = llo[la], lhi[la]
        node, a, b, sk = node[~leaf], a[~leaf], b[~leaf], sk[~leaf]
        mid = a + (b - a) // 2
        right = node + 2 * (mid - a)  # the left subtree's 2 (mid - a) - 1 nodes follow the node
        levels.append((node, node + 1, right))
        node, a, b, sk = (np.concatenate([node + 1, right]), np.concatenate([a, mid]), np.concatenate([mid, b]),
                          np.concatenate([right, sk]))
    for parent, left, right in reversed(levels):  # bottom-up: a node's box is its children's
        blo[parent] = np.minimum(blo[left], blo[right])
        bhi[parent] = np.maximum(bhi[left], bhi[right])
    nodes = np.zeros((total, 8), np.float32)
    lo32, hi32 = (blo - PAD).astype(np.float32), (bhi + PAD).astype(np.float32)
    nodes[:, 0:3] = np.nextafter(lo32, np.float32(-np.inf))
    nodes[:, 4:7] = np.nextafter(hi32, np.float32(np.inf))
    nodes[:, 3] = skip.view(np.float32)
    nodes[:, 7] = word.view(np.float32)
    return nodes, order.astype(np.int32)


def build(rmesh_tri, tri_adr, tri_num):
    """The shadow tables of a scene's render meshes (module docstring): dict of bvh_nodes [nnode, 8]
    f32, bvh_tri [ntri] i32, bvh_root [nslot] i32."""
    tri = np.asarray(rmesh_tri, np.float32)
    nodes_all, tri_all, roots = [], [], []
    nnode = 0
    for adr, num in zip(np.asarray(tri_adr, np.int64), np.asarray(tri_num, np.int64)):
        if num == 0:
            roots.append(-1)
            continue
        t = tri[adr:adr + num].astype(np.float64)
        verts = np.stack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]], 1)
        nodes, order = build_slot(verts)
        sk, wd = nodes[:, 3].view(np.int32), nodes[:, 7].view(np.int32)
        sk[sk >= 0] += nnode
        wd[wd != 0] += np.int32(sum(len(x) for x in tri_all) << 3)
        roots.append(nnode)
        nodes_all.append(nodes)
        tri_all.append(order + np.int32(adr))
        nnode += len(nodes)
    return {"bvh_nodes": np.ascontiguousarray(np.concatenate(nodes_all)) if nodes_all else np.zeros((0, 8), np.float32),
            "bvh_tri": np.concatenate(tri_all).astype(np.int32) if tri_all else np.zeros(0, np.int32),
            "bvh_root": np.asarray(roots, np.int32)}
