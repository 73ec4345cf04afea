"""Static bounding-volume hierarchies of the model's meshes, built on the host (numpy only).

One binary tree per mesh, in the mesh's own frame, over its triangles.  Meshes are rigid, so a tree is built once
(by `create_render_context`) and never refit.  The ray and render kernels (csrc/mjw_ray.h `mesh_bvh`) walk it in
place of the loop over every face.

Layout, all meshes in three flat arrays:

  node (nnode, 8) float32   words 0-2 the box minimum, 3-5 the box maximum, 6-7 two int32 (bit patterns, read them
                            with `.view(np.int32)`): an inner node holds (left child, right child | axis << 29),
                            child indices counted from the mesh's first node, axis = the split axis (the walk visits
                            the child on the ray's side first); a leaf holds (first triangle, -count), the offset
                            counted from the mesh's first entry of `tri`.  A leaf is the node with word 7 <= 0.
  tri  (nmeshface,) int32   face ids local to the mesh, grouped by leaf; mesh i owns the entries
                            mesh_faceadr[i] .. + mesh_facenum[i] (mesh_face itself is not reordered).
  adr  (nmesh, 4) int32     per mesh: first node (its root), number of nodes, first entry of `tri`, depth in levels.

Build: a node with more than BVH_LEAF triangles is split at the object median of the triangle centroids along the
longest axis of the centroid bounds, ties broken by face id, so duplicate triangles and coincident centroids
split like any others and the build always ends.  The halves hold ceil(n / 2) and floor(n / 2) triangles, hence a
tree over n triangles has at most ceil(log2(n / BVH_LEAF)) + 1 levels.  Nodes are numbered level by level, so a
child's index is always greater than its parent's.  A node's box is the exact float32 minimum / maximum of its
triangles' vertices.  The build runs level by level over all meshes at once.
"""

from __future__ import annotations

import numpy as np

BVH_LEAF = 4  # triangles per leaf at the most
BVH_MAX_DEPTH = 32  # levels; the device's traversal stack holds 64 entries
# Meshes with fewer faces keep the loop over their faces (RenderContext.bvh_min_faces, a host int the caller may
# change; 0 walks every mesh).  From the measurements in DESIGN.md section 3.7: on a single mesh of up to 37 faces
# the walk was never faster than the face loop (3 to 25 % slower), while in the aloha_pot scene, whose smallest
# meshes have 64 to 127 faces, leaving just those to the face loop costs a factor of 1.8.
BVH_MIN_FACES = 64
NODE_WORDS = 8
AXIS_SHIFT = 29


def depth_bound(nface: int) -> int:
  """Levels a tree over nface triangles has at the most: ceil(log2(nface / BVH_LEAF)) + 1."""
  n, k = max(int(nface), 1), 0
  while n > BVH_LEAF:
    n, k = (n + 1) // 2, k + 1
  return k + 1


def _ranges(start, count):
  """Concatenated aranges start[i] .. start[i] + count[i] and the segment id of every element."""
  seg = np.repeat(np.arange(len(count)), count)
  first = np.cumsum(count) - count
  return start[seg] + (np.arange(int(count.sum())) - first[seg]), seg, first


def build_mesh_bvh(mesh_vert, mesh_vertadr, mesh_face, mesh_faceadr, mesh_facenum):
  """(node, tri, adr, max_depth) for the host model's meshes (see the module docstring for the layout)."""
  vert = np.ascontiguousarray(np.asarray(mesh_vert, dtype=np.float32).reshape(-1, 3))
  face = np.asarray(mesh_face, dtype=np.int64).reshape(-1, 3)
  vertadr = np.asarray(mesh_vertadr, dtype=np.int64).reshape(-1)
  faceadr = np.asarray(mesh_faceadr, dtype=np.int64).reshape(-1)
  facenum = np.asarray(mesh_facenum, dtype=np.int64).reshape(-1)
  nmesh, nface = len(facenum), len(face)
  if nmesh == 0:
    return np.zeros((0, NODE_WORDS), np.float32), np.zeros(0, np.int32), np.zeros((0, 4), np.int32), 0
  assert len(vertadr) == nmesh and len(faceadr) == nmesh and np.all(facenum >= 0) and np.all(faceadr >= 0) and np.all(faceadr + facenum <= nface)

  # per face (global id): its mesh, its three vertices, centroid (float64 of the float32 vertices), vertex bounds
  fmesh = np.zeros(nface, dtype=np.int64)
  gid, seg, _ = _ranges(faceadr, facenum)
  fmesh[gid] = seg
  tv = vert[face + vertadr[fmesh][:, None]]  # (nface, 3, 3)
  cent = tv.astype(np.float64).mean(axis=1)
  flo, fhi = tv.min(axis=1), tv.max(axis=1)

  perm = np.arange(nface, dtype=np.int64)  # global face ids, reordered in place within each mesh's range
  # the level being split: one entry per node
  start, count, mesh_of = faceadr.copy(), facenum.copy(), np.arange(nmesh)
  local = np.zeros(nmesh, dtype=np.int64)  # node index within its mesh
  nnode = np.ones(nmesh, dtype=np.int64)
  depth = np.ones(nmesh, dtype=np.int64)
  levels = []  # per level: (mesh, local index, start, count, axis or -1, left child's local index)
  while len(start):
    big = count > BVH_LEAF
    axis = np.full(len(start), -1, dtype=np.int64)
    left = np.zeros(len(start), dtype=np.int64)
    nb = int(big.sum())
    if nb:
      idx, seg, first = _ranges(start[big], count[big])
      c = cent[perm[idx]]
      ext = np.maximum.reduceat(c, first, axis=0) - np.minimum.reduceat(c, first, axis=0)
      ax = ext.argmax(axis=1)
      key = c[np.arange(len(idx)), ax[seg]]
      order = np.lexsort((perm[idx], key, seg))  # by node, then centroid, then face id
      perm[idx] = perm[idx][order]
      axis[big] = ax
      # children are numbered in the order of their parents, after every node of this level
      m_big = mesh_of[big]
      change = np.r_[True, m_big[1:] != m_big[:-1]]
      run0 = np.maximum.accumulate(np.where(change, np.arange(nb), 0))
      rank = np.arange(nb) - run0  # this parent's rank among its mesh's split nodes of the level
      left[big] = nnode[m_big] + 2 * rank
    levels.append((mesh_of, local, start, count, axis, left))
    if not nb:
      break
    m_big, s, n = mesh_of[big], start[big], count[big]
    nl = (n + 1) // 2
    np.add.at(nnode, m_big, 2)
    depth[np.unique(m_big)] += 1
    assert depth.max() <= BVH_MAX_DEPTH, "mesh BVH deeper than the traversal stack allows"
    # interleave left and right children (the nodes of a mesh stay contiguous and in order)
    start = np.stack([s, s + nl], axis=1).reshape(-1)
    count = np.stack([nl, n - nl], axis=1).reshape(-1)
    mesh_of = np.repeat(m_big, 2)
    local = np.stack([left[big], left[big] + 1], axis=1).reshape(-1)

  nodeadr = np.cumsum(nnode) - nnode
  total = int(nnode.sum())
  lo = np.zeros((total, 3), dtype=np.float32)
  hi = np.zeros((total, 3), dtype=np.float32)
  ints = np.zeros((total, 2), dtype=np.int32)
  plo, phi = flo[perm], fhi[perm]
  for mesh_of, local, start, count, axis, left in reversed(levels):
    g = nodeadr[mesh_of] + local
    leaf = axis < 0
    if leaf.any():
      gl, s, n = g[leaf], start[leaf], count[leaf]
      full = n > 0  # (a mesh without faces has an empty root: a zero box and no triangle)
      if full.any():
        idx, seg, first = _ranges(s[full], n[full])
        lo[gl[full]] = np.minimum.reduceat(plo[idx], first, axis=0)
        hi[gl[full]] = np.maximum.reduceat(phi[idx], first, axis=0)
      ints[gl, 0] = s - faceadr[mesh_of[leaf]]
      ints[gl, 1] = -n
    inner = ~leaf
    if inner.any():
      gi, l = g[inner], nodeadr[mesh_of[inner]] + left[inner]
      lo[gi] = np.minimum(lo[l], lo[l + 1])
      hi[gi] = np.maximum(hi[l], hi[l + 1])
      ints[gi, 0] = left[inner]
      ints[gi, 1] = (left[inner] + 1) | (axis[inner] << AXIS_SHIFT)
  assert int(nnode.max()) < (1 << AXIS_SHIFT)

  node = np.zeros((total, NODE_WORDS), dtype=np.float32)
  node[:, 0:3], node[:, 3:6] = lo, hi
  node.view(np.int32)[:, 6:8] = ints
  tri = (perm - faceadr[fmesh[perm]]).astype(np.int32)
  for i in range(nmesh):
    assert depth[i] <= depth_bound(int(facenum[i]))
  adr = np.stack([nodeadr, nnode, faceadr, depth], axis=1).astype(np.int32)
  return node, tri, adr, int(depth.max())
