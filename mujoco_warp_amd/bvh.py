"""Bounding-volume hierarchies built on the host (numpy only): the static trees of the model's meshes and, at the end
of the file, the tables of flex rendering, whose trees have a static topology and boxes the device refits.

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
# Flexes with fewer faces keep the loop over their faces (RenderContext.flex_bvh_min_faces, likewise a host int).  From
# the measurements in DESIGN.md section 3.11: on the 30 x 30 towel (3596 faces) the walk is 2.4 to 4.5 times faster than
# the face loop; where below that the two cross has not been measured, so the meshes' threshold is kept.
FLEX_BVH_MIN_FACES = BVH_MIN_FACES
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


# ---- flex rendering: the host-built tables of a render context made with render_flex ---------------------------------
#
# A flex's faces are not stored per world.  A face is three corner records (vertex, sign, source), and a corner's
# point is xpos[vertex] + sign * radius * n, n the vertex normal (source < 0) or the flat normal of element `source`;
# sign 0 is the vertex itself.  Faces per flex (mujoco_warp/_src/bvh.py:608-975):
#   dim 2   element e = (v0, v1, v2): face 2e = (v0+, v1+, v2+), face 2e + 1 = (v0-, v2-, v1-); then boundary fragment
#           s = (i0, i1), an edge with one element only, in edge order: face 2 nelem + 2s = (i0+, i1-, i1+) and the
#           next (i1-, i0+, i0-).  With smooth = False the element faces take the element's flat normal; the fragment
#           faces keep the vertex normals.
#   dim 3   one face per flex_shell triangle, the vertices themselves
#   dim 1   none (the edges are drawn as capsules)
# Every id in the tables is global: flex_vertadr / flex_elemadr are already added.
FLEX_INFO_WORDS = 12


def flex_rest_xpos(mjm):
  """World positions of the flex vertices at qpos0, (nflexvert, 3) float64: the vertex bodies' frames composed down
  the body tree (at qpos0 a joint adds nothing to its body's frame)."""
  nbody = int(mjm.nbody)
  pos = np.asarray(mjm.body_pos, dtype=np.float64).reshape(nbody, 3)
  quat = np.asarray(mjm.body_quat, dtype=np.float64).reshape(nbody, 4)
  parent = np.asarray(mjm.body_parentid).reshape(nbody)
  xpos, xquat = np.zeros((nbody, 3)), np.zeros((nbody, 4))
  xquat[0] = [1.0, 0.0, 0.0, 0.0]

  def mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])

  def rot(q, v):
    u = q[1:]
    return v + 2.0 * np.cross(u, np.cross(u, v) + q[0] * v)

  for b in range(1, nbody):  # parents come before their children
    p = int(parent[b])
    xpos[b] = xpos[p] + rot(xquat[p], pos[b])
    xquat[b] = mul(xquat[p], quat[b] / max(np.linalg.norm(quat[b]), 1e-300))
  return xpos[np.asarray(mjm.flex_vertbodyid, dtype=np.int64).reshape(-1)]


def flex_vertex_normals(xpos, elem_vert, inc_adr, inc):
  """(nflexvert, 3) float64: per vertex the normalised sum of the unit normals of its incident dim-2 elements; a zero
  sum, and a zero-area element's normal, stay zero."""
  x = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)
  ev = np.asarray(elem_vert, dtype=np.int64).reshape(-1, 3)
  n = np.cross(x[ev[:, 1]] - x[ev[:, 0]], x[ev[:, 2]] - x[ev[:, 0]]) if len(ev) else np.zeros((0, 3))
  ln = np.linalg.norm(n, axis=1, keepdims=True)
  n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
  out = np.zeros_like(x)
  for v in range(len(x)):
    for e in inc[inc_adr[v] : inc_adr[v + 1]]:
      out[v] += n[e]
  ln = np.linalg.norm(out, axis=1, keepdims=True)
  return np.where(ln > 0, out / np.where(ln > 0, ln, 1.0), 0.0), n


def flex_face_points(corner, face_radius, xpos, vert_norm, elem_norm):
  """(nface, 3, 3) float64: the points of the corner records (what the device makes on the fly)."""
  c = np.asarray(corner, dtype=np.int64).reshape(-1, 3, 3)
  x = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)
  vert, sign, src = c[..., 0], c[..., 1], c[..., 2]
  n = np.where((src < 0)[..., None], np.asarray(vert_norm)[vert], np.asarray(elem_norm).reshape(-1, 3)[np.maximum(src, 0)] if len(elem_norm) else 0.0)
  return x[vert] + (sign * np.asarray(face_radius, dtype=np.float64).reshape(-1, 1))[..., None] * n


def flex_levels(node, adr):
  """Per tree depth + 1 local node indices: the first node of each level, then the node count (nodes are numbered
  level by level, so a level is a contiguous range).  Returns (level, leveladr)."""
  ints = np.ascontiguousarray(node).view(np.int32).reshape(-1, NODE_WORDS)[:, 6:8]
  level, leveladr = [], []
  for nadr, nnode, _, depth in np.asarray(adr).reshape(-1, 4):
    lvl = np.zeros(nnode, dtype=np.int64)
    for i in range(nnode):
      a, b = int(ints[nadr + i, 0]), int(ints[nadr + i, 1])
      if b > 0:
        lvl[a] = lvl[b & ((1 << AXIS_SHIFT) - 1)] = lvl[i] + 1
    assert np.all(np.diff(lvl) >= 0) and int(lvl.max()) + 1 == depth
    leveladr.append(len(level))
    level += [int(np.searchsorted(lvl, k)) for k in range(depth)] + [int(nnode)]
  return np.asarray(level, dtype=np.int32), np.asarray(leveladr, dtype=np.int32)


def build_flex_tables(mjm, smooth=True):
  """The host tables of flex rendering as a dict of numpy arrays: info (nflex, 12) int32 (dim, vertadr, vertnum, first
  face, faces, first node, nodes, depth, first level entry, edgeadr, edgenum, 0), corner (nface, 3, 3), elem_vert
  (nflexelem, 3; zero rows for elements that are no triangles), edge_vert (nflexedge, 2), the vertex -> element CSR
  inc_adr / inc (ascending), frag (per flex its boundary fragments, global vertex ids), and one static tree per flex
  from build_mesh_bvh over the rest-pose faces (smooth normals whatever `smooth`): node, tri, adr, level, depth."""
  nflex, nvert, nelem = int(mjm.nflex), int(mjm.nflexvert), int(mjm.nflexelem)
  I = lambda name: np.asarray(getattr(mjm, name), dtype=np.int64)
  dim, vertadr, vertnum = I("flex_dim").reshape(-1), I("flex_vertadr").reshape(-1), I("flex_vertnum").reshape(-1)
  elemadr, elemnum, elemdataadr = I("flex_elemadr").reshape(-1), I("flex_elemnum").reshape(-1), I("flex_elemdataadr").reshape(-1)
  edgeadr, edgenum = I("flex_edgeadr").reshape(-1), I("flex_edgenum").reshape(-1)
  shelladr, shellnum = I("flex_shelldataadr").reshape(-1), I("flex_shellnum").reshape(-1)
  elem, shell = I("flex_elem").reshape(-1), I("flex_shell").reshape(-1)
  edge, flap = I("flex_edge").reshape(-1, 2), I("flex_edgeflap").reshape(-1, 2)
  radius = np.asarray(mjm.flex_radius, dtype=np.float64).reshape(-1)

  elem_vert = np.zeros((nelem, 3), dtype=np.int64)
  edge_vert = np.zeros((len(edge), 2), dtype=np.int64)
  inc = [[] for _ in range(nvert)]
  corner, corner_smooth, frags, face_radius, faceadr, facenum = [], [], [], [], [], []
  for f in range(nflex):
    va, ne = int(vertadr[f]), int(elemnum[f])
    edge_vert[edgeadr[f] : edgeadr[f] + edgenum[f]] = edge[edgeadr[f] : edgeadr[f] + edgenum[f]] + va
    frag = np.zeros((0, 2), dtype=np.int64)
    if dim[f] == 2:
      el = elem[elemdataadr[f] : elemdataadr[f] + 3 * ne].reshape(ne, 3) + va
      ge = elemadr[f] + np.arange(ne)
      elem_vert[ge] = el
      for e in range(ne):
        for v in el[e]:
          inc[v].append(int(ge[e]))
      sl = slice(int(edgeadr[f]), int(edgeadr[f] + edgenum[f]))
      frag = edge_vert[sl][flap[sl, 1] == -1]
      nf = len(frag)
      c = np.zeros((2 * ne + 2 * nf, 3, 3), dtype=np.int64)
      c[..., 2] = -1
      c[0 : 2 * ne : 2, :, 0], c[0 : 2 * ne : 2, :, 1] = el, 1
      c[1 : 2 * ne : 2, :, 0], c[1 : 2 * ne : 2, :, 1] = el[:, [0, 2, 1]], -1
      i0, i1 = frag[:, 0], frag[:, 1]
      c[2 * ne :: 2, :, 0], c[2 * ne :: 2, :, 1] = np.stack([i0, i1, i1], axis=1), [1, -1, 1]
      c[2 * ne + 1 :: 2, :, 0], c[2 * ne + 1 :: 2, :, 1] = np.stack([i1, i0, i0], axis=1), [-1, 1, -1]
      cs = c.copy()
      if not smooth:
        c[0 : 2 * ne : 2, :, 2] = c[1 : 2 * ne : 2, :, 2] = ge[:, None]
    elif dim[f] == 3:
      ns = int(shellnum[f])
      c = np.zeros((ns, 3, 3), dtype=np.int64)
      c[..., 0] = shell[shelladr[f] : shelladr[f] + 3 * ns].reshape(ns, 3) + va
      c[..., 2] = -1
      cs = c
    else:
      c = cs = np.zeros((0, 3, 3), dtype=np.int64)
    faceadr.append(sum(facenum))
    facenum.append(len(c))
    corner.append(c)
    corner_smooth.append(cs)
    frags.append(frag)
    face_radius.append(np.full(len(c), radius[f]))
  cat = lambda parts, tail: np.concatenate(parts, axis=0) if parts else np.zeros((0,) + tail, dtype=np.int64)
  corner, corner_smooth = cat(corner, (3, 3)), cat(corner_smooth, (3, 3))
  face_radius = np.concatenate(face_radius) if face_radius else np.zeros(0)
  inc_adr = np.concatenate([[0], np.cumsum([len(x) for x in inc])]).astype(np.int64)
  inc_flat = np.asarray([e for x in inc for e in x], dtype=np.int64)

  # the static topology: build_mesh_bvh over the rest-pose faces, each face its own three "vertices"
  nface = len(corner)
  if nflex:
    rest = flex_rest_xpos(mjm)
    vn, en = flex_vertex_normals(rest, elem_vert, inc_adr, inc_flat)
    pts = flex_face_points(corner_smooth, face_radius, rest, vn, en).reshape(-1, 3)
    fa = np.asarray(faceadr, dtype=np.int64)
    local = np.arange(nface) - np.repeat(fa, facenum)
    face = 3 * local[:, None] + np.arange(3)[None, :]
    node, tri, adr, depth = build_mesh_bvh(pts, 3 * fa, face, fa, facenum)
  else:
    node, tri, adr, depth = build_mesh_bvh(np.zeros((0, 3)), [], np.zeros((0, 3)), [], [])
  level, leveladr = flex_levels(node, adr)
  info = np.zeros((nflex, FLEX_INFO_WORDS), dtype=np.int32)
  if nflex:
    info[:, 0], info[:, 1], info[:, 2], info[:, 3], info[:, 4] = dim, vertadr, vertnum, faceadr, facenum
    info[:, 5], info[:, 6], info[:, 7], info[:, 8], info[:, 9], info[:, 10] = adr[:, 0], adr[:, 1], adr[:, 3], leveladr, edgeadr, edgenum
  i32 = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.int32))
  return dict(info=info, corner=i32(corner), elem_vert=i32(elem_vert), edge_vert=i32(edge_vert), inc_adr=i32(inc_adr), inc=i32(inc_flat),
              frag=frags, node=node, tri=tri, adr=adr, level=level, depth=int(depth), face_radius=face_radius)
