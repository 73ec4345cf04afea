"""The yardstick of the island tests: constraint islands of one world from its constraint rows, in numpy.

A row r < n has a set of kinematic trees T(r):

  EQUALITY, connect / weld        body_treeid of the two bodies (through site_bodyid with site semantics)
  FRICTION_DOF                    dof_treeid[efc_id]
  LIMIT_JOINT                     dof_treeid[jnt_dofadr[efc_id]]
  CONTACT_*, both geoms >= 0      body_treeid[geom_bodyid[g]] of both geoms; efc_id is the contact's slot
  every other row                 dof_treeid of the dofs whose entry in the row of J is non-zero

with tree ids < 0 (static bodies) dropped, and an id outside its array contributing nothing.  A tree in some T(r) is
constrained, every row joins the trees of its set, the islands are the connected components of the constrained
trees, numbered in ascending order of their smallest tree.  Written from that table; no code of any other
implementation is used.
"""

import numpy as np

EQUALITY, FRICTION_DOF, FRICTION_TENDON, LIMIT_JOINT, LIMIT_TENDON, CONTACT_FRICTIONLESS, CONTACT_PYRAMIDAL, CONTACT_ELLIPTIC = range(8)
CONTACTS = (CONTACT_FRICTIONLESS, CONTACT_PYRAMIDAL, CONTACT_ELLIPTIC)
EQ_CONNECT, EQ_WELD = 0, 1
OBJ_SITE = 6


def tree_ids(mjm):
  """(body_treeid, dof_treeid, ntree) of a host model: a tree starts at every dof without a parent dof; a body's
  tree is that of the dofs of the body it is welded to, -1 when that is the world."""
  nv = int(mjm.nv)
  dof_treeid = np.zeros(nv, dtype=np.int32)
  ntree = 0
  for v in range(nv):
    if mjm.dof_parentid[v] < 0:
      ntree += 1
    dof_treeid[v] = ntree - 1
  body_treeid = np.full(int(mjm.nbody), -1, dtype=np.int32)
  for b in range(int(mjm.nbody)):
    w = int(mjm.body_weldid[b])
    if w > 0:
      body_treeid[b] = dof_treeid[mjm.body_dofadr[w]]
  return body_treeid, dof_treeid, ntree


def model_ids(mjm):
  """The model's id arrays `islands` reads, as a dict."""
  body_treeid, dof_treeid, ntree = tree_ids(mjm)
  neq = int(getattr(mjm, "neq", 0))
  return dict(
    ntree=ntree, nv=int(mjm.nv), body_treeid=body_treeid, dof_treeid=dof_treeid, jnt_dofadr=np.asarray(mjm.jnt_dofadr),
    geom_bodyid=np.asarray(mjm.geom_bodyid), site_bodyid=np.asarray(mjm.site_bodyid),
    eq_type=np.asarray(mjm.eq_type)[:neq], eq_obj1id=np.asarray(mjm.eq_obj1id)[:neq], eq_obj2id=np.asarray(mjm.eq_obj2id)[:neq],
    eq_objtype=np.asarray(mjm.eq_objtype)[:neq],
  )


def _at(a, i):
  """a[i], or -1 when i is outside a."""
  return int(a[i]) if 0 <= i < len(a) else -1


def row_trees(ids, efc_type, efc_id, Jrow, contact_geom):
  """The set T(r) of one row (a Python set of tree ids)."""
  ntree = ids["ntree"]
  t, i = int(efc_type), int(efc_id)
  generic = False
  trees = []
  if t == EQUALITY:
    et = _at(ids["eq_type"], i)
    if et in (EQ_CONNECT, EQ_WELD):
      b = [int(ids["eq_obj1id"][i]), int(ids["eq_obj2id"][i])]
      if int(ids["eq_objtype"][i]) == OBJ_SITE:
        b = [_at(ids["site_bodyid"], x) for x in b]
      trees = [_at(ids["body_treeid"], x) for x in b]
    elif 0 <= i < len(ids["eq_type"]):
      generic = True
  elif t == FRICTION_DOF:
    trees = [_at(ids["dof_treeid"], i)]
  elif t == LIMIT_JOINT:
    trees = [_at(ids["dof_treeid"], _at(ids["jnt_dofadr"], i))]
  elif t in CONTACTS:
    if 0 <= i < len(contact_geom):
      g = [int(contact_geom[i][0]), int(contact_geom[i][1])]
      if g[0] >= 0 and g[1] >= 0:
        trees = [_at(ids["body_treeid"], _at(ids["geom_bodyid"], x)) for x in g]
      else:
        generic = True
  else:
    generic = True
  if generic:
    trees = [int(ids["dof_treeid"][v]) for v in np.nonzero(np.asarray(Jrow)[:ids["nv"]])[0]]
  return {x for x in trees if 0 <= x < ntree}


def islands(ids, efc_type, efc_id, J, contact_geom, n, njmax):
  """(nisland, tree_island (ntree,), dof_island (nv,), efc_island (njmax,)) of one world.  J: (>= n, >= nv) dense
  rows (rebuilt from the slots on the sparse path); contact_geom: the (slots, 2) array efc_id points into."""
  ntree, nv = ids["ntree"], ids["nv"]
  parent = list(range(ntree))

  def find(x):
    while parent[x] != x:
      x = parent[x]
    return x

  constrained = np.zeros(ntree, dtype=bool)
  any_tree = np.full(njmax, -1, dtype=np.int64)
  for r in range(n):
    T = sorted(row_trees(ids, efc_type[r], efc_id[r], J[r] if len(J) > r else (), contact_geom))
    for x in T:
      constrained[x] = True
      a, b = find(T[0]), find(x)
      if a != b:
        parent[max(a, b)] = min(a, b)
    if T:
      any_tree[r] = T[0]
  tree_island = np.full(ntree, -1, dtype=np.int32)
  nisland = 0
  for t in range(ntree):  # ascending: a component is met first at its smallest tree
    if not constrained[t]:
      continue
    root = find(t)
    if tree_island[root] < 0:
      tree_island[root] = nisland
      nisland += 1
    tree_island[t] = tree_island[root]
  dof_island = tree_island[ids["dof_treeid"]] if nv else np.zeros(0, dtype=np.int32)
  efc_island = np.full(njmax, -1, dtype=np.int32)
  for r in range(n):
    if any_tree[r] >= 0:
      efc_island[r] = tree_island[any_tree[r]]
  return nisland, tree_island, np.asarray(dof_island, dtype=np.int32), efc_island


def oracle_world(ids, od, w):
  """`islands` over world w of a CPU oracle Data (oracle/orc.py) after its position stage."""
  n = min(int(od.nefc[w, 0]), od.njmax)
  J = od.efc_J[w].reshape(od.njmax, ids["nv"]) if ids["nv"] else np.zeros((od.njmax, 0))
  return islands(ids, od.efc_type[w], od.efc_id[w], J, od.con_geom[w].reshape(-1, 2), n, od.njmax)


def device_rows(m, d, w):
  """World w's row arrays read back from a device Data: (efc_type, efc_id, dense J, n)."""
  n = max(0, min(int(d.nefc[w]), d.njmax))
  nv = m.nv
  if m.is_sparse:
    vals = d.efc.J[w, :, :n].cpu().numpy()
    cols = d.efc.J_colind[w, :, :n].cpu().numpy()
    nnz = d.efc.J_rownnz[w, :n].cpu().numpy()
    J = np.zeros((n, nv), dtype=np.float64)
    for r in range(n):
      for k in range(min(int(nnz[r]), vals.shape[0])):
        if vals[k, r] != 0.0 and 0 <= cols[k, r] < nv:
          J[r, cols[k, r]] = 1.0  # only the pattern matters
  else:
    J = d.efc.J[w, :n, :nv].cpu().numpy()
  return d.efc.type[w].cpu().numpy(), d.efc.id[w].cpu().numpy(), J, n


def device_world(ids, m, d, w, contact_geom=None):
  """`islands` over world w of a device Data, from its own rows read back."""
  efc_type, efc_id, J, n = device_rows(m, d, w)
  if contact_geom is None:
    contact_geom = d.contact.geom.cpu().numpy()
  return islands(ids, efc_type, efc_id, J, contact_geom, n, d.njmax)
