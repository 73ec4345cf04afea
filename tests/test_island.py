"""Constraint islands, host side: the public surface (mjw.island, the four Data arrays, Model.body_treeid /
dof_treeid, the mjw_island entry point and its side struct), and the yardstick tests/island_ref.py pinned on the
hand-written expectations of tests/island_scenes.py over the CPU oracle's rows.  The kernel is tested in
tests/test_gpu_island.py.
"""

import ctypes

import numpy as np
import pytest

from tests import island_ref as ir
from tests import island_scenes as sc
from tests.common import oracle_from_state


def _small(nworld=3, njmax=20):
  import mujoco_warp_amd as mjw

  mjm = sc.BY_ID["two_pairs"].model()
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=nworld, njmax=njmax, nconmax=4, device="cpu", m=m)
  return mjw, mjm, m, d


# ---- surface ----------------------------------------------------------------------------------------
def test_island_is_exported():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib

  assert callable(mjw.island)
  assert "mjw_island" in _lib.ENTRY_POINTS and "mjw_island_t" in _lib._H


def test_data_has_the_four_arrays_and_reset_restores_them():
  import torch

  mjw, mjm, m, d = _small()
  for make in (lambda: d, lambda: mjw.put_data(mjm, mjw.MjData(mjm), nworld=3, njmax=20, nconmax=4, device="cpu", m=m)):
    dd = make()
    assert tuple(dd.nisland.shape) == (3,) and tuple(dd.tree_island.shape) == (3, m.ntree) == (3, 4)
    assert tuple(dd.dof_island.shape) == (3, mjm.nv) and tuple(dd.efc_island.shape) == (3, 20)
    assert all(t.dtype == torch.int32 for t in (dd.nisland, dd.tree_island, dd.dof_island, dd.efc_island))
    assert not dd.nisland.any()
    assert all(bool((t == -1).all()) for t in (dd.tree_island, dd.dof_island, dd.efc_island))
  for t in (d.nisland, d.tree_island, d.dof_island, d.efc_island):
    t.fill_(5)
  mjw.reset_data(m, d, torch.tensor([True, False, True]))
  assert d.nisland.tolist() == [0, 5, 0]
  for t in (d.tree_island, d.dof_island, d.efc_island):
    assert t[:, 0].tolist() == [-1, 5, -1] and bool((t[1] == 5).all())
  mjw.reset_data(m, d)
  assert not d.nisland.any() and all(bool((t == -1).all()) for t in (d.tree_island, d.dof_island, d.efc_island))


TREE_XML = """<mujoco><worldbody>
<body name="static" pos="0 0 1"><geom type="sphere" size=".1"/></body>
<body name="mover" pos="1 0 1"><freejoint/><geom type="sphere" size=".1"/>
  <body name="welded_child" pos="0 0 .2"><geom type="sphere" size=".05"/>
    <body name="hinged" pos="0 0 .2"><joint type="hinge" axis="0 1 0"/><geom type="sphere" size=".05"/></body></body></body>
<body name="jointless" pos="2 0 1"><geom type="sphere" size=".1"/>
  <body name="fixed_child" pos="0 0 .2"><geom type="sphere" size=".05"/>
    <body name="grandchild" pos="0 0 .2"><joint type="slide" axis="0 0 1"/><geom type="sphere" size=".05"/>
      <body name="leaf" pos="0 0 .2"><joint type="ball"/><geom type="sphere" size=".05"/></body></body></body></body>
</worldbody></mujoco>"""


def test_put_model_tree_ids():
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(TREE_XML)
  m = mjw.put_model(mjm, device="cpu")
  assert m.ntree == 2
  # world, static, mover, welded_child, hinged, jointless, fixed_child, grandchild, leaf
  assert m.body_treeid.tolist() == [-1, -1, 0, 0, 0, -1, -1, 1, 1]
  assert m.dof_treeid.tolist() == [0] * 7 + [1] * 4
  body_treeid, dof_treeid, ntree = ir.tree_ids(mjm)  # the yardstick's own derivation agrees
  assert ntree == 2 and body_treeid.tolist() == m.body_treeid.tolist() and dof_treeid.tolist() == m.dof_treeid.tolist()
  empty = mjw.put_model(mjw.load_model_from_string('<mujoco><worldbody><geom type="plane" size="1 1 .1"/></worldbody></mujoco>'), device="cpu")
  assert empty.ntree == 0 and empty.dof_treeid.numel() == 0 and empty.body_treeid.tolist() == [-1]


def test_struct_mirror_abi_and_cap():
  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.island import ISLAND_LDS_TREES

  assert ctypes.sizeof(_lib.CIsland) == 2 * 4 + 6 * 8
  L = _lib.lib()
  assert L.mjw_sizeof_island() == ctypes.sizeof(_lib.CIsland)
  assert L.mjw_island_lds_trees() == ISLAND_LDS_TREES
  assert _lib.ABI_VERSION == 36 and L.mjw_abi_version() == 36


def test_mjw_island_argument_checks_without_a_launch():
  """Null pointers and a wrong ntree come back through mjw_last_error; nworld == 0 returns 0 (no GPU here)."""
  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.io import cdata, cmodel
  from mujoco_warp_amd.island import _cisland

  mjw, _, m, d = _small()
  L = _lib.lib()
  ci = _cisland(m, d)
  assert L.mjw_island(None, cdata(d), ci, None) == -1
  assert b"mjw_island" in L.mjw_last_error() and b"null" in L.mjw_last_error()
  assert L.mjw_island(cmodel(m), None, ci, None) == -1
  assert L.mjw_island(cmodel(m), cdata(d), None, None) == -1
  assert L.mjw_island(cmodel(m), _lib.CData(), ci, None) == 0  # nworld = 0
  bad = _lib.CIsland()
  ctypes.memmove(ctypes.byref(bad), ctypes.byref(ci), ctypes.sizeof(ci))
  bad.ntree = m.ntree + 1
  assert L.mjw_island(cmodel(m), cdata(d), bad, None) not in (0, -1)
  assert b"ntree" in L.mjw_last_error()
  bad.ntree, bad.tree_island = m.ntree, None
  assert L.mjw_island(cmodel(m), cdata(d), bad, None) == -1
  assert b"null" in L.mjw_last_error()


def test_cpu_data_fails_like_inverse_and_no_trees_launch_nothing():
  mjw, mjm, m, d = _small()
  with pytest.raises(RuntimeError, match="ROCm device only"):
    mjw.island(m, d)
  with pytest.raises(RuntimeError, match="ROCm device only"):
    mjw.inverse(m, d)
  mjm0 = mjw.load_model_from_string('<mujoco><worldbody><geom type="plane" size="1 1 .1"/></worldbody></mujoco>')
  m0 = mjw.put_model(mjm0, device="cpu")
  d0 = mjw.make_data(mjm0, nworld=2, device="cpu", m=m0)
  d0.nisland.fill_(3)
  mjw.island(m0, d0)  # ntree == 0: nisland zeroed, nothing launched (a launch would raise on this host Data)
  assert d0.nisland.tolist() == [0, 0] and tuple(d0.tree_island.shape) == (2, 0)


# ---- the yardstick and the scenes agree ----------------------------------------------------------------
def _oracle(mjm, qpos, njmax, nconmax, eq_active=None):
  nw = qpos.shape[0]
  _, od = oracle_from_state(mjm, qpos, np.zeros((nw, mjm.nv)), np.zeros((nw, mjm.nu)), njmax=njmax, nconmax=nconmax)
  if eq_active is not None:
    od.eq_active[:] = eq_active
  od.fwd_position()
  return od


@pytest.mark.parametrize("scene", sc.SCENES, ids=[s.id for s in sc.SCENES])
def test_yardstick_matches_the_hand_written_expectation(scene):
  mjm = scene.model()
  ids = ir.model_ids(mjm)
  assert ids["ntree"] == len(scene.tree_island)
  od = _oracle(mjm, scene.state(mjm, 1), scene.njmax, scene.nconmax)
  n = int(od.nefc[0, 0])
  assert n <= scene.njmax
  types = set(od.efc_type[0, :n].tolist())
  assert set(scene.rows) <= types, (scene.rows, types)  # the scene produces the rows it is there for
  nisland, tree_island, dof_island, efc_island = ir.oracle_world(ids, od, 0)
  assert nisland == scene.nisland and tree_island.tolist() == list(scene.tree_island)
  assert dof_island.tolist() == [scene.tree_island[t] for t in ids["dof_treeid"]]
  assert (efc_island[n:] == -1).all() and (efc_island[:n] >= 0).all() and set(efc_island[:n].tolist()) == set(range(nisland))
  if scene.generic:  # its rows take the Jacobian scan: none of them is a typed row
    for r in range(n):
      t, i = int(od.efc_type[0, r]), int(od.efc_id[0, r])
      assert t in (ir.FRICTION_TENDON, ir.LIMIT_TENDON) or (t == ir.EQUALITY and mjm.eq_type[i] not in (ir.EQ_CONNECT, ir.EQ_WELD))


def test_yardstick_on_the_column_worlds():
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(sc.COLUMN_XML)
  ids = ir.model_ids(mjm)
  od = _oracle(mjm, sc.column_qpos(mjm), 16, 4)
  for w, (_, nisland, tree_island, ncon) in enumerate(sc.COLUMN_WORLDS):
    assert int(od.nefc[w, 0]) == 4 * ncon
    got = ir.oracle_world(ids, od, w)
    assert got[0] == nisland and got[1].tolist() == tree_island


@pytest.mark.parametrize("ntree,bodies,jacobian", [(1, "slide", None), (2, "free", None), (33, "slide", None), (64, "slide", "dense")])
def test_yardstick_on_the_size_edge_worlds(ntree, bodies, jacobian):
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(sc.edge_model_xml(ntree, bodies, jacobian))
  ids = ir.model_ids(mjm)
  act = sc.edge_eq_active(ntree, bodies)
  od = _oracle(mjm, np.tile(mjm.qpos0, (len(act), 1)), sc.edge_njmax(ntree), 1, eq_active=act)
  for w, name in enumerate(sc.edge_worlds(bodies)):
    nisland, tree_island, rows = sc.edge_expected(ntree, name)
    assert int(od.nefc[w, 0]) == rows
    got = ir.oracle_world(ids, od, w)
    assert got[0] == nisland and got[1].tolist() == tree_island


def test_yardstick_on_hand_built_rows():
  """Rows the oracle does not produce: ids outside their arrays contribute nothing, a contact with a flex side
  scans J, a row of three trees joins all three, and the reference's order trap is one island."""
  ids = dict(ntree=4, nv=4, body_treeid=np.array([-1, 0, 1, 2, 3]), dof_treeid=np.arange(4), jnt_dofadr=np.arange(4),
             geom_bodyid=np.array([0, 1, 2]), site_bodyid=np.zeros(0, int), eq_type=np.array([2, 0]), eq_obj1id=np.array([0, 3]),
             eq_obj2id=np.array([1, 9]), eq_objtype=np.array([3, 1]))
  J = np.zeros((8, 4))
  J[0, [1, 2]] = 1.0   # joint equality over trees 1, 2
  J[1, [0, 2]] = -2.0  # then over 0, 2
  J[4, [0, 3]] = 1.0   # a contact with a flex side
  efc_type = np.array([ir.EQUALITY, ir.EQUALITY, ir.FRICTION_DOF, ir.CONTACT_PYRAMIDAL, ir.CONTACT_PYRAMIDAL, ir.EQUALITY, ir.LIMIT_JOINT, 0])
  efc_id = np.array([0, 0, 7, 5, 1, 1, -1, 0])  # dof 7, contact 5, joint -1: outside; equality 1: body 3 and body 9 (outside)
  contact_geom = np.array([[1, 2], [-1, 2]])
  nisland, tree_island, dof_island, efc_island = ir.islands(ids, efc_type, efc_id, J, contact_geom, 7, 8)
  assert nisland == 1 and tree_island.tolist() == [0, 0, 0, 0] and efc_island.tolist() == [0, 0, -1, -1, 0, 0, -1, -1]
  nisland, tree_island, _, efc_island = ir.islands(ids, efc_type, efc_id, J, contact_geom, 2, 8)  # only the trap's two rows
  assert nisland == 1 and tree_island.tolist() == [0, 0, 0, -1] and efc_island.tolist() == [0, 0] + [-1] * 6
  J3 = np.zeros((1, 4))
  J3[0, [0, 1, 3]] = 1.0
  nisland, tree_island, _, _ = ir.islands(ids, np.array([ir.LIMIT_TENDON]), np.array([0]), J3, contact_geom, 1, 1)
  assert nisland == 1 and tree_island.tolist() == [0, 0, -1, 0]
