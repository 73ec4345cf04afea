"""The island kernel (csrc/mjw_island.hip) on the device.  Every comparison is exact: integers, every world, every
entry of nisland / tree_island / dof_island / efc_island.  Each case is compared with the hand-written expectation
of its scene (tests/island_scenes.py) and with the numpy yardstick (tests/island_ref.py) run on the device's own
row arrays read back; the outputs are pre-filled with -7 so that an entry the kernel skips shows.
"""

import numpy as np
import pytest

from tests import island_ref as ir
from tests import island_scenes as sc
from tests.common import np_

pytestmark = pytest.mark.gpu

OUTPUTS = ("nisland", "tree_island", "dof_island", "efc_island")


def _device(mjm, qpos, njmax, nconmax, eq_active=None, qvel=None, ctrl=None):
  import torch

  import mujoco_warp_amd as mjw

  nworld = qpos.shape[0]
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, njmax=njmax, nconmax=nconmax, device="cuda", m=m)
  d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32, device="cuda")
  if qvel is not None:
    d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32, device="cuda")
  if ctrl is not None:
    d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32, device="cuda")
  if eq_active is not None:
    d.eq_active[:] = torch.as_tensor(eq_active, dtype=torch.int32, device="cuda")
  return m, d


def _island(m, d):
  """Garbage into the outputs, one launch, the outputs back as numpy."""
  import torch

  import mujoco_warp_amd as mjw

  for f in OUTPUTS:
    getattr(d, f).fill_(-7)
  mjw.island(m, d)
  torch.cuda.synchronize()
  return {f: getattr(d, f).cpu().numpy() for f in OUTPUTS}


def _check_against_ref(mjm, m, d, got, label=""):
  """Every world against the yardstick over the device's rows; returns the per-world row counts n."""
  ids = ir.model_ids(mjm)
  assert ids["ntree"] == m.ntree
  contact_geom = d.contact.geom.cpu().numpy()
  ns = []
  for w in range(d.nworld):
    efc_type, efc_id, J, n = ir.device_rows(m, d, w)
    nisland, tree_island, dof_island, efc_island = ir.islands(ids, efc_type, efc_id, J, contact_geom, n, d.njmax)
    assert int(got["nisland"][w]) == nisland, (label, w, int(got["nisland"][w]), nisland)
    np.testing.assert_array_equal(got["tree_island"][w], tree_island, err_msg=f"{label} world {w} tree_island")
    np.testing.assert_array_equal(got["dof_island"][w], dof_island, err_msg=f"{label} world {w} dof_island")
    np.testing.assert_array_equal(got["efc_island"][w], efc_island, err_msg=f"{label} world {w} efc_island")
    assert (got["efc_island"][w, n:] == -1).all()
    ns.append(n)
  return ns


def _check_expected(got, w, nisland, tree_island, dof_treeid):
  assert int(got["nisland"][w]) == nisland, (w, int(got["nisland"][w]), nisland)
  assert got["tree_island"][w].tolist() == list(tree_island), (w, got["tree_island"][w].tolist())
  assert got["dof_island"][w].tolist() == [tree_island[t] for t in dof_treeid]


def _row_types(d, w):
  n = max(0, min(int(d.nefc[w]), d.njmax))
  return d.efc.type[w, :n].cpu().numpy().tolist()


# ---- all scenes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sc.SCENES, ids=[s.id for s in sc.SCENES])
def test_scene(scene):
  import mujoco_warp_amd as mjw

  mjm = scene.model()
  m, d = _device(mjm, scene.state(mjm, 2), scene.njmax, scene.nconmax)
  mjw.fwd_position(m, d)
  got = _island(m, d)
  ids = ir.model_ids(mjm)
  for w in range(2):
    types = _row_types(d, w)
    assert set(scene.rows) <= set(types), (scene.rows, types)  # no vacuous pass: the rows it exists for are there
    _check_expected(got, w, scene.nisland, scene.tree_island, ids["dof_treeid"])
  _check_against_ref(mjm, m, d, got, scene.id)


# ---- per-world divergence, the njmax cut, njmax == 0 --------------------------------------------------------
def _column(njmax):
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(sc.COLUMN_XML)
  m, d = _device(mjm, sc.column_qpos(mjm), njmax, 4)
  mjw.fwd_position(m, d)
  return mjm, m, d


def test_worlds_diverge():
  mjm, m, d = _column(16)
  got = _island(m, d)
  ids = ir.model_ids(mjm)
  for w, (_, nisland, tree_island, ncon) in enumerate(sc.COLUMN_WORLDS):
    assert int(d.nefc[w]) == 4 * ncon and all(t == ir.CONTACT_PYRAMIDAL for t in _row_types(d, w))
    _check_expected(got, w, nisland, tree_island, ids["dof_treeid"])
  assert got["nisland"].tolist() == [0, 1, 1, 2]
  _check_against_ref(mjm, m, d, got)


@pytest.mark.parametrize("njmax", [4, 6])
def test_njmax_cuts_the_last_contact(njmax):
  """World 3 has two contacts of four rows: njmax 4 cuts the second whole, 6 cuts through it."""
  mjm, m, d = _column(njmax)
  assert int(d.nefc[3]) > njmax
  got = _island(m, d)
  ns = _check_against_ref(mjm, m, d, got)  # the yardstick at n = min(nefc, njmax)
  assert ns == [0, 4, 4, njmax]
  for w in range(4):
    assert (got["efc_island"][w, ns[w]:] == -1).all()
  assert got["nisland"][:3].tolist() == [0, 1, 1] and int(got["nisland"][3]) >= 1


def test_njmax_zero():
  """No row storage at all: no row, so no island; no position stage is needed for that."""
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(sc.COLUMN_XML)
  m, d = _device(mjm, sc.column_qpos(mjm), 0, 4)
  got = _island(m, d)
  assert got["nisland"].tolist() == [0] * 4 and (got["tree_island"] == -1).all() and (got["dof_island"] == -1).all()
  assert got["efc_island"].shape == (4, 0)


# ---- disable flags ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["constraint", "contact"])
def test_disable_flag_gives_the_no_row_answer(flag):
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(sc.COLUMN_XML)
  mjm.opt.disableflags = int(mjm.opt.disableflags) | {"constraint": 1, "contact": 16}[flag]
  m, d = _device(mjm, sc.column_qpos(mjm), 16, 4)
  mjw.fwd_position(m, d)
  got = _island(m, d)
  assert d.nefc.tolist() == [0] * 4
  assert got["nisland"].tolist() == [0] * 4
  for f in ("tree_island", "dof_island", "efc_island"):
    assert (got[f] == -1).all(), f
  _check_against_ref(mjm, m, d, got)


# ---- size edges ------------------------------------------------------------------------------------------
def _cap():
  from mujoco_warp_amd.island import ISLAND_LDS_TREES

  return ISLAND_LDS_TREES


# (ntree, bodies, jacobian, path the model must take).  Slide bodies: four worlds, joint equalities (rows that
# scan J) and connects (typed rows), each as a reversed chain and as one pair at the far end.  Free spheres with
# connects: the two typed worlds; six dofs a tree put them on the sparse path from six trees on.  The two models
# around the LDS cap are slide bodies only: the host compiler needs minutes for that many free bodies.
EDGES = ([(n, "slide", None, "dense") for n in (1, 2, 31, 32)] + [(64, "slide", "dense", "dense")]
         + [(n, "slide", None, "sparse") for n in (33, 63, 64, 65, 255, 256, 257)]
         + [(n, "free", None, "dense") for n in (1, 2)] + [(n, "free", None, "sparse") for n in (31, 32, 33, 63, 64, 65, 255, 256, 257)]
         + [("cap", "slide", None, "sparse"), ("cap+1", "slide", None, "sparse")])


@pytest.mark.parametrize("ntree,bodies,jacobian,path", EDGES, ids=[f"{b}-{n}-{p}" for n, b, _, p in EDGES])
def test_size_edge(ntree, bodies, jacobian, path):
  import mujoco_warp_amd as mjw

  ntree = {"cap": _cap(), "cap+1": _cap() + 1}.get(ntree, ntree)
  mjm = mjw.load_model_from_string(sc.edge_model_xml(ntree, bodies, jacobian))
  act = sc.edge_eq_active(ntree, bodies)
  m, d = _device(mjm, np.tile(mjm.qpos0, (len(act), 1)), sc.edge_njmax(ntree), 1, eq_active=act if mjm.neq else None)
  assert m.ntree == ntree and bool(m.is_sparse) == (path == "sparse")
  mjw.fwd_position(m, d)
  got = _island(m, d)
  dof_treeid = ir.tree_ids(mjm)[1]
  for w, name in enumerate(sc.edge_worlds(bodies)):
    nisland, tree_island, rows = sc.edge_expected(ntree, name)
    assert int(d.nefc[w]) == rows
    if rows:  # the world's rows are of the kind it is there for
      eq_ids = d.efc.id[w, :rows].cpu().numpy()
      assert set(_row_types(d, w)) == {ir.EQUALITY}
      assert (np.isin(np.asarray(mjm.eq_type)[eq_ids], (ir.EQ_CONNECT, ir.EQ_WELD)) == name.startswith("typed")).all()
    _check_expected(got, w, nisland, tree_island, dof_treeid)
  if ntree <= 257:  # beyond, the hand-written expectation above is the check (the yardstick's Python loops take too long)
    _check_against_ref(mjm, m, d, got)
  else:
    for w, name in enumerate(sc.edge_worlds(bodies)):
      rows = sc.edge_expected(ntree, name)[2]
      assert (got["efc_island"][w, :rows] == 0).all() and (got["efc_island"][w, rows:] == -1).all()


# ---- benchmark models -------------------------------------------------------------------------------------
def test_humanoid_after_50_steps():
  import torch

  import mujoco_warp_amd as mjw
  from tests.common import humanoid_model, random_states

  mjm = humanoid_model("CG")
  qpos, qvel, ctrl = random_states(mjm, 4, seed=3)
  m, d = _device(mjm, qpos, 64, 24, qvel=qvel, ctrl=ctrl)
  for _ in range(50):
    mjw.step(m, d)
  mjw.fwd_position(m, d)  # the rows of the state the last step left
  torch.cuda.synchronize()
  got = _island(m, d)
  ns = _check_against_ref(mjm, m, d, got, "humanoid")
  assert max(ns) > 0 and all((got["nisland"][w] == 1) == (ns[w] > 0) for w in range(4))  # one tree: one island once any row is active


@pytest.mark.parametrize("name,nworld,steps", [("franka", 16, 0), ("apollo", 4, 0), ("cloth", 2, 5)])
def test_benchmark_model(name, nworld, steps):
  import torch

  import mujoco_warp_amd as mjw
  from tests import parity_models as pm

  mjm, qpos, qvel, ctrl, njmax, nconmax, _ = pm.setup(name)
  m, d = _device(mjm, qpos[:nworld], njmax, nconmax, qvel=qvel[:nworld], ctrl=ctrl[:nworld])
  for _ in range(steps):
    mjw.step(m, d)
  mjw.fwd_position(m, d)
  torch.cuda.synchronize()
  got = _island(m, d)
  ns = _check_against_ref(mjm, m, d, got, name)
  assert max(ns) > 0 and int(got["nisland"].max()) >= 1


# ---- non-interference and graph capture ---------------------------------------------------------------------
COMPARED = ("qpos", "qvel", "act", "qacc", "qacc_warmstart", "act_dot", "time", "energy", "xpos", "xquat", "xmat", "xipos", "ximat", "xanchor",
            "xaxis", "geom_xpos", "geom_xmat", "site_xpos", "site_xmat", "cam_xpos", "cam_xmat", "light_xpos", "light_xdir", "subtree_com", "cdof",
            "cinert", "crb", "qM", "qLD", "actuator_length", "actuator_velocity", "actuator_force", "cvel", "cdof_dot", "qfrc_bias", "qfrc_spring",
            "qfrc_damper", "qfrc_gravcomp", "qfrc_fluid", "qfrc_passive", "qfrc_actuator", "qfrc_smooth", "qacc_smooth", "qfrc_constraint",
            "cacc", "cfrc_int", "cfrc_ext", "sensordata", "ne", "nf", "nl", "nefc", "solver_niter", "flexvert_xpos", "flexedge_length")
COMPARED_EFC = ("J", "pos", "margin", "D", "vel", "aref", "frictionloss", "force", "Ma", "type", "state")


@pytest.mark.parametrize("which", ["humanoid", "flex_ropes"])
def test_island_between_steps_changes_nothing(which):
  import torch

  import mujoco_warp_amd as mjw
  from tests.common import humanoid_model, random_states

  if which == "humanoid":
    mjm = humanoid_model("CG")
    qpos, qvel, ctrl = random_states(mjm, 8, seed=5)
    args = dict(njmax=64, nconmax=24, qvel=qvel, ctrl=ctrl)
  else:
    scene = sc.BY_ID[which]
    mjm = scene.model()
    qpos, args = scene.state(mjm, 3), dict(njmax=scene.njmax, nconmax=scene.nconmax)
  datas = []
  for with_island in (False, True):
    m, d = _device(mjm, qpos, **args)
    mjw.step(m, d)
    if with_island:
      d.nisland.fill_(-7)
      mjw.island(m, d)
    mjw.step(m, d)
    torch.cuda.synchronize()
    datas.append(d)
  a, b = datas
  assert bool((b.nisland >= 0).all()) and int(b.nisland.max()) >= 1  # the launch did run, and found rows
  for f in COMPARED:
    assert torch.equal(getattr(a, f), getattr(b, f)), f
  for f in COMPARED_EFC:
    assert torch.equal(getattr(a.efc, f), getattr(b.efc, f)), "efc." + f


def test_graph_capture_of_step_then_island():
  """One linear capture (no parallel branches), as tests/test_graph.py: step then island captured once and replayed."""
  import torch

  import mujoco_warp_amd as mjw
  from tests.common import humanoid_model, random_states

  mjm = humanoid_model("CG")
  qpos, qvel, ctrl = random_states(mjm, 33, seed=9)
  nstep = 5
  m, d = _device(mjm, qpos, 64, 24, qvel=qvel, ctrl=ctrl)
  mjw.step(m, d)
  mjw.island(m, d)
  torch.cuda.synchronize()
  q0 = np_(d.qpos)
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=s):
    mjw.step(m, d)
    mjw.island(m, d)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(np_(d.qpos), q0)  # capture records, it does not run
  for f in OUTPUTS:
    getattr(d, f).fill_(-7)
  for _ in range(1, nstep):
    g.replay()
  torch.cuda.synchronize()
  m2, d2 = _device(mjm, qpos, 64, 24, qvel=qvel, ctrl=ctrl)
  for _ in range(nstep):
    mjw.step(m2, d2)
    mjw.island(m2, d2)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(np_(d.qpos), np_(d2.qpos))
  assert int(d2.nisland.max()) == 1  # the squatting humanoid stands on the floor: rows, and its one tree an island
  for f in OUTPUTS:
    assert torch.equal(getattr(d, f), getattr(d2, f)), f
