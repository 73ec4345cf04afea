"""tests/sensor_cases.py on the CPU: every case reaches the edge it exists for, proved on the fp64 oracle alone, a few
closed forms pin the oracle's rne_postconstraint where they are cheap, the checker's own measures behave, and put_model
refuses a sensor model whose LDS layout cannot fit, on the dense path as on the sparse one."""

import numpy as np
import pytest

from tests import sensor_cases as sc


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_case_reaches_its_edge(case):
  mjm = case.model()
  st = case.states(mjm)
  o = sc.reference(case, mjm, st)
  assert case.edge and case.check in sc.PREDICATES
  assert st[0].shape == (sc.NWORLD, mjm.nq) and np.abs(st[1]).min() > 0  # NWORLD seeded random states
  sc.PREDICATES[case.check](case, mjm, st, o)
  if case.rows:
    assert int(o["nefc"].min()) > 0
  # the fp32 oracle, whose error sets the bar, builds the same rows: the fp64 forces written over its own line up
  o32 = sc.oracle_run(case, mjm, st, real_bits="32f", solution=o)
  assert np.array_equal(o32["nefc"], o["nefc"]) and np.array_equal(o32["efc_type"], o["efc_type"]) and np.array_equal(o32["efc_id"], o["efc_id"])
  assert all(sc.strict_units(o32[f], o[f]) < 20 for f in sc.FIELDS)  # fp32 follows fp64: the bar stays a bar
  for f in sc.FIELDS:
    assert np.isfinite(o[f]).all()


def test_case_list_covers_the_issue():
  ids = [c.id for c in sc.CASES]
  assert len(set(ids)) == len(ids)
  for want in ("bodies-2", "bodies-chain-64", "bodies-chain-65", "bodies-chain-66", "bodies-chain-129", "bodies-star-66", "bodies-star-129",
               "bodies-chain-65-generic", "bodies-chain-65-sparse", "sensors-1", "sensors-63", "sensors-64", "sensors-65", "sensors-130",
               "cutoff-on", "cutoff-off", "equality", "rowcut", "batched-2", "batched-3", "flag-nosensor", "flag-nogravity"):
    assert want in ids
  assert {f"contact-{c}-{k}" for c in ("pyramidal", "elliptic") for k in (1, 3, 4, 6)} <= set(ids)
  from mujoco_warp_amd import types

  assert (sc.DSBL_GRAVITY, sc.DSBL_SENSOR) == (int(types.DisableBit.GRAVITY), int(types.DisableBit.SENSOR))
  assert (sc.S_TOUCH, sc.S_ACCELEROMETER, sc.S_FORCE, sc.S_GEOMDIST, sc.S_CLOCK) == tuple(
    int(getattr(types.SensorType, n)) for n in ("TOUCH", "ACCELEROMETER", "FORCE", "GEOMDIST", "CLOCK"))
  assert (sc.EQ_CONNECT, sc.EQ_WELD, sc.EQ_JOINT, sc.EQ_TENDON) == tuple(int(getattr(types.EqType, n)) for n in ("CONNECT", "WELD", "JOINT", "TENDON"))


def test_strict_units_and_bar():
  want = np.array([[1.0, 0.0, -2.0]] * sc.NWORLD)
  assert sc.strict_units(want, want) == 0.0
  got = want.copy()
  got[1, 2] += 2 * (sc.RTOL * 2.0 + sc.FLOOR * 2.0)  # twice the strict bar on that element
  assert abs(sc.strict_units(got, want) - 2.0) < 1e-9
  got = want.copy()
  got[0, 1] = 3 * sc.FLOOR * 2.0  # a zero entry is held by the floor alone
  assert abs(sc.strict_units(got, want) - 3.0) < 1e-9
  assert sc.strict_units(np.full_like(want, np.nan), want) == np.inf
  case = sc.BY_ID["equality"]
  assert sc.bar(case, 0.1) == 1.0 and sc.bar(case, 10.0) == 40.0 and sc.bar(sc.BY_ID["bodies-2"], 0.2) == 1.0


def test_stage_slots_partition_sensordata():
  mjm = sc.BY_ID["sensors-130"].model()
  slots = sc.stage_slots(mjm)
  assert sorted(np.concatenate(list(slots.values())).tolist()) == list(range(mjm.nsensordata))
  assert all(len(v) for v in slots.values())


# ---- closed forms ----------------------------------------------------------------------------------------------------
def test_chain_at_rest_root_force_reads_the_total_weight():
  """The 65-body chain at rest (its 64 links with no joint, so nothing moves): the root's force sensor reads the total
  weight, pointing up, in the site's frame.  On the moving chain the force parts of cfrc_ext are the applied forces."""
  from mujoco_warp_amd.mjcf import quat_to_mat

  still = sc.Case("rigid", "closed form", sc.chain_xml(65, 0), "none")
  rigid = still.model()
  assert (rigid.nbody, rigid.nv) == (65, 0)
  o = sc.oracle_run(still, rigid, still.states(rigid))
  weight = 9.81 * float(np.asarray(rigid.body_mass)[1:].sum())
  k = [i for i in range(rigid.nsensor) if rigid.sensor_type[i] == sc.S_FORCE and rigid.site_bodyid[rigid.sensor_objid[i]] == 1][0]
  f = o["sensordata"][:, int(rigid.sensor_adr[k]) : int(rigid.sensor_adr[k]) + 3]
  R = quat_to_mat(np.asarray(rigid.site_quat)[int(rigid.sensor_objid[k])])  # the bodies are not rotated: the site's world frame
  assert weight > 1.0 and np.allclose(f @ R.T, np.tile([0, 0, weight], (sc.NWORLD, 1)), rtol=1e-12, atol=1e-12 * weight)
  case = sc.BY_ID["bodies-chain-65"]
  mjm = case.model()
  o = sc.oracle_run(case, mjm, case.states(mjm))
  ext = o["cfrc_ext"].reshape(sc.NWORLD, mjm.nbody, 6)[:, :, 3:]
  assert np.allclose(ext, case.xfrc_applied(mjm)[:, :, :3], rtol=1e-12, atol=1e-14)


def test_weld_bodies_see_equal_and_opposite_force():
  """A weld's two bodies take +f and -f (cfrc_ext force part).  Bodies c and d of the equality model carry other
  constraints too, so the test uses two free bodies joined by one weld and nothing else."""
  xml = ('<mujoco><option timestep="0.002"/><worldbody>'
         '<body name="a" pos="0 0 1"><freejoint/><geom type="box" size=".05 .04 .03" contype="0" conaffinity="0" mass=".5"/><site name="sa"/></body>'
         '<body name="b" pos=".3 .1 1"><freejoint/><geom type="box" size=".05 .04 .03" contype="0" conaffinity="0" mass=".8"/><site name="sb"/></body>'
         '</worldbody><equality><weld body1="a" body2="b" torquescale="2.5" anchor=".02 0 .01"/></equality>'
         '<sensor><force site="sa"/><force site="sb"/></sensor></mujoco>')
  case = sc.Case("weld", "closed form", xml, "none", rows=True, seed=5, noise=sc.NEAR)
  mjm = case.model()
  st = case.states(mjm)
  o = sc.oracle_run(case, mjm, st)
  ext = o["cfrc_ext"].reshape(sc.NWORLD, 3, 6)
  assert (o["nefc"] == 6).all() and np.abs(ext[:, 1, 3:]).min() > 1e-3
  assert np.allclose(ext[:, 1, 3:], -ext[:, 2, 3:], rtol=1e-13, atol=0)
  assert np.allclose(ext[:, 1, 3:], o["efc_force"][:, :3], rtol=1e-13)  # body 1 takes +force
  assert not ext[:, 0].any()  # the world body takes nothing


def test_connect_anchor_carries_no_torque():
  """A body hung from the world by one connect: the constraint force acts at the anchor, so cfrc_ext's torque about the
  tree's com is (anchor - com) x f."""
  xml = ('<mujoco><option timestep="0.002"/><worldbody>'
         '<body name="a" pos="0 0 1"><freejoint/><geom type="box" size=".05 .04 .03" contype="0" conaffinity="0" mass=".5"/><site name="sa"/></body>'
         '</worldbody><equality><connect body1="a" anchor=".1 .02 .05"/></equality><sensor><torque site="sa"/></sensor></mujoco>')
  case = sc.Case("connect", "closed form", xml, "none", rows=True, seed=6, noise=sc.NEAR)
  mjm = case.model()
  st = case.states(mjm)
  o = sc.oracle_run(case, mjm, st)
  ext = o["cfrc_ext"].reshape(sc.NWORLD, 2, 6)[:, 1]
  f = o["efc_force"][:, :3]
  xmat = o["xmat"].reshape(sc.NWORLD, 2, 3, 3)[:, 1]
  anchor = o["xpos"].reshape(sc.NWORLD, 2, 3)[:, 1] + np.einsum("wij,j->wi", xmat, [0.1, 0.02, 0.05])
  com = o["subtree_com"].reshape(sc.NWORLD, 2, 3)[:, 1]
  assert np.allclose(ext[:, 3:], f, rtol=1e-13) and np.allclose(ext[:, :3], np.cross(anchor - com, f), rtol=1e-10, atol=1e-13)


# ---- put_model: the sensor kernel's LDS layout -----------------------------------------------------------------------
def _many_bodies_xml(nbody, tactile=False):
  kids = "".join(f'<body pos="{0.01 * (i % 30)} {0.01 * (i // 30)} 0"><geom size=".004"/></body>' for i in range(nbody - 2))
  asset = '<asset><mesh name="pad" vertex="0 0 0 .1 0 0 0 .1 0 0 0 .1" face="0 2 1 0 1 3 0 3 2 1 2 3"/></asset>' if tactile else ""
  pad = '<geom name="fpad" type="mesh" mesh="pad" contype="0" conaffinity="0" mass="0"/>' if tactile else ""
  sens = '<tactile geom="fpad" mesh="pad"/>' if tactile else '<gyro site="s"/>'
  return (f'<mujoco>{asset}<default><geom contype="0" conaffinity="0"/></default><worldbody><body pos="0 0 1"><joint type="hinge"/><geom size=".05"/>'
          f'<site name="s"/>{pad}{kids}</body></worldbody><sensor>{sens}</sensor></mujoco>')


def _layout_words(nbody, nv, tactile):
  """make_slayout (csrc/mjw_sensor.hip), restated: cacc, cfrc_int, cfrc_ext, cvel (6 per body), cinert (10), subtree_com (3),
  cdof, cdof_dot (6 per dof), qvel, qacc, each rounded up to 4 words, and 64 words of tactile partners."""
  r4 = lambda n: -(-n // 4) * 4  # noqa: E731
  return 4 * r4(6 * nbody) + r4(10 * nbody) + r4(3 * nbody) + 2 * r4(6 * nv) + 2 * r4(nv) + 64 * tactile


@pytest.mark.parametrize("tactile", [False, True])
def test_put_model_refuses_a_sensor_model_past_the_lds_layout(tactile):
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf
  from mujoco_warp_amd.io import is_sparse

  fits = 440 if tactile else 442  # the last nbody (nv 1) whose layout is within 16384 words
  assert _layout_words(fits, 1, tactile) <= 16384 < _layout_words(fits + 1, 1, tactile)
  assert _layout_words(fits + 1, 1, False) <= 16384 or not tactile  # the 64 tactile words decide the tactile pair
  ok = mjcf.load_model_from_string(_many_bodies_xml(fits, tactile))
  assert ok.nbody == fits and ok.nv == 1 and not is_sparse(ok)  # the dense path
  m = mjw.put_model(ok, device="cpu")
  assert m.nsensor == 1 and (m.nsensortaxel > 0) == tactile
  over = mjcf.load_model_from_string(_many_bodies_xml(fits + 1, tactile))
  with pytest.raises(NotImplementedError, match=r"16384 words \(64 KB\) of LDS.*nbody %d, nv 1 need %d.*at launch" % (fits + 1, _layout_words(fits + 1, 1, tactile))):
    mjw.put_model(over, device="cpu")
  over.nsensor = 0  # without sensors the kernel never runs: no refusal
  for f in ("type", "datatype", "needstage", "objtype", "objid", "reftype", "refid", "dim", "adr", "cutoff", "noise"):
    setattr(over, "sensor_" + f, getattr(over, "sensor_" + f)[:0])
  over.sensor_intprm = over.sensor_intprm[:0]
  over.nsensordata = 0
  mjw.put_model(over, device="cpu")


def test_put_model_refuses_on_the_sparse_path_too():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf
  from mujoco_warp_amd.io import is_sparse

  xml = _many_bodies_xml(443).replace("<mujoco>", '<mujoco><option jacobian="sparse"/>')
  mjm = mjcf.load_model_from_string(xml)
  assert is_sparse(mjm)
  with pytest.raises(NotImplementedError, match="64 KB"):
    mjw.put_model(mjm, device="cpu")
