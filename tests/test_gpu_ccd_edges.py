"""The convex collision code (csrc/mjw_ccd.h) on the device at its capacity and degeneracy edges.

Layer A: each family of tests/ccd_cases.py through mjw_kat(0, ...) -- kat_ccd_kernel, one wavefront per case, one launch
per family -- judged by the shared acceptance rule (ccd_cases.classify / verdict: pass against the fp64 oracle at the
project's bars, tie with an fp32 oracle build where fp32 itself cannot hold them, anything else within 1 % and bound by
the depth / separation property).  The poses that fill the face array exactly, and one short of it, have to pass; the
overflowing ones return no contact, as the oracle does.

Layer B: small models through fwd_position on the dense path (ccd_kernel / ccd_hf_kernel) and with opt.jacobian = 1
(sp::ccd_kernel), contact for contact against the fp64 oracle (test_collision_types._match), each run twice from fresh
Data and compared bit for bit:
  primlanes  one body carrying K = 63, 64, 65, 129 cylinders over a plane; only cylinders 0, 63, 64 and K - 1 touch, so the
             pre-pass's lane loop over the primitive pairs (p = lane; p += 64) shows its first and its second pass.
  stale      five boxes over a static box interleaved with plane-cylinder pairs; worlds where every box pair, none, and
             every other one passes the broadphase filter: a rejected pair after an accepted one leaves no contacts.
  itswitch   one box-box pair alone (EPA at 16 iterations) and next to an ellipsoid pair (opt.ccd_iterations).
  hfmix      a heightfield model that also has box-box and mesh-box pairs: ordinary convex pairs in ccd_hf_kernel.
  pairs      an explicit <pair> with its own margin and gap next to geom margins, and a pair that bypasses the filter.
  batched    per-world geom_size, geom_margin, pair_margin and opt.ccd_tolerance at nb = nworld (the device model takes
             them as tensors with a leading world dimension), each world against an oracle model of its row.
  sensors    geom distance / normal / fromto sensors on a separated and a penetrating pose of every pair type (ccd_pair
             with a cutoff, in the sensor stage).
Also: the multi-contact points of the multibox family inside both faces, ccd_support of a mesh alone (stride passes and
the lowest-index tie-break), and the pre-pass's own records after an accepted pair turns rejected on the same Data.
"""
import numpy as np
import pytest

from tests import ccd_cases as cc
from tests.common import gpu_from_state, np_, oracle_from_state
from tests.test_collision_types import _load, _match

pytestmark = pytest.mark.gpu


# ---- Layer A ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.FAMILIES))
def test_gpu_ccd_family(name):
  fam, ref = cc.family(name), cc.references(name)
  got = cc.run_device(name)
  assert np.isfinite(got).all(), "a case wrote no result"
  res = cc.classify(name, got, [ref["o32"], ref["o32f"]])
  print(name, f"n {res['n']} pass {res['passed']:.4f} tie {res['tie']:.4f} (cap {res['tie_cap']}) unmatched {res['un']:.4f} "
        f"(cap {res['un_cap']}) property failures {int((~res['property']).sum())} worst dist err {res['worst_dist']:.2e}")
  fails = cc.verdict(name, res)
  if name == "capacity":
    tr = ref["trace"]
    for i, cid in enumerate(fam.ids):
      if "-overflow-" in cid:  # face array full: no contact, exactly as the oracle
        assert tr[i, cc.T["epa_exit"]] == cc.EXIT["face array full"] and ref["o64"][i, 0] == 0
        if got[i, 0] != 0:
          fails.append(f"{cid}: the oracle overflows the face array and reports no contact, the device reports {got[i, :2]}")
      elif "-full-" in cid or "-full-1-" in cid:  # either side of that exit
        if res["cls"][i] == 2:
          fails.append(f"{cid}: unmatched next to the face array's overflow: device {got[i, :2]} oracle {ref['o64'][i, :2]}")
  assert not fails, fails


def test_gpu_ccd_family_is_deterministic():
  a, b = cc.run_device("capacity"), cc.run_device("capacity")
  assert np.array_equal(a, b)


# ---- Layer B ----------------------------------------------------------------------------------------------------------
TOL = (2e-5, 2e-4, 2e-3)  # distance, position, normal: tests/test_collision_types.py, polytope pairs
TOL_SMOOTH = (2e-5, 2e-3, 5e-2)  # ... pairs with an ellipsoid or a cylinder


def _contacts(d):
  """The contact pool as rows (world, geoms, dist, pos, normal), sorted: the order of the pool is not part of the result."""
  n = min(int(d.nacon[0]), d.naconmax)
  rows = np.concatenate([d.contact.worldid[:n].cpu().numpy().reshape(n, 1).astype(np.float64), d.contact.geom[:n].cpu().numpy().reshape(n, 2).astype(np.float64),
                         np_(d.contact.dist[:n]).reshape(n, 1), np_(d.contact.pos[:n]).reshape(n, 3), np_(d.contact.frame[:n]).reshape(n, 9)], axis=1)
  return rows[np.lexsort(rows.T[::-1])]


def _forward_twice(xml, qpos, sparse, tol, nconmax=64, edit=None):
  """fwd_position on two fresh Data: every world contact for contact against the oracle, the two runs bit for bit."""
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(xml)
  if edit:
    edit(mjm)
  if sparse:
    mjm.opt.jacobian = 1
  nworld = len(qpos)
  zeros = np.zeros((nworld, mjm.nv)), np.zeros((nworld, mjm.nu))
  _, od = oracle_from_state(mjm, qpos, *zeros, njmax=256, nconmax=nconmax)
  od.fwd_position()
  runs = []
  for _ in range(2):
    m, d = gpu_from_state(mjm, qpos, *zeros, njmax=256, nconmax=nconmax)
    assert bool(m.is_sparse) == sparse
    mjw.fwd_position(m, d)
    torch.cuda.synchronize()
    for w in range(nworld):
      _match(mjm, d, od, w, *tol)
    runs.append(_contacts(d))
  assert runs[0].shape == runs[1].shape and np.array_equal(runs[0], runs[1])
  return m, od


def _tilted(qpos0, nworld, deg, axis=(1, 0, 0)):
  qpos = np.tile(qpos0, (nworld, 1))
  for w in range(nworld):
    a = np.deg2rad(deg[w]) / 2
    qpos[w, 3:7] = [np.cos(a), *(np.sin(a) * np.asarray(axis, float))]
  return qpos


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("K", [63, 64, 65, 129])
def test_gpu_primlanes(K, sparse):
  touching = sorted({0, 63, 64, K - 1} & set(range(K)))
  geoms = "".join(f'<geom type="cylinder" size=".02 .02" pos="{0.05 * i:.2f} 0 {-0.005 if i in touching else 0.05}" contype="0" conaffinity="1"/>'
                  for i in range(K))
  xml = f"""<mujoco><worldbody><geom type="plane" size="20 20 .1" contype="1" conaffinity="0"/>
  <body pos="0 0 .02"><freejoint/>{geoms}</body></worldbody></mujoco>"""
  qpos0 = _load(xml).qpos0
  m, od = _forward_twice(xml, _tilted(qpos0, 3, (0.0, 3.0, -6.0)), sparse, TOL_SMOOTH)
  assert m.nxn == K  # every plane-cylinder pair is in the list; the cylinders do not pair with each other
  for w in range(3):
    n = int(od.ncon[w, 0])
    assert n >= len(touching)
    assert {int(g) for g in od.con_geom[w, :2 * n]} == {0} | {1 + i for i in touching}


STALE = """<mujoco><worldbody><geom type="plane" size="20 20 .1"/><geom type="box" size="1 .3 .05" pos=".5 0 .05"/>
<body pos="0 {y} .135"><freejoint/>{geoms}</body></worldbody></mujoco>"""


@pytest.mark.parametrize("sparse", [False, True])
def test_gpu_stale_records(sparse):
  """Box pairs over the static box alternate with plane-cylinder pairs in the pair list; per world every box pair passes
  the broadphase filter (y = -0.2), none does (y = 3), or every other one (y = 0.25: the odd boxes sit 0.4 to the side).  A
  pair the filter rejects, run after an accepted one in the same workspace, has to leave a record of zero contacts."""
  geoms = ""
  for i in range(5):
    geoms += f'<geom type="box" size=".04 .04 .04" pos="{0.25 * i:.2f} {0.4 * (i % 2):.1f} 0" euler="3 2 0"/>'
    geoms += f'<geom type="cylinder" size=".03 .04" pos="{0.25 * i:.2f} -0.6 -0.1" euler="2 0 0"/>'
  xml = STALE.format(y=0, geoms=geoms)
  qpos = np.tile(_load(xml).qpos0, (4, 1))
  qpos[:, 1] = [-0.2, 3.0, 0.25, -0.2]
  _, od = _forward_twice(xml, qpos, sparse, TOL_SMOOTH)
  on_box = [sorted({int(b) for a, b in od.con_geom[w, :2 * int(od.ncon[w, 0])].reshape(-1, 2) if a == 1}) for w in range(4)]
  assert on_box[0] == [2, 4, 6, 8, 10] and on_box[1] == [] and on_box[2] == [2, 6, 10] and on_box[3] == on_box[0], on_box


ITSWITCH = """<mujoco><worldbody><geom type="box" size=".3 .3 .05"/>
<body pos="0 0 .125" euler="20 10 0"><freejoint/><geom type="box" size=".1 .07 .05"/></body>{extra}</worldbody></mujoco>"""


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("mixed", [False, True])
def test_gpu_itswitch(mixed, sparse):
  """The same box-box pair alone (every convex pair is box-box: EPA at 16 iterations) and next to an ellipsoid pair (EPA at
  opt.ccd_iterations)."""
  extra = '<body pos=".1 .1 .16"><freejoint/><geom type="ellipsoid" size=".14 .09 .06" contype="2" conaffinity="2"/></body>' if mixed else ""
  xml = ITSWITCH.format(extra=extra).replace('<geom type="box" size=".3 .3 .05"/>', '<geom type="box" size=".3 .3 .05" contype="3" conaffinity="3"/>')
  mjm = _load(xml)
  rng = np.random.default_rng(3)
  qpos = np.tile(mjm.qpos0, (4, 1))
  q = qpos[:, 3:7] + rng.normal(0, 0.1, (4, 4))
  qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
  m, od = _forward_twice(xml, qpos, sparse, TOL_SMOOTH if mixed else TOL)
  assert m.ccd_epa_iterations == (35 if mixed else 16)
  assert int((od.ncon[:, 0] >= 1).sum()) >= 3


@pytest.mark.parametrize("sparse", [False, True])
def test_gpu_hfmix(sparse):
  """A heightfield model runs every convex pair in ccd_hf_kernel: a box on a static box and a mesh on it next to the
  heightfield, and a box on the heightfield itself."""
  rng = np.random.default_rng(5)
  elev = " ".join(f"{v:.4f}" for v in rng.uniform(0, 1, 42))
  xml = f"""<mujoco><asset><hfield name="h" nrow="6" ncol="7" size=".6 .5 .15 .1" elevation="{elev}"/>
  <mesh name="poly" vertex="0.12 0 0  0 0.1 0  -0.12 0 0  0 -0.1 0  0 0 0.09  0.02 0.01 -0.08"/></asset>
  <worldbody><geom type="hfield" hfield="h" pos=".05 -.03 0" euler="0 0 20"/><geom type="box" size=".4 .4 .05" pos="2 0 .05"/>
  <body pos="1.85 0 .14" euler="15 8 0"><freejoint/><geom type="box" size=".1 .07 .05"/></body>
  <body pos="2.15 .1 .17" euler="0 25 0"><freejoint/><geom type="mesh" mesh="poly"/></body>
  <body pos="0 0 .16" euler="10 20 0"><freejoint/><geom type="box" size=".12 .08 .05"/></body></worldbody></mujoco>"""
  mjm = _load(xml)
  qpos = np.tile(mjm.qpos0, (3, 1))
  qpos[1, 2] += 0.004
  qpos[2, 9] -= 0.004
  m, od = _forward_twice(xml, qpos, sparse, (5e-5, 5e-4, 5e-3))  # the heightfield scenes' bar (tests/test_hfield.py)
  assert m.nhfield == 1
  for w in range(3):
    pairs = {tuple(p) for p in od.con_geom[w, :2 * int(od.ncon[w, 0])].reshape(-1, 2).tolist()}
    assert (1, 2) in pairs and (1, 3) in pairs and (0, 4) in pairs, pairs  # box-box, box-mesh and heightfield-box


@pytest.mark.parametrize("sparse", [False, True])
def test_gpu_explicit_pairs(sparse):
  """An explicit <pair> with its own margin and gap next to geom margins, and a pair of geoms that the contype filter
  would drop, far apart: it bypasses the broadphase filter, runs the narrowphase and finds nothing."""
  xml = """<mujoco><worldbody><geom name="base" type="cylinder" size=".3 .05" margin=".004"/>
  <body pos="0 0 .105" euler="12 5 0"><freejoint/><geom name="a" type="ellipsoid" size=".14 .09 .06" margin=".002"/></body>
  <body pos=".5 0 .118" euler="5 0 0"><freejoint/><geom name="b" type="ellipsoid" size=".1 .08 .06" contype="0" conaffinity="0"/></body>
  <body pos="5 5 1"><freejoint/><geom name="c" type="cylinder" size=".05 .05" contype="0" conaffinity="0"/></body>
  </worldbody><contact><pair geom1="base" geom2="b" margin=".012" gap=".003"/><pair geom1="b" geom2="c"/></contact></mujoco>"""
  mjm = _load(xml)
  qpos = np.tile(mjm.qpos0, (3, 1))
  qpos[1, 2] += 0.003
  qpos[2, 9] += 0.0007  # 8.5 mm: inside the pair's margin - gap of 9 mm, outside any geom margin
  qpos[:, 7] = [0.2, 0.2, 0.15]
  _, od = _forward_twice(xml, qpos, sparse, TOL_SMOOTH)
  for w in range(3):
    pairs = {frozenset(p) for p in od.con_geom[w, :2 * int(od.ncon[w, 0])].reshape(-1, 2).tolist()}
    assert pairs == {frozenset((0, 1)), frozenset((0, 2))}, pairs


def test_gpu_multibox_points_inside_both_faces():
  """The multi-contact points themselves (mjw_kat(2, ...) returns them): for every clipped polygon of 3 .. 8 vertices and
  every strip, each kept point lies inside both boxes' faces, and the first eight floats are those of the plain entry."""
  recs, _ = cc.family("multibox").arrays()
  got = cc.run_device("multibox", points=True)
  assert np.array_equal(got[:, :8], cc.run_device("multibox"))
  assert (got[:, 0] >= 3).sum() > 60  # most poses keep three or four points
  bad = cc.box_points_outside(recs, got)
  assert not bad, [(cc.family("multibox").ids[c], i, got[c, :2]) for c, i in bad[:6]]
  for name in ("aligned",):  # box-box records without multi-contact carry the witness points there
    g = cc.run_device(name, points=True)
    assert np.array_equal(g[:, 8:11], g[:, 2:5]) and np.array_equal(g[:, 20:23], g[:, 5:8])


def test_gpu_mesh_support_tie_break():
  """ccd_support of a mesh on its own: the strided scan's second and later passes (4 .. 250 vertices), and the butterfly's
  tie-break -- on the lattice cube's faces and on duplicated vertex sets the lowest index wins."""
  recs, mv, want, ids = cc.support_cases()
  got = cc._kat(3, recs, np.concatenate([[0], mv.reshape(-1)]), 4)
  assert (want >= 0).sum() > 200
  bad = cc.support_failures(recs, mv, want, ids, got)
  assert not bad, bad[:8]


def test_gpu_stale_record_words():
  """The pre-pass's own records (Data.ccd_out, word 0 = the pair's contact count): on one Data, a world where the box pairs
  are accepted and collide, then the same worlds moved away so that the filter rejects them.  The records of the second
  run are those of a fresh Data given the second state only: no count and no point of the first run is left."""
  import torch

  import mujoco_warp_amd as mjw

  geoms = ""
  for i in range(5):
    geoms += f'<geom type="box" size=".04 .04 .04" pos="{0.25 * i:.2f} {0.4 * (i % 2):.1f} 0" euler="3 2 0"/>'
    geoms += f'<geom type="cylinder" size=".03 .04" pos="{0.25 * i:.2f} -0.6 -0.1" euler="2 0 0"/>'
  mjm = _load(STALE.format(y=0, geoms=geoms))
  for sparse in (False,):  # the dense path's ccd_kernel; the sparse pre-pass keeps its box records elsewhere (test_gpu_stale_records sees its contacts)
    mjm.opt.jacobian = 1 if sparse else 0
    first = np.tile(mjm.qpos0, (3, 1))
    first[:, 1] = -0.2
    second = first.copy()
    second[:, 1] = [3.0, 0.25, -0.2]
    zeros = np.zeros((3, mjm.nv)), np.zeros((3, mjm.nu))
    m, d = gpu_from_state(mjm, first, *zeros, njmax=256, nconmax=64)
    mjw.fwd_position(m, d)
    torch.cuda.synchronize()
    rec1 = np_(d.ccd_out).reshape(3, -1, 32)
    d.qpos[:] = torch.as_tensor(second, dtype=torch.float32, device="cuda")
    mjw.fwd_position(m, d)
    torch.cuda.synchronize()
    rec2 = np_(d.ccd_out).reshape(3, -1, 32)
    _, fresh = gpu_from_state(mjm, second, *zeros, njmax=256, nconmax=64)
    mjw.fwd_position(m, fresh)
    torch.cuda.synchronize()
    rec3 = np_(fresh.ccd_out).reshape(3, -1, 32)
    n1, n2 = (rec1[:, :, 0] > 0).sum(1), (rec2[:, :, 0] > 0).sum(1)
    assert (n1 == n1[0]).all() and n2[0] == n1[0] - 5 and n2[1] == n1[0] - 2 and n2[2] == n1[0], (sparse, n1, n2)
    assert np.array_equal(rec2[:, :, 0], rec3[:, :, 0]), sparse
    for a, b in zip(rec2[rec3[:, :, 0] > 0], rec3[rec3[:, :, 0] > 0]):  # the words a record of nc points defines
      nc = int(b[0])
      assert np.array_equal(a[:4 + 4 * nc], b[:4 + 4 * nc]) and np.array_equal(a[20:20 + 3 * nc], b[20:20 + 3 * nc]), sparse


SENSOR_GEOMS = {2: 'type="sphere" size=".12"', 3: 'type="capsule" size=".08 .12"', 4: 'type="ellipsoid" size=".14 .09 .06"',
                5: 'type="cylinder" size=".1 .08"', 6: 'type="box" size=".1 .07 .05"', 7: 'type="mesh" mesh="poly"'}
SENSOR_PAIRS = [(a, b) for a in range(2, 8) for b in range(a, 8)]


@pytest.mark.parametrize("pair", SENSOR_PAIRS, ids=[f"{cc.NAMES[a]}-{cc.NAMES[b]}" for a, b in SENSOR_PAIRS])
def test_gpu_collision_sensors(pair):
  """Geom distance, normal and fromto sensors (cutoff 10: ccd_pair with a cutoff in the sensor stage) on every pair type,
  one separated and one penetrating world.  Bar: the sensor sweep's (tests/sensor_cases.py) -- 1e-5 |want| + 1e-6
  max |want| per world, or 4 x the fp32 oracle's own error where that is larger.  The fp32 oracle's error is taken over
  both of its builds (plain and fused): on ellipsoids and cylinders GJK stops short of its 1e-6 tolerance in fp32, and
  what is left depends on the rounding of each step -- on these poses the two builds are 0 to 450 strict units from
  fp64 and up to ten times apart from each other, so neither alone says what fp32 can hold.  Polytope pairs stay at
  the strict bar.  Measured, device / larger fp32 build, strict units: polytope pairs 0.01 .. 0.3 / 0.01 .. 0.25; pairs
  with an ellipsoid or a cylinder 8 .. 230 / 9 .. 190."""
  import torch

  import mujoco_warp_amd as mjw

  xml = f"""<mujoco><asset><mesh name="poly" vertex="0.12 0 0  0 0.1 0  -0.12 0 0  0 -0.1 0  0 0 0.14  0.02 0.01 -0.08"/></asset>
  <worldbody><body name="a" euler="20 -35 10"><geom name="a" {SENSOR_GEOMS[pair[0]]}/></body>
  <body name="b" pos=".3 .02 .03" euler="-15 40 70"><freejoint/><geom name="b" {SENSOR_GEOMS[pair[1]]}/></body></worldbody>
  <sensor><distance geom1="a" geom2="b" cutoff="10"/><normal geom1="a" geom2="b" cutoff="10"/><fromto geom1="a" geom2="b" cutoff="10"/>
  <distance geom1="b" geom2="a" cutoff="10"/><fromto geom1="b" geom2="a" cutoff="10"/></sensor></mujoco>"""
  mjm = _load(xml)
  qpos = np.tile(mjm.qpos0, (2, 1))
  qpos[0, 0], qpos[1, 0] = 0.4, 0.13  # separated by centimetres; overlapping by centimetres
  zeros = np.zeros((2, mjm.nv)), np.zeros((2, mjm.nu))
  _, od = oracle_from_state(mjm, qpos, *zeros)
  od.forward()
  want, w32 = np.asarray(od.sensordata, np.float64), []
  for bits in (32, "32f"):
    _, o32 = oracle_from_state(mjm, qpos, *zeros, real_bits=bits)
    o32.forward()
    w32.append(np.asarray(o32.sensordata, np.float64))
  assert want[0, 0] > 0.01 and want[1, 0] < -0.005, want[:, 0]
  runs = []
  for _ in range(2):
    m, d = gpu_from_state(mjm, qpos, *zeros)
    mjw.forward(m, d)
    torch.cuda.synchronize()
    runs.append(np_(d.sensordata))
  assert np.array_equal(runs[0], runs[1])
  strict = 1e-5 * np.abs(want) + 1e-6 * np.abs(want).max(axis=1, keepdims=True)
  dev, ref = (np.abs(runs[0] - want) / strict).max(), max((np.abs(w - want) / strict).max() for w in w32)
  bar = max(1.0, 4 * ref)
  print(pair, f"device {dev:.3g} fp32 oracle builds {ref:.3g} bar {bar:.3g} (units of the strict bar)")
  assert dev <= bar, (dev, bar)


@pytest.mark.parametrize("sparse", [False, True])
def test_gpu_batched_fields(sparse):
  """Per-world geom_size (with geom_rbound / geom_aabb kept consistent), geom_margin, pair_margin and opt.ccd_tolerance at
  nb = nworld, set on the device model as tests/sensor_cases.py does; every world against an oracle model of its row."""
  import copy

  import torch

  import mujoco_warp_amd as mjw

  xml = """<mujoco><worldbody><geom name="base" type="cylinder" size=".3 .05" margin=".004"/>
  <body pos="0 0 .105" euler="12 5 0"><freejoint/><geom name="a" type="ellipsoid" size=".14 .09 .06" margin=".002"/></body>
  <body pos=".2 0 .118" euler="5 0 0"><freejoint/><geom name="b" type="ellipsoid" size=".1 .08 .06" contype="0" conaffinity="0"/></body>
  </worldbody><contact><pair geom1="base" geom2="b" margin=".012" gap=".003"/></contact></mujoco>"""
  mjm = _load(xml)
  if sparse:
    mjm.opt.jacobian = 1
  nworld = 3
  rows = []
  for w in range(nworld):
    mw = copy.deepcopy(mjm)
    s = 1 + 0.03 * w
    mw.geom_size = np.array(mjm.geom_size, float).copy()
    mw.geom_size[1:] *= s
    mw.geom_rbound = np.array(mjm.geom_rbound, float).copy()
    mw.geom_rbound[1:] *= s
    mw.geom_aabb = np.array(mjm.geom_aabb, float).copy()
    mw.geom_aabb[1:] *= s
    mw.geom_margin = np.array(mjm.geom_margin, float) + 0.001 * w
    mw.pair_margin = np.array(mjm.pair_margin, float) + 0.002 * w
    mw.opt.ccd_tolerance = (1e-6, 1e-5, 1e-4)[w]
    rows.append(mw)
  qpos = np.tile(mjm.qpos0, (nworld, 1))
  zeros = np.zeros((1, mjm.nv)), np.zeros((1, mjm.nu))
  ods = []
  for w in range(nworld):
    _, od = oracle_from_state(rows[w], qpos[w:w + 1], *zeros, njmax=64, nconmax=16)
    od.fwd_position()
    ods.append(od)
  assert len({round(float(od.con_dist[0, 0]), 5) for od in ods}) == nworld  # the rows give different answers
  runs = []
  for _ in range(2):
    m, d = gpu_from_state(mjm, qpos, np.zeros((nworld, mjm.nv)), np.zeros((nworld, mjm.nu)), njmax=64, nconmax=16)
    f32 = lambda a: torch.as_tensor(np.stack(a), dtype=torch.float32, device="cuda").contiguous()  # noqa: E731
    for name in ("geom_size", "geom_rbound", "geom_aabb", "geom_margin", "pair_margin"):
      setattr(m, name, f32([np.asarray(getattr(mw, name), float).reshape(np.asarray(getattr(mjm, name)).shape) for mw in rows]))
    m.opt.ccd_tolerance = f32([np.array([mw.opt.ccd_tolerance]) for mw in rows])
    mjw.fwd_position(m, d)
    torch.cuda.synchronize()
    for w in range(nworld):
      nacon = min(int(d.nacon[0]), d.naconmax)
      sel = np.nonzero(d.contact.worldid[:nacon].cpu().numpy() == w)[0]
      od = ods[w]
      n = int(od.ncon[0, 0])
      assert len(sel) == n, (w, len(sel), n)
      gd, gg = np_(d.contact.dist[sel]), d.contact.geom[sel].cpu().numpy()
      for i in range(n):
        j = [k for k in range(n) if sorted(gg[k]) == sorted(od.con_geom[0, 2 * i:2 * i + 2])]
        assert j and abs(gd[j[0]] - od.con_dist[0, i]) <= 2e-5, (w, i, gd, od.con_dist[0, :n])
        assert np.abs(np_(d.contact.pos[sel])[j[0]] - od.con_pos[0, 3 * i:3 * i + 3]).max() <= 2e-3
    runs.append(_contacts(d))
  assert np.array_equal(runs[0], runs[1])
