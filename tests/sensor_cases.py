"""The sensor kernel at every body, sensor, stage and row-source edge: the models, the states, the checker and the case list.

csrc/mjw_sensor.hip runs one 64-lane wave per world.  Its per-body loops stride by 64 (`b = lane; b < nb; b += 64`), its
cacc level pass walks the bodies in chunks of 64, its sensor loops stride by 64 over the sensors, sensor_write clips by
data type, cfrc_ext collects xfrc_applied, the connect / weld rows and the contacts, `stages` selects position / velocity /
acceleration work, and every per-world model field is read through MR(...).  The cases below are the smallest models that
reach each of those edges; every case names the edge it exists for and carries a predicate (`PREDICATES[case.check]`)
that proves on the fp64 oracle alone that the edge is reached (tests/test_sensor_cases.py asserts them).

  bodies-*      contact- and constraint-free trees (qacc = qacc_smooth): nbody 2, 64, 65, 66, 129 as a chain (depth crosses
                body 64: a chunk-1 body sums a chunk-0 parent's cacc, nlevel > 64) and as a star (the root's subtree ends
                past body 64), hinged bodies mixed with dof-less welded ones so that nv <= 32; one chain with nv 40 under
                jacobian="dense" (the generic kernel) and its twin on the sparse path (energy_kinetic walks M_rowadr /
                M_colind).  Sites on the root, on bodies 63 and 64 and on the last body carry accelerometer, force, torque,
                velocimeter, gyro, framelinacc, frameangacc, subtreecom, subtreelinvel, subtreeangmom, framepos / framequat
                with a reference frame; e_potential and e_kinetic; xfrc_applied is non-zero on every body.
  sensors-*     nsensor 1, 63, 64, 65, 130 on one small tree: dims 1 / 2 (camprojection) / 3 / 4 and the three stages
                interleaved, so sensor_adr is irregular and the sensors at index >= 64 are of every stage; a geom
                distance sensor takes the collision instantiation (sensor_coll_kernel) through the stride, and
                sensors-130-plain the plain one.
  cutoff-*      a cutoff below the magnitude reached on a REAL sensor (both signs over the worlds), POSITIVE ones (touch,
                and a joint limit force that the case sets to -3 and +5 by hand before the acceleration stage runs: no
                solver output is negative there, and only a negative value tells "clipped above only" from REAL), an AXIS
                one (framexaxis) and QUATERNION ones (framequat, ballquat); cutoff-off is the twin with every cutoff 0.
  equality      connect and weld with body and with site semantics, the world as first and as second body, a weld
                with torquescale and relpose, an inactive constraint among them, and a joint and a tendon equality
                behind them (the connect / weld scan has to stop there); force, torque and accelerometer on every body.
  contact-*     condim 1, 3, 4, 6 in both cones: a box on the floor (four contacts on one body), a sphere resting on that
                box (both bodies non-world) and a sphere on a two-link arm whose parent carries the sensors (cfrc_int
                holds a subtree); force, torque, touch and two contact sensors (force and torque data).
  rowcut        the contact scene (condim 3, pyramidal) with njmax inside a contact's rows.  The reference decodes a
                cut pyramid with zeros for the rows at or past njmax (support.py:241-265) and the oracle does the same
                (contact_force_local, contact_force_world), so force / torque / contact sensors are defined and compared.
                The touch sensor is left out of this case: the reference sums efc_force[efc_address[i]] with address -1
                for a cut row (sensor.py:2043-2051), an out-of-range read, so its value on a cut contact is undefined.
  batched-*     the equality model with sensor_cutoff, site_pos, site_quat, opt.gravity, opt.magnetic, body_mass (with
                body_subtreemass and body_inertia kept consistent), eq_data and jnt_stiffness given a leading dimension
                of 2 (nworld 3: world 2 reads row 0) and of nworld; every world is compared with an oracle run of its row.
  flag-*        DSBL_SENSOR: sensordata keeps a sentinel; DSBL_GRAVITY: the root cacc is zero.

The device check (`run_case`) takes the kernel out of the solver's shadow: after one forward on both sides (row
counts, types and ids asserted equal) the oracle's qacc and efc_force, rounded to fp32, are written into the Data and
mjw.sensor_acc runs on them; sensordata, cacc, cfrc_int and cfrc_ext are compared after that call.  Then the stages
are run one at a time over a sentinel-filled sensordata.

Bars.  An error is measured in units of the project's strict bar (tests/test_gpu_parity_strict.py: |err| <= 1e-5 |want|
+ 1e-6 max|want| per world and field), worst element.  A case holds that bar (1.0) unless the oracle pair shows that
fp32 cannot: the fp32 oracle (real_bits "32f", same states, its own fp32 kinematics, contacts and rows, then the fp64
oracle's qacc and efc_force written over its own and the acceleration stage run on them -- what the device is given) is
measured against the fp64 oracle on the same case and field, and the device's bar is 4 x that error, never below 1.0;
the factor covers a different summation order.  Measured that way every case with rows but one stays at 1.0 (the
cutoff model's free box rests on the floor: its cfrc_int is what is left of cancelling forces, 4 units in fp32), and
the chains of 64 and more bodies rise above it (bodies several metres from the tree's com: cinert and cacc carry
lever-arm terms that cancel in cfrc_int and in the site-frame sensors; 12 units at 129 bodies).  No bar is derived from a
device result.
tools/sensor_edges.py writes the three numbers per case and field to profiles/sensor_edges.json.
"""
import copy
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

NWORLD = 3
RTOL, FLOOR = 1e-5, 1e-6  # tests/test_gpu_parity_strict.py
NOISE_FACTOR = 4.0
SENTINEL = -7654.25  # exact in fp32, not a value any sensor here takes
FIELDS = ("sensordata", "cacc", "cfrc_int", "cfrc_ext")
DSBL_GRAVITY, DSBL_SENSOR = 1 << 7, 1 << 13  # types.DisableBit
S_TOUCH, S_ACCELEROMETER, S_FORCE, S_GEOMDIST, S_CLOCK = 0, 1, 4, 39, 45  # types.SensorType
AXES = ("1 0 0", "0 1 0", "0 0 1", "1 1 0", "0 1 1")
FREE_DEFAULTS = '<default><geom contype="0" conaffinity="0" density="400"/><joint armature="0.05"/></default>'


def _option(jacobian=None, flags="", cone=None):
  attr = (f' jacobian="{jacobian}"' if jacobian else "") + (f' cone="{cone}"' if cone else "")
  return f'<option timestep="0.002" magnetic="0.1 -0.5 0.3"{attr}>{flags}</option>'


# ---- body-count trees ------------------------------------------------------------------------------------------------
def _link(i, pos, joint, site, inner=""):
  s = f'<site name="s{i}" pos=".02 .01 -.01" euler="20 30 -10"/>' if site else ""
  return f'<body name="b{i}" pos="{pos}">{joint}<geom type="capsule" size=".02" fromto="0 0 0 .06 .01 -.03"/>{s}{inner}</body>'


def _hinge(i):
  return f'<joint name="j{i}" type="hinge" axis="{AXES[i % len(AXES)]}"/>'


def _marks(n):
  """The bodies that carry sensors: the root, 63 and 64 exactly, and the last one."""
  return sorted({1, 63, 64, n} & set(range(1, n + 1)))


def _hinged(n, nv, forced):
  """min(nv, n) of the bodies 1..n: `forced` ones first, the rest spread evenly."""
  forced = sorted(set(forced) & set(range(1, n + 1)))
  spread = [int(x) for x in np.round(np.linspace(1, n, min(nv, n)))]
  rest = [b for b in dict.fromkeys(spread) if b not in forced]
  return set((forced + rest)[: min(nv, n)])


def _tree_sensors(marks):
  out = ""
  for i in marks:
    out += (f'<accelerometer site="s{i}"/><force site="s{i}"/><torque site="s{i}"/><velocimeter site="s{i}"/><gyro site="s{i}"/>'
            f'<framelinacc objtype="body" objname="b{i}"/><frameangacc objtype="site" objname="s{i}"/>'
            f'<subtreecom body="b{i}"/><subtreelinvel body="b{i}"/><subtreeangmom body="b{i}"/>'
            f'<framepos objtype="site" objname="s{i}" reftype="body" refname="b1"/>'
            f'<framequat objtype="body" objname="b{i}" reftype="site" refname="s1"/>')
  return out + "<e_potential/><e_kinetic/>"


def chain_xml(nbody, nv, jacobian=None, flags=""):
  """nbody - 1 nested bodies; min(nv, nbody - 1) of them hinged (1, 63, 64, 65 and the last among them), the others welded."""
  n = nbody - 1
  marks, hinged = _marks(n), _hinged(n, nv, (1, 63, 64, 65, n))
  inner = ""
  for i in range(n, 0, -1):
    inner = _link(i, "0 0 1" if i == 1 else ".06 .01 -.03", _hinge(i) if i in hinged else "", i in marks, inner)
  return f"<mujoco>{_option(jacobian, flags)}{FREE_DEFAULTS}<worldbody>{inner}</worldbody><sensor>{_tree_sensors(marks)}</sensor></mujoco>"


def star_xml(nbody, nv):
  """A root on a ball joint with nbody - 2 children, nv - 3 of them hinged (63, 64 and the last among them): the root's
  subtree is every body.  (Not a free root: a free-floating tree in gravity has cfrc_int near 0 by cancellation, which no
  fp32 evaluation holds at the strict bar.)"""
  n = nbody - 1
  marks, hinged = _marks(n), _hinged(n, nv - 2, (1, 63, 64, n))
  kids = "".join(_link(i, f"{0.07 * (i % 12) - 0.4} {0.07 * (i // 12) - 0.4} .05", _hinge(i) if i in hinged else "", i in marks)
                 for i in range(2, n + 1))
  root = (f'<body name="b1" pos="0 0 1"><joint name="j1" type="ball"/><geom type="box" size=".45 .45 .02"/>'
          f'<site name="s1" pos=".02 .01 -.01" euler="20 30 -10"/>{kids}</body>')
  return f"<mujoco>{_option()}{FREE_DEFAULTS}<worldbody>{root}</worldbody><sensor>{_tree_sensors(marks)}</sensor></mujoco>"


# ---- sensor-count tree -----------------------------------------------------------------------------------------------
# dims 1, 2, 3, 4 and the three stages interleaved; {k} cycles over the three sites / geoms
SENSOR_POOL = (
  '<accelerometer site="s{k}"/>', '<jointvel joint="jh"/>', '<force site="s{k}"/>', '<ballquat joint="jb"/>',
  '<velocimeter site="s{k}"/>', '<actuatorfrc actuator="m0"/>', '<framepos objtype="site" objname="s{k}" reftype="body" refname="r"/>',
  '<torque site="s{k}"/>', '<distance geom1="g{k}" geom2="g{k1}" cutoff="1"/>', '<jointpos joint="jh"/>',
  '<camprojection site="s{k}" camera="cam"/>', '<gyro site="s{k}"/>', '<framequat objtype="site" objname="s{k}"/>',
)


def sensors_xml(nsensor, collision=True):
  pool = [p if collision or "distance" not in p else "<clock/>" for p in SENSOR_POOL]
  sens = "".join(pool[i % len(pool)].format(k=i % 3, k1=(i + 1) % 3) for i in range(nsensor))
  tree = ('<camera name="cam" pos="0 -1.5 .8" euler="90 0 0" fovy="50" resolution="64 48"/>'
          '<body name="r" pos="0 0 .8"><joint name="jr" type="ball"/><geom name="g0" type="box" size=".05 .04 .03"/>'
          '<site name="s0" pos=".02 .01 .03" euler="10 40 -25"/>'
          '<body name="a" pos=".1 0 0"><joint name="jh" type="hinge" axis="0 1 0"/><geom name="g1" type="sphere" size=".03" pos=".05 0 0"/>'
          '<site name="s1" pos=".05 0 .01" euler="-30 5 60"/>'
          '<body name="h" pos=".1 0 0"><joint name="jb" type="ball"/><geom name="g2" type="sphere" size=".02" pos=".04 0 0"/>'
          '<site name="s2" pos=".04 .01 0"/></body></body></body>')
  return (f'<mujoco>{_option()}{FREE_DEFAULTS}<worldbody>{tree}</worldbody><actuator><motor name="m0" joint="jh" gear="2"/></actuator>'
          f"<sensor>{sens}</sensor></mujoco>")


# ---- cutoff ----------------------------------------------------------------------------------------------------------
CUTOFF_XML = (f'<mujoco>{_option()}<default><joint armature="0.05"/></default><worldbody><geom type="plane" size="2 2 .1"/>'
              '<body name="box" pos="0 0 .097"><freejoint/><geom type="box" size=".1 .1 .1" mass="1"/><site name="tb" type="box" size=".12 .12 .12"/></body>'
              '<body name="arm" pos=".6 0 .6"><joint name="jb" type="ball"/><geom type="capsule" size=".02" fromto="0 0 0 .2 0 0" contype="0" conaffinity="0"/>'
              '<site name="sa" pos=".1 0 0" euler="30 20 10"/>'
              '<body pos=".2 0 0"><joint name="jh" type="hinge" axis="0 1 0" range="-11 11" limited="true"/>'
              '<geom type="sphere" size=".03" pos=".05 0 0" contype="0" conaffinity="0"/></body></body>'
              '</worldbody><sensor><jointvel name="real_vel" joint="jh" cutoff=".2"/><jointlimitfrc name="positive_limit" joint="jh" cutoff="1"/><gyro name="real_gyro" site="sa" cutoff=".1"/>'
              '<accelerometer name="real_acc" site="sa" cutoff="3"/><touch name="positive" site="tb" cutoff="2"/>'
              '<framexaxis name="axis" objtype="site" objname="sa" cutoff=".3"/><framequat name="quat_frame" objtype="site" objname="sa" cutoff=".3"/>'
              '<ballquat name="quat_ball" joint="jb" cutoff=".3"/></sensor></mujoco>')
CUTOFF_OFF_XML = re.sub(r' cutoff="[^"]*"', "", CUTOFF_XML)

# ---- equality --------------------------------------------------------------------------------------------------------
_EQ_GEOM = '<geom type="box" size=".05 .04 .03" contype="0" conaffinity="0" mass=".5"/>'
_EQ_BODIES = {  # name: (pos, joint, sites)
  "a": ("0 0 1", "<freejoint/>", '<site name="sa" pos=".15 0 0" euler="10 20 30"/>'),
  "b": (".3 0 1", "<freejoint/>", '<site name="sb" pos="-.15 0 0"/>'),
  "c": (".6 0 1", "<freejoint/>", '<site name="sc" pos="0 .03 .02" euler="-20 5 40"/>'),
  "d": (".3 .3 1", "<freejoint/>", '<site name="sd" pos="-.15 0 0"/>'),
  "e": ("0 .3 1", '<joint name="je" type="ball"/>', '<site name="se" pos=".15 0 0"/><site name="se2" pos="0 .1 0"/>'),
  "f": (".9 0 1.1", '<joint name="jf" type="ball"/>', '<site name="sf" pos="0 .02 -.1" euler="5 5 5"/>'),
}
EQUALITY_XML = (
  f'<mujoco>{_option()}<default><joint armature="0.05"/></default><worldbody><site name="sw" pos="0 .4 1"/>'
  + "".join(f'<body name="{n}" pos="{p}">{j}{_EQ_GEOM}{s}</body>' for n, (p, j, s) in _EQ_BODIES.items())
  + '<body name="h1" pos="0 -.4 1"><joint name="h1" type="hinge" axis="0 1 0" stiffness="2"/>' + _EQ_GEOM
  + '<body name="h2" pos=".1 0 0"><joint name="h2" type="hinge" axis="0 1 0" stiffness=".5"/>' + _EQ_GEOM + "</body></body></worldbody>"
  '<tendon><fixed name="t1"><joint joint="h1" coef="1"/><joint joint="h2" coef=".5"/></fixed></tendon><equality>'
  '<connect name="c_body_a_world" body1="a" anchor=".02 0 .05"/>'
  '<weld name="w_body_c_d" body1="c" body2="d" torquescale="2.5" relpose="-.29 .31 .01 0.9987503 0 0.0499792 0" anchor="0 .02 0"/>'
  '<connect name="c_site_a_b" site1="sa" site2="sb"/>'
  '<connect name="c_inactive" body1="b" anchor="0 0 .1" active="false"/>'
  '<joint name="j_h1_h2" joint1="h1" joint2="h2"/>'
  '<weld name="w_site_d_e" site1="sd" site2="se"/>'
  '<connect name="c_body_world_f" body1="world" body2="f" anchor=".9 0 1"/>'
  '<connect name="c_site_world_e" site1="sw" site2="se2"/>'
  '<weld name="w_body_world_b" body1="world" body2="b"/>'
  '<weld name="w_body_c_world" body1="c" anchor=".01 0 0"/>'
  '<tendon name="t_t1" tendon1="t1"/></equality><sensor>'
  + "".join(f'<force site="s{n}"/><torque site="s{n}"/><accelerometer site="s{n}"/>' for n in _EQ_BODIES)
  + '<magnetometer site="sa"/><e_potential/><gyro site="sc" cutoff=".05"/><framepos objtype="site" objname="sc"/>'
  '<framequat objtype="site" objname="sa"/><jointvel joint="h1" cutoff=".1"/></sensor></mujoco>')
EQ_CONNECT, EQ_WELD, EQ_JOINT, EQ_TENDON = 0, 1, 2, 3  # types.EqType


# ---- contact ---------------------------------------------------------------------------------------------------------
def contact_xml(condim, cone, touch=True):
  t = lambda s: f'<touch site="{s}"/>' if touch else ""  # noqa: E731
  return (
    f'<mujoco>{_option(cone=cone)}<default><geom condim="{condim}" friction="0.8 0.02 0.01"/><joint armature="0.05"/></default><worldbody>'
    '<geom name="floor" type="plane" size="3 3 .1"/>'
    '<body name="base" pos="0 0 .046"><freejoint/><geom name="gb" type="box" size=".15 .15 .05" mass="2"/><site name="sbase" type="box" size=".2 .2 .08"/></body>'
    '<body name="ball" pos=".03 -.02 .143"><freejoint/><geom name="gs" type="sphere" size=".05" mass=".5"/><site name="sball" type="sphere" size=".07"/></body>'
    '<body name="par" pos=".8 0 .4"><joint name="jp" type="hinge" axis="0 1 0"/><geom type="capsule" size=".02" fromto="0 0 0 .2 0 0" contype="0" conaffinity="0"/>'
    '<site name="spar" pos=".05 0 0" euler="0 30 0"/>'
    '<body name="kid" pos=".2 0 0"><joint name="jk" type="hinge" axis="0 1 0"/><geom type="capsule" size=".015" fromto="0 0 0 0 0 -.3" contype="0" conaffinity="0"/>'
    '<geom name="gk" type="sphere" size=".05" pos="0 0 -.354"/><site name="skid" type="sphere" size=".07" pos="0 0 -.354"/></body></body>'
    "</worldbody><sensor>"
    + "".join(f'<force site="{s}"/><torque site="{s}"/>{t(s)}' for s in ("sbase", "sball", "spar", "skid"))
    + '<contact body1="base" num="5" data="found force torque"/><contact subtree1="par" data="found force torque pos" reduce="netforce"/>'
    '<accelerometer site="sbase"/></sensor></mujoco>')


# ---- states ----------------------------------------------------------------------------------------------------------
def states(mjm, seed, pos=0.1, quat=None, angle=0.05, slide=0.4, vel=0.5):
  """Seeded random qpos / qvel / ctrl about qpos0.  quat None: random unit quaternions; else a perturbation of that size."""
  rng = np.random.default_rng(seed)
  qpos = np.tile(np.asarray(mjm.qpos0, np.float64), (NWORLD, 1))

  def rot(a):
    if quat is None:
      q = rng.normal(size=(NWORLD, 4))
    else:
      q = qpos[:, a : a + 4] + rng.normal(0, quat, (NWORLD, 4))
    qpos[:, a : a + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)

  for j in range(mjm.njnt):
    a, t = int(mjm.jnt_qposadr[j]), int(mjm.jnt_type[j])
    if t == 0:
      qpos[:, a : a + 3] += rng.normal(0, pos, (NWORLD, 3))
      rot(a + 3)
    elif t == 1:
      rot(a)
    else:
      qpos[:, a] += rng.normal(0, slide if t == 2 else angle, NWORLD)
  return qpos, rng.normal(0, vel, (NWORLD, mjm.nv)), rng.uniform(-1, 1, (NWORLD, mjm.nu))


class Case:
  def __init__(self, id, edge, xml, check, bodies=None, rows=False, njmax=64, nconmax=16, seed=0, noise=None, twin=None, batch=0,
               xfrc=False, expect=None, flag=0):
    self.id, self.edge, self.xml, self.check, self.rows = id, edge, xml, check, rows
    self.njmax, self.nconmax, self.seed, self.noise = njmax, nconmax, seed, noise or {}
    self.twin, self.batch, self.xfrc, self.expect, self.flag = twin, batch, xfrc, expect or {}, flag

  def model(self, xml=None):
    from mujoco_warp_amd import mjcf

    return mjcf.load_model_from_string(xml or self.xml)

  def states(self, mjm):
    qpos, qvel, ctrl = states(mjm, self.seed, **self.noise)
    if self.id.startswith("cutoff"):  # the REAL sensors take both signs over the worlds, well past their cutoffs
      dof = int(mjm.jnt_dofadr[mjm.jnt_names.index("jh")])
      qpos[:, int(mjm.jnt_qposadr[mjm.jnt_names.index("jh")])] = [0.3, 0.28, 0.32]  # past the hinge's upper limit (11 degrees)
      qvel[:, dof] = [0.5, -0.6, 0.4]
      qvel[:, dof - 3 : dof] = [[0.4, -0.5, 0.3], [-0.6, 0.2, 0.5], [0.3, 0.4, -0.7]]
    return qpos, qvel, ctrl

  def synthetic(self, mjm, o):
    """A solution to evaluate the acceleration stage on in place of the solver's, or None.  The cutoff cases give the
    hinge's limit row a force of -3 in world 0 and +5 in world 1: a POSITIVE sensor is clipped above only, which no
    solver output shows (its limit and contact forces are never negative)."""
    if not self.id.startswith("cutoff"):
      return None
    syn = dict(qacc=o["qacc"].copy(), efc_force=o["efc_force"].copy())
    for w, f in ((0, -3.0), (1, 5.0)):
      rows = np.nonzero(o["efc_type"][w, : int(o["nefc"][w, 0])] == 3)[0]  # ConstraintType.LIMIT_JOINT
      assert len(rows) == 1
      syn["efc_force"][w, rows[0]] = f
    return syn

  def xfrc_applied(self, mjm):
    x = np.zeros((NWORLD, mjm.nbody, 6))
    if self.xfrc:
      x[:, 1:] = np.random.default_rng(self.seed + 1000).normal(0, 0.05, (NWORLD, mjm.nbody - 1, 6))
    return x


TOUCHING = dict(pos=0.0004, quat=0.001, angle=0.002, vel=0.2)  # qpos0 holds the penetrations; the noise keeps every contact
NEAR = dict(pos=0.01, quat=0.02, angle=0.05, vel=0.3)  # equality constraints: a small violation in every row


def _cases():
  c = []
  tree = dict(check="tree", xfrc=True, noise=dict(vel=0.3, angle=0.1))  # moderate accelerations: the lever-arm terms stay small
  c.append(Case("bodies-2", "a single moving body: lane 1 only", chain_xml(2, 1), expect=dict(nbody=2, nv=1), **tree))
  for nb in (64, 65, 66, 129):
    c.append(Case(f"bodies-chain-{nb}", f"chain of depth {nb - 1}: " + ("the last body of chunk 0" if nb == 64 else "a chunk-1 body under a chunk-0 parent, nlevel > 64"),
                  chain_xml(nb, 30), expect=dict(nbody=nb, nv=30, sparse=False), seed=nb, **tree))
  for nb in (65, 66, 129):
    c.append(Case(f"bodies-star-{nb}", "star: the root's subtree sum and one level pass cross body 64", star_xml(nb, 30),
                  expect=dict(nbody=nb, nv=30, sparse=False), seed=nb + 1, **tree))
  c.append(Case("bodies-chain-65-generic", "nv 40, dense Jacobian: the generic kernel's Data feeds the sensor kernel", chain_xml(65, 40, "dense"),
                expect=dict(nbody=65, nv=40, sparse=False), seed=7, **tree))
  c.append(Case("bodies-chain-65-sparse", "nv 40 on the sparse path: energy_kinetic over M_rowadr / M_colind", chain_xml(65, 40, "sparse"),
                expect=dict(nbody=65, nv=40, sparse=True), seed=7, **tree))
  for n in (1, 63, 64, 65, 130):
    c.append(Case(f"sensors-{n}", f"nsensor {n}: the sensor lane stride, irregular sensor_adr", sensors_xml(n), "sensors",
                  expect=dict(nsensor=n, coll=n > 8), seed=20 + n, noise=dict(pos=0.05, angle=0.3)))
  c.append(Case("sensors-130-plain", "nsensor 130 without a collision sensor: the plain instantiation past lane 63", sensors_xml(130, False), "sensors",
                expect=dict(nsensor=130, coll=False), seed=150, noise=dict(pos=0.05, angle=0.3)))
  c.append(Case("cutoff-on", "cutoffs that bite on REAL / POSITIVE and must not on AXIS / QUATERNION", CUTOFF_XML, "cutoff", rows=True,
                twin=CUTOFF_OFF_XML, seed=31, noise=dict(TOUCHING, quat=None)))
  c.append(Case("cutoff-off", "the same model, cutoff 0", CUTOFF_OFF_XML, "none", rows=True, seed=31, noise=dict(TOUCHING, quat=None)))
  c.append(Case("equality", "connect / weld rows into cfrc_ext: semantics, anchors, signs, world bodies, the scan's stop", EQUALITY_XML, "equality",
                rows=True, seed=41, noise=NEAR))
  for cone in ("pyramidal", "elliptic"):
    for condim in (1, 3, 4, 6):
      c.append(Case(f"contact-{cone}-{condim}", f"contact rows into cfrc_ext, touch and the contact sensor: condim {condim}, {cone} cone",
                    contact_xml(condim, cone), "contact", rows=True, njmax=96, seed=50 + condim, noise=TOUCHING, expect=dict(condim=condim, cone=cone)))
  c.append(Case("rowcut", "njmax inside a pyramidal contact's rows", contact_xml(3, "pyramidal", touch=False), "rowcut", rows=True, njmax=14,
                seed=53, noise=TOUCHING))
  c.append(Case("batched-2", "per-world model fields, leading dimension 2: world 2 reads row 0", EQUALITY_XML, "batched", rows=True, seed=41,
                noise=NEAR, batch=2))
  c.append(Case(f"batched-{NWORLD}", "per-world model fields, leading dimension nworld", EQUALITY_XML, "batched", rows=True, seed=41, noise=NEAR,
                batch=NWORLD))
  c.append(Case("flag-nosensor", "DSBL_SENSOR: no launch, sensordata untouched", chain_xml(5, 4, flags='<flag sensor="disable"/>'), "nosensor",
                flag=DSBL_SENSOR, seed=61, xfrc=True))
  c.append(Case("flag-nogravity", "DSBL_GRAVITY: the root cacc is zero", chain_xml(5, 4, flags='<flag gravity="disable"/>'), "nogravity",
                twin=chain_xml(5, 4), flag=DSBL_GRAVITY, seed=62, xfrc=True))
  return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ---- batched model fields ----------------------------------------------------------------------------------------------
BATCHED = ("sensor_cutoff", "site_pos", "site_quat", "opt.gravity", "opt.magnetic", "body_mass", "body_subtreemass", "body_inertia", "eq_data",
           "jnt_stiffness")


def _get(mjm, name):
  return getattr(mjm.opt, name[4:]) if name.startswith("opt.") else getattr(mjm, name)


def batched_rows(mjm, nrow, seed):
  """nrow host models that differ in every BATCHED field; masses, subtree masses and inertias stay consistent."""
  rng = np.random.default_rng(seed + 500)
  rows = []
  for r in range(nrow):
    mw = copy.deepcopy(mjm)
    mw.sensor_cutoff = np.asarray(mjm.sensor_cutoff, np.float64) * (1.0 + 0.5 * r)
    mw.site_pos = np.asarray(mjm.site_pos, np.float64) + rng.normal(0, 0.004, np.shape(mjm.site_pos))
    q = np.asarray(mjm.site_quat, np.float64) + rng.normal(0, 0.05, np.shape(mjm.site_quat))
    mw.site_quat = q / np.linalg.norm(q, axis=1, keepdims=True)
    mw.opt.gravity = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), -9.81 * rng.uniform(0.6, 1.4)])
    mw.opt.magnetic = rng.normal(0, 0.4, 3)
    f = np.concatenate([[1.0], rng.uniform(0.7, 1.3, mjm.nbody - 1)])
    mw.body_mass = np.asarray(mjm.body_mass, np.float64) * f
    mw.body_inertia = np.asarray(mjm.body_inertia, np.float64) * f[:, None]
    sub = mw.body_mass.copy()
    for b in range(mjm.nbody - 1, 0, -1):
      sub[int(mjm.body_parentid[b])] += sub[b]
    mw.body_subtreemass = sub
    data = np.array(mjm.eq_data, np.float64)
    body_sem = np.isin(mjm.eq_type, (EQ_CONNECT, EQ_WELD)) & (np.asarray(mjm.eq_objtype) == 1)
    data[body_sem, 0:3] += rng.normal(0, 0.004, (int(body_sem.sum()), 3))
    data[np.asarray(mjm.eq_type) == EQ_WELD, 10] *= 1.0 + 0.3 * (r + 1)
    mw.eq_data = data
    mw.jnt_stiffness = np.asarray(mjm.jnt_stiffness, np.float64) * (1.0 + r)
    rows.append(mw)
  return rows


def apply_batched(m, rows):
  """The rows' BATCHED fields, stacked, as the device model's tensors."""
  import torch

  for name in BATCHED:
    t = torch.as_tensor(np.stack([np.asarray(_get(mw, name), np.float64) for mw in rows]), dtype=torch.float32, device=m.opt.gravity.device)
    if name.startswith("opt."):
      setattr(m.opt, name[4:], t.contiguous())
    else:
      setattr(m, name, t.contiguous())


# ---- oracle ------------------------------------------------------------------------------------------------------------
def oracle_run(case, mjm, st, real_bits=64, solution=None):
  """One oracle forward of the case.  With `solution` (the fp64 run's output) its qacc and efc_force are then written over
  this run's and the acceleration stage is evaluated again on them: with real_bits "32f" that is the fp32 view of what
  the device is given.  Batched cases run one single-world oracle per world, on its row."""
  from oracle import orc

  qpos, qvel, ctrl = st
  xfrc = case.xfrc_applied(mjm)
  models = [mjm] * NWORLD
  if case.batch:
    rows = batched_rows(mjm, case.batch, case.seed)
    models = [rows[w % case.batch] for w in range(NWORLD)]
  groups = [list(range(NWORLD))] if not case.batch else [[w] for w in range(NWORLD)]
  out = {}
  for g in groups:
    om = orc.OracleModel(models[g[0]], real_bits=real_bits)
    od = orc.OracleData(om, len(g), case.njmax, max(case.nconmax, 16))
    od.qpos[:], od.qvel[:], od.ctrl[:] = qpos[g], qvel[g], ctrl[g]
    od.xfrc_applied[:] = xfrc[g].reshape(len(g), -1)
    od.forward()
    if solution is not None:
      od.qacc[:], od.efc_force[:] = solution["qacc"][g], solution["efc_force"][g]
      od.sensor_acc()
    for k, a in od.arrays.items():
      out.setdefault(k, []).append(np.array(a, np.float64 if a.dtype.kind == "f" else a.dtype))
  return {k: np.concatenate(v, axis=0) for k, v in out.items()}


def reference(case, mjm, st):
  """The fp64 oracle's view of the case: one forward, evaluated again on the case's synthetic solution if it has one."""
  o = oracle_run(case, mjm, st)
  syn = case.synthetic(mjm, o)
  return o if syn is None else oracle_run(case, mjm, st, solution=syn)


def strict_units(got, want):
  """The worst |got - want| over the elements in units of the strict bar (rtol |want| + floor max|want| per world)."""
  got = np.asarray(got, np.float64).reshape(NWORLD, -1)
  want = np.asarray(want, np.float64).reshape(NWORLD, -1)
  if want.size == 0:
    return 0.0
  tol = RTOL * np.abs(want) + FLOOR * np.abs(want).max(axis=1, keepdims=True)
  err = np.abs(got - want)
  with np.errstate(divide="ignore", invalid="ignore"):
    u = np.where(err == 0, 0.0, err / tol)
  return float(np.nan_to_num(u, nan=np.inf).max())


def bar(case, noise):
  """The device's bar in strict units: max(1, 4 x the fp32 oracle's error)."""
  return max(1.0, NOISE_FACTOR * noise)


def stage_slots(mjm):
  """Per stage (1 position, 2 velocity, 3 acceleration) the sensordata slots of its sensors."""
  out = {}
  for st in (1, 2, 3):
    idx = [np.arange(a, a + n) for a, n, s in zip(mjm.sensor_adr, mjm.sensor_dim, mjm.sensor_needstage) if s == st]
    out[st] = np.concatenate(idx).astype(int) if idx else np.zeros(0, int)
  return out


def contact_rows(o, w, njmax):
  """(row, contact, rows of that contact) for the contacts of world w with a first row inside njmax."""
  ncon = int(o["ncon"][w, 0])
  adr = o["con_efc_address"][w].reshape(-1, 10)[:ncon]
  return [(int(adr[c, 0]), c) for c in range(ncon) if 0 <= adr[c, 0] < njmax]


# ---- predicates: the edge is reached, on the fp64 oracle alone -----------------------------------------------------------
def _sens(mjm, o, name):
  k = mjm.sensor_names.index(name)
  a, n = int(mjm.sensor_adr[k]), int(mjm.sensor_dim[k])
  return o["sensordata"][:, a : a + n], float(mjm.sensor_cutoff[k])


def check_tree(case, mjm, st, o):
  from mujoco_warp_amd.io import is_sparse

  e = case.expect
  assert (mjm.nbody, mjm.nv) == (e["nbody"], e["nv"])
  if "sparse" in e:
    assert bool(is_sparse(mjm)) == e["sparse"]
  assert int(o["nefc"].max()) == 0 and np.abs(o["qacc"] - o["qacc_smooth"]).max() <= 1e-9 * np.abs(o["qacc"]).max()
  par = np.asarray(mjm.body_parentid)
  nb = mjm.nbody
  bodies = sorted({int(mjm.site_bodyid[i]) for t, i in zip(mjm.sensor_type, mjm.sensor_objid) if t == S_ACCELEROMETER})
  assert 1 in bodies and nb - 1 in bodies
  if nb > 64:
    assert any(b >= 64 and par[b] < 64 for b in range(1, nb)), "no chunk-1 body under a chunk-0 parent"
    assert 63 in bodies and 64 in bodies
    level = np.zeros(nb, int)
    for b in range(1, nb):
      level[b] = level[par[b]] + 1
    if "chain" in case.id:
      assert level.max() + 1 > 64
      assert level[64] == 64 and np.abs(o["cacc"].reshape(NWORLD, nb, 6)[:, 64] - o["cacc"].reshape(NWORLD, nb, 6)[:, 0]).max() > 1e-3
    else:
      assert level.max() == 2 and all(par[b] == 1 for b in range(2, nb))  # the root's subtree is every body
  x = case.xfrc_applied(mjm)
  assert np.abs(x[:, 1]).min() > 0 and np.abs(x[:, nb - 1]).min() > 0
  assert np.abs(o["cfrc_ext"].reshape(NWORLD, nb, 6)[:, nb - 1]).max() > 0
  assert np.abs(o["sensordata"]).min(axis=0).max() > 0


def check_sensors(case, mjm, st, o):
  e = case.expect
  assert mjm.nsensor == e["nsensor"]
  assert bool((np.asarray(mjm.sensor_type) == S_GEOMDIST).any()) == e["coll"]  # the collision instantiation
  assert int(o["nefc"].max()) == 0
  if mjm.nsensor >= 13:
    assert set(np.asarray(mjm.sensor_dim)) == {1, 2, 3, 4} and set(np.asarray(mjm.sensor_needstage)) == {1, 2, 3}
    assert len(set(np.diff(mjm.sensor_adr))) == 4  # irregular addresses
  if mjm.nsensor >= 130:
    assert set(np.asarray(mjm.sensor_needstage)[64:]) == {1, 2, 3} and set(np.asarray(mjm.sensor_dim)[64:]) == {1, 2, 3, 4}
  # every sensor writes something: no slot is zero in all worlds (clock aside, time 0)
  live = np.abs(o["sensordata"]).max(axis=0) > 0
  clock = np.concatenate([[a] for a, t in zip(mjm.sensor_adr, mjm.sensor_type) if t == S_CLOCK] or [np.zeros(0, int)]).astype(int)
  assert live[np.setdiff1d(np.arange(mjm.nsensordata), clock)].all()


def check_cutoff(case, mjm, st, o):
  twin = case.model(case.twin)
  assert np.all(np.asarray(twin.sensor_cutoff) == 0) and np.all(np.asarray(mjm.sensor_cutoff) > 0)
  t = reference(case, twin, st)
  assert int(o["nefc"].min()) > 0
  for name in ("real_vel", "real_gyro", "real_acc"):
    free, _ = _sens(twin, t, name)
    cut, c = _sens(mjm, o, name)
    assert (free > c).any() and (free < -c).any(), name  # both signs exceed the cutoff
    assert np.array_equal(cut, np.clip(free, -c, c)), name
  free, _ = _sens(twin, t, "positive")
  cut, c = _sens(mjm, o, "positive")
  assert (free > c).all() and np.array_equal(cut, np.minimum(free, c))
  free, _ = _sens(twin, t, "positive_limit")
  cut, c = _sens(mjm, o, "positive_limit")
  assert free[0, 0] == -3.0 < -c and free[1, 0] == 5.0 > c and free[2, 0] > 0  # the synthetic limit forces
  assert cut[0, 0] == -3.0 and cut[1, 0] == c  # clipped above only
  for name in ("axis", "quat_frame", "quat_ball"):
    free, _ = _sens(twin, t, name)
    cut, c = _sens(mjm, o, name)
    assert (np.abs(free) > c).any(axis=1).all() and np.array_equal(cut, free), name  # never clipped


def check_equality(case, mjm, st, o):
  names = list(mjm.eq_names)
  want = [n for n in names if n.startswith("c_") and n != "c_inactive"] + [n for n in names if n.startswith("w_")] + ["j_h1_h2", "t_t1"]
  assert not mjm.eq_active0[names.index("c_inactive")] and names.index("c_inactive") < names.index("j_h1_h2") < names.index("w_site_d_e")
  width = {EQ_CONNECT: 3, EQ_WELD: 6, EQ_JOINT: 1, EQ_TENDON: 1}
  ids = sum(([names.index(n)] * width[int(mjm.eq_type[names.index(n)])] for n in want), [])
  for w in range(NWORLD):
    assert int(o["ne"][w, 0]) == int(o["nefc"][w, 0]) == len(ids) == 4 * 3 + 4 * 6 + 2
    assert o["efc_id"][w, : len(ids)].tolist() == ids  # connects, welds, then the joint and the tendon row
    assert np.abs(o["efc_force"][w, : len(ids)]).min() > 0
  sem = {n: (int(mjm.eq_objtype[i]), int(mjm.eq_obj1id[i]), int(mjm.eq_obj2id[i])) for i, n in enumerate(names)}
  assert sem["c_body_a_world"][0] == 1 and sem["c_body_a_world"][2] == 0 and sem["c_body_world_f"][1] == 0
  assert sem["w_body_world_b"][1] == 0 and sem["w_body_c_world"][2] == 0 and sem["c_site_a_b"][0] == 6 and sem["w_site_d_e"][0] == 6
  assert mjm.site_bodyid[sem["c_site_world_e"][1]] == 0
  i = names.index("w_body_c_d")
  assert mjm.eq_data[i, 10] == 2.5 and abs(mjm.eq_data[i, 6] - 0.9987503) < 1e-6


def check_contact(case, mjm, st, o):
  e = case.expect
  body = np.asarray(mjm.geom_bodyid)
  base, par, kid = (mjm.body_names.index(n) for n in ("base", "par", "kid"))
  assert int(mjm.body_parentid[kid]) == par
  rows = {"pyramidal": {1: 1, 3: 4, 4: 6, 6: 10}, "elliptic": {1: 1, 3: 3, 4: 4, 6: 6}}[e["cone"]][e["condim"]]
  types = {"pyramidal": 6, "elliptic": 7}[e["cone"]] if e["condim"] > 1 else 5
  for w in range(NWORLD):
    ncon = int(o["ncon"][w, 0])
    g = body[o["con_geom"][w].reshape(-1, 2)[:ncon]]
    assert ncon == 6 and (o["con_dim"][w, :ncon] == e["condim"]).all()
    assert ((g[:, 0] != 0) & (g[:, 1] != 0)).sum() == 1  # the sphere on the box
    assert (g == base).any(axis=1).sum() == 5  # four floor corners and the sphere
    assert (g == kid).any(axis=1).sum() == 1 and not (g == par).any()
    assert int(o["nefc"][w, 0]) == 6 * rows <= case.njmax and (o["efc_type"][w, : 6 * rows] == types).all()
    assert len(contact_rows(o, w, case.njmax)) == 6
  assert np.abs(_sensor_of(mjm, o, S_FORCE, "spar")).max() > 1e-3  # the parent's force sensor carries the subtree's contact


def _sensor_of(mjm, o, stype, site):
  k = [i for i in range(mjm.nsensor) if mjm.sensor_type[i] == stype and mjm.sensor_objid[i] == mjm.site_names.index(site)][0]
  return o["sensordata"][:, int(mjm.sensor_adr[k]) : int(mjm.sensor_adr[k]) + int(mjm.sensor_dim[k])]


def check_rowcut(case, mjm, st, o):
  full = copy.copy(case)
  full.njmax = 96
  t = oracle_run(full, mjm, st)
  assert not (np.asarray(mjm.sensor_type) == S_TOUCH).any()  # no touch sensor: undefined on a cut contact in the reference
  for w in range(NWORLD):
    assert int(t["nefc"][w, 0]) == 24 > case.njmax
    first = sorted(r for r, _ in contact_rows(t, w, 96))
    assert first == [0, 4, 8, 12, 16, 20] and any(r < case.njmax < r + 4 for r in first)  # the cut falls inside a contact
    kept = contact_rows(o, w, case.njmax)
    assert sorted(r for r, _ in kept) == [0, 4, 8, 12]


def check_batched(case, mjm, st, o):
  rows = batched_rows(mjm, case.batch, case.seed)
  for name in BATCHED:
    a = [np.asarray(_get(mw, name), np.float64) for mw in rows]
    assert all(np.abs(a[0] - x).max() > 0 for x in a[1:]), name  # the rows differ in every batched field
  for mw in rows:
    sub = np.asarray(mw.body_mass, np.float64).copy()
    for b in range(mjm.nbody - 1, 0, -1):
      sub[int(mjm.body_parentid[b])] += sub[b]
    assert np.allclose(sub, mw.body_subtreemass, rtol=1e-14)
    assert np.allclose(np.asarray(mw.body_inertia)[1:] / np.asarray(mjm.body_inertia)[1:], (np.asarray(mw.body_mass)[1:] / np.asarray(mjm.body_mass)[1:])[:, None])
  # the same state evaluated on two rows gives different sensors: each field reaches an output
  if case.batch < NWORLD:
    assert NWORLD % case.batch != 0 or NWORLD > case.batch  # some world wraps
  plain = oracle_run(BY_ID["equality"], mjm, st)
  assert np.abs(plain["sensordata"] - o["sensordata"]).max(axis=1).min() > 1e-3


def check_nosensor(case, mjm, st, o):
  assert mjm.opt.disableflags & DSBL_SENSOR and mjm.nsensor > 0
  assert not o["sensordata"].any()  # the oracle clears sensordata and evaluates nothing


def check_nogravity(case, mjm, st, o):
  assert mjm.opt.disableflags & DSBL_GRAVITY
  t = oracle_run(case, case.model(case.twin), st)
  nb = mjm.nbody
  assert not o["cacc"].reshape(NWORLD, nb, 6)[:, 0].any()
  assert np.allclose(t["cacc"].reshape(NWORLD, nb, 6)[:, 0, 3:], -np.asarray(mjm.opt.gravity))
  acc = [i for i in range(mjm.nsensor) if mjm.sensor_type[i] == S_ACCELEROMETER][0]
  a = int(mjm.sensor_adr[acc])
  assert np.abs(o["sensordata"][:, a : a + 3] - t["sensordata"][:, a : a + 3]).max() > 1.0


PREDICATES = dict(tree=check_tree, sensors=check_sensors, cutoff=check_cutoff, equality=check_equality, contact=check_contact, rowcut=check_rowcut,
                  batched=check_batched, nosensor=check_nosensor, nogravity=check_nogravity, none=lambda *a: None)


# ---- device ------------------------------------------------------------------------------------------------------------
def _np(t):
  return t.detach().cpu().numpy()


def _device(case, mjm, st):
  import torch

  import mujoco_warp_amd as mjw

  qpos, qvel, ctrl = st
  m = mjw.put_model(mjm, device="cuda")
  if case.batch:
    apply_batched(m, batched_rows(mjm, case.batch, case.seed))
  d = mjw.make_data(mjm, nworld=NWORLD, nconmax=case.nconmax, njmax=case.njmax, device="cuda", m=m)
  f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
  d.qpos[:], d.qvel[:], d.ctrl[:] = f32(qpos), f32(qvel), f32(ctrl)
  d.xfrc_applied[:] = f32(case.xfrc_applied(mjm)).reshape(d.xfrc_applied.shape)
  return m, d


def _rows_equal(case, mjm, d, o):
  """nefc, efc_type and efc_id of the device equal the oracle's (contact ids through the contacts' geoms)."""
  bad = []
  nefc = _np(d.nefc).reshape(-1)
  typ, eid = _np(d.efc.type), _np(d.efc.id)
  geom = _np(d.contact.geom)
  for w in range(NWORLD):
    n = int(o["nefc"][w, 0])
    if int(nefc[w]) != n:
      bad.append(f"nefc[w{w}] {int(nefc[w])} != {n}")
      continue
    n = min(n, case.njmax)
    if not np.array_equal(typ[w, :n], o["efc_type"][w, :n]):
      bad.append(f"efc_type[w{w}]")
      continue
    og = o["con_geom"][w].reshape(-1, 2)
    for r in range(n):
      if typ[w, r] >= 5:  # contact rows: the same geom pair
        if not np.array_equal(geom[eid[w, r]], og[o["efc_id"][w, r]]):
          bad.append(f"efc_id[w{w}, {r}]: contact geoms {geom[eid[w, r]].tolist()} != {og[o['efc_id'][w, r]].tolist()}")
      elif eid[w, r] != o["efc_id"][w, r]:
        bad.append(f"efc_id[w{w}, {r}] {eid[w, r]} != {o['efc_id'][w, r]}")
  return bad


def _sensor_kernels(m, d):
  """The sensor kernels one traced step launches (the step advances d: call it last)."""
  import torch

  from mujoco_warp_amd.forward import StepTracer

  tr = StepTracer()
  tr.step(m, d)
  torch.cuda.synchronize()
  return [k for k, _ in tr.durations()[0] if "sensor" in k]


def run_case(case):
  """The device against the oracle on one case: {"values": {field: {device, fp32_oracle, bar}} in strict units, "kernels",
  "failures": [...]} -- see the module docstring."""
  import torch

  import mujoco_warp_amd as mjw

  mjm = case.model()
  st = case.states(mjm)
  o = reference(case, mjm, st)
  o32 = oracle_run(case, mjm, st, real_bits="32f", solution=o)
  slots = stage_slots(mjm)
  bad, values = [], {}
  m, d = _device(case, mjm, st)
  d.sensordata.fill_(SENTINEL)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  fwd = {f: _np(getattr(d, f)).copy() for f in FIELDS}
  if case.flag & DSBL_SENSOR:
    if not (fwd["sensordata"] == np.float32(SENTINEL)).all():
      bad.append("DSBL_SENSOR: forward wrote sensordata")
  else:
    # a. the kernel on the oracle's accelerations and row forces
    if case.rows:
      bad += _rows_equal(case, mjm, d, o)
    if not bad:
      n = min(case.njmax, o["efc_force"].shape[1])
      d.qacc[:] = torch.as_tensor(o["qacc"], dtype=torch.float32, device="cuda")
      d.efc.force[:, :n] = torch.as_tensor(o["efc_force"][:, :n], dtype=torch.float32, device="cuda")
      mjw.sensor_acc(m, d)
      torch.cuda.synchronize()
      for f in FIELDS:
        dev, noise = strict_units(_np(getattr(d, f)), o[f]), strict_units(o32[f], o[f])
        values[f] = dict(device=dev, fp32_oracle=noise, bar=bar(case, noise))
        if not dev <= values[f]["bar"]:
          bad.append(f"{f}: {dev:.3g} strict units > bar {values[f]['bar']:.3g} (fp32 oracle {noise:.3g})")
      got = _np(d.sensordata)
      untouched = np.concatenate([slots[1], slots[2]])
      if not np.array_equal(got[:, untouched], fwd["sensordata"][:, untouched]):
        bad.append("sensor_acc changed a position / velocity slot")
  # b. stage isolation on a fresh Data: each stage writes exactly its sensors' slots, bitwise what forward gave
  m2, d2 = _device(case, mjm, st)
  for stage in ("fwd_position", "fwd_velocity", "fwd_actuation", "fwd_acceleration", "solve"):
    getattr(mjw, stage)(m2, d2)
  d2.sensordata.fill_(SENTINEL)
  seen = np.zeros(mjm.nsensordata, bool)
  for k, fn in ((1, mjw.sensor_pos), (2, mjw.sensor_vel), (3, mjw.sensor_acc)):
    fn(m2, d2)
    torch.cuda.synchronize()
    got = _np(d2.sensordata)
    if not (case.flag & DSBL_SENSOR):
      seen[slots[k]] = True
    if not (got[:, ~seen] == np.float32(SENTINEL)).all():
      bad.append(f"stage {k} wrote a slot of another stage")
    if not np.array_equal(got[:, seen].view(np.uint32), fwd["sensordata"][:, seen].view(np.uint32)):
      bad.append(f"stage {k}: slots differ from forward's ({np.abs(got[:, seen] - fwd['sensordata'][:, seen]).max():.3g})")
    if (got[:, seen] == np.float32(SENTINEL)).any():
      bad.append(f"stage {k} left a slot of its own unwritten")
  if not (case.flag & DSBL_SENSOR):
    for f in ("cacc", "cfrc_int", "cfrc_ext"):
      getattr(d2, f).fill_(SENTINEL)
    mjw.rne_postconstraint(m2, d2)
    torch.cuda.synchronize()
    for f in ("cacc", "cfrc_int", "cfrc_ext"):
      if not np.array_equal(_np(getattr(d2, f)).view(np.uint32), fwd[f].view(np.uint32)):
        bad.append(f"rne_postconstraint: {f} differs from forward's ({np.abs(_np(getattr(d2, f)) - fwd[f]).max():.3g})")
  kernels = _sensor_kernels(m2, d2)
  want = [] if case.flag & DSBL_SENSOR else ["mjw::sensor_coll_kernel" if (np.asarray(mjm.sensor_type) == S_GEOMDIST).any() else "mjw::sensor_acc_kernel"]
  if [k.split("(")[0] for k in kernels] != want:
    bad.append(f"kernels {kernels} != {want}")
  return dict(id=case.id, edge=case.edge, nbody=int(mjm.nbody), nv=int(mjm.nv), nsensor=int(mjm.nsensor), nefc=o["nefc"].reshape(-1).tolist(),
              values=values, kernels=kernels, failures=bad)
