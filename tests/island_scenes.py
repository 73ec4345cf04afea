"""Small scenes for the island tests.  Each carries its expected `nisland` and `tree_island`, written out by hand,
and the constraint row types it exists for (`rows`: at least one row of each must be present in every world).

Trees are numbered in the order of their first dof, i.e. in body order here.  Geoms that only give a body mass have
contype = conaffinity = 0, so that a scene has exactly the rows it is there for.
"""

from __future__ import annotations

import dataclasses
import os
from typing import Optional, Sequence

import numpy as np

from tests.island_ref import (CONTACT_ELLIPTIC, CONTACT_FRICTIONLESS, CONTACT_PYRAMIDAL, EQUALITY, FRICTION_DOF, FRICTION_TENDON, LIMIT_JOINT,
                              LIMIT_TENDON)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASS = '<geom type="sphere" size=".05" contype="0" conaffinity="0"/>'


@dataclasses.dataclass
class Scene:
  id: str
  xml: str
  nisland: int
  tree_island: Sequence[int]
  rows: Sequence[int] = ()        # efc types that must be present
  generic: bool = False           # the rows it exists for take the Jacobian-scan path
  qpos: Optional[dict] = None     # {qpos address: value} on top of qpos0
  path: Optional[str] = None      # a model file in place of xml
  njmax: int = 64
  nconmax: int = 8

  def model(self):
    from mujoco_warp_amd import mjcf

    return mjcf.load_model(self.path) if self.path else mjcf.load_model_from_string(self.xml)

  def state(self, mjm, nworld):
    qpos = np.tile(np.asarray(mjm.qpos0, dtype=np.float64), (nworld, 1))
    for a, v in (self.qpos or {}).items():
      qpos[:, a] = v
    return qpos


def free_bodies(n, spacing=1.0):
  return "".join(f'<body name="b{i}" pos="{spacing * i} 0 1"><freejoint/>{MASS}</body>' for i in range(n))


def slide_bodies(n, extra=""):
  return "".join(f'<body name="b{i}" pos="{i} 0 1"><joint name="j{i}" type="slide" axis="0 0 1"{extra}/>{MASS}</body>' for i in range(n))


def welds(pairs, kind="weld"):
  return "".join(f'<{kind} body1="b{a}" body2="b{b}"' + (' anchor="0 0 0"' if kind == "connect" else "") + "/>" for a, b in pairs)


def joint_eqs(pairs):
  return "".join(f'<joint joint1="j{a}" joint2="j{b}"/>' for a, b in pairs)


def wrap(world, equality="", tendon="", option=""):
  return (f"<mujoco><option timestep=\"0.002\" {option}/><worldbody>{world}</worldbody>"
          + (f"<tendon>{tendon}</tendon>" if tendon else "") + (f"<equality>{equality}</equality>" if equality else "") + "</mujoco>")


def _sphere(name, pos, condim):
  return f'<body name="{name}" pos="{pos}"><freejoint/><geom type="sphere" size=".1" condim="{condim}"/></body>'


def _two_spheres(condim, option=""):
  # two free spheres that overlap by 2 cm, far above anything else
  return wrap(_sphere("s0", "0 0 1", condim) + _sphere("s1", "0 0 1.18", condim), option=option)


_FIXED3 = '<fixed name="t">' + "".join(f'<joint joint="j{i}" coef="1"/>' for i in range(3)) + "</fixed>"

SCENES = [
  # ---- the reference's topologies
  Scene("weld_pair", wrap(free_bodies(2), welds([(0, 1)])), 1, [0, 0], [EQUALITY]),
  Scene("chain_of_three", wrap(free_bodies(3), welds([(0, 1), (1, 2)])), 1, [0, 0, 0], [EQUALITY]),
  Scene("star_hub_last", wrap(free_bodies(4), welds([(3, 0), (3, 1), (3, 2)])), 1, [0, 0, 0, 0], [EQUALITY]),
  Scene("two_pairs", wrap(free_bodies(4), welds([(0, 1), (2, 3)])), 2, [0, 0, 1, 1], [EQUALITY]),
  Scene("weld_and_connect_same_pair", wrap(free_bodies(2), welds([(0, 1)]) + welds([(0, 1)], "connect")), 1, [0, 0], [EQUALITY]),
  Scene("weld_to_world", wrap(free_bodies(2), '<weld body1="b0"/>'), 1, [0, -1], [EQUALITY]),
  Scene("lone_free_body", wrap(free_bodies(1)), 0, [-1]),
  Scene("joint_equality_inside_a_tree",
        wrap(f'<body pos="0 0 1"><joint name="j0" type="hinge" axis="0 1 0"/>{MASS}<body pos="0 0 -.3"><joint name="j1" type="hinge" axis="0 1 0"/>{MASS}</body></body>'
             + free_bodies(1), joint_eqs([(0, 1)])), 1, [0, -1], [EQUALITY], generic=True),
  # ---- every row type
  Scene("joint_frictionloss", wrap(slide_bodies(1, ' frictionloss="1"') + free_bodies(1)), 1, [0, -1], [FRICTION_DOF]),
  Scene("hinge_limit", wrap(f'<body pos="0 0 1"><joint type="hinge" axis="0 1 0" limited="true" range="30 60"/>{MASS}</body>' + free_bodies(1)),
        1, [0, -1], [LIMIT_JOINT]),
  Scene("ball_limit", wrap(free_bodies(1) + f'<body pos="0 1 1"><joint type="ball" limited="true" range="0 30"/>{MASS}</body>'),
        1, [-1, 0], [LIMIT_JOINT], qpos={7: np.cos(np.pi / 4), 8: np.sin(np.pi / 4), 9: 0.0, 10: 0.0}),  # 90 degrees about x
  Scene("tendon_limit", wrap(slide_bodies(3), tendon='<fixed name="t" limited="true" range="1 2"><joint joint="j0" coef="1"/><joint joint="j2" coef="1"/></fixed>'),
        1, [0, -1, 0], [LIMIT_TENDON], generic=True),
  Scene("tendon_frictionloss", wrap(slide_bodies(3), tendon='<fixed name="t" frictionloss="1"><joint joint="j1" coef="1"/><joint joint="j2" coef="1"/></fixed>'),
        1, [-1, 0, 0], [FRICTION_TENDON], generic=True),
  Scene("joint_equality_across_two_trees", wrap(slide_bodies(3), joint_eqs([(0, 2)])), 1, [0, -1, 0], [EQUALITY], generic=True),
  Scene("tendon_equality_across_three_trees", wrap(slide_bodies(4), '<tendon tendon1="t"/>', tendon=_FIXED3), 1, [0, 0, 0, -1], [EQUALITY], generic=True),
  Scene("connect_with_sites",
        wrap("".join(f'<body name="b{i}" pos="{i} 0 1"><freejoint/>{MASS}<site name="s{i}" pos=".1 0 0"/></body>' for i in range(3)),
             '<connect site1="s2" site2="s0"/>'), 1, [0, -1, 0], [EQUALITY]),
  Scene("sphere_on_plane", wrap('<geom type="plane" size="5 5 .1"/>' + _sphere("s0", "0 0 .09", 3) + _sphere("s1", "2 0 1", 3)), 1, [0, -1], [CONTACT_PYRAMIDAL]),
  Scene("spheres_frictionless", _two_spheres(1), 1, [0, 0], [CONTACT_FRICTIONLESS]),
  Scene("spheres_pyramidal", _two_spheres(3), 1, [0, 0], [CONTACT_PYRAMIDAL]),
  Scene("spheres_elliptic", _two_spheres(3, 'cone="elliptic"'), 1, [0, 0], [CONTACT_ELLIPTIC]),
  # ---- the order trap: generic rows coupling (1, 2) and then (0, 2) are one island
  Scene("generic_rows_1_2_then_0_2", wrap(slide_bodies(3), joint_eqs([(1, 2), (0, 2)])), 1, [0, 0, 0], [EQUALITY], generic=True),
  # ---- listing order must not matter
  Scene("weld_chain_reversed", wrap(free_bodies(5), welds([(4, 3), (3, 2), (2, 1), (1, 0)])), 1, [0] * 5, [EQUALITY]),
  Scene("interleaved_chains", wrap(free_bodies(6), welds([(4, 2), (5, 3), (2, 0), (3, 1)])), 2, [0, 1, 0, 1, 0, 1], [EQUALITY]),
  # ---- flex: two pinned ropes of 12 vertices with edge equalities (11 moving vertices = trees each), no contacts
  Scene("flex_ropes", "", 2, [0] * 11 + [1] * 11, [EQUALITY], generic=True, path=os.path.join(ROOT, "models", "test_data", "flex", "rope.xml")),
]
BY_ID = {s.id: s for s in SCENES}


# ---- size edges: n trees as one reversed chain (1 island), or unconstrained but for one coupled pair at the far end.
# One model holds both patterns; a world switches one on through eq_active, so a size costs one model per body kind.
EDGE_WORLDS = ("generic_chain", "generic_far_pair", "typed_chain", "typed_far_pair")


def edge_pairs(ntree, pattern):
  if ntree < 2:
    return []
  return [(i, i - 1) for i in range(ntree - 1, 0, -1)] if pattern == "chain" else [(ntree - 1, ntree - 2)]


def edge_model_xml(ntree, bodies, jacobian=None):
  """bodies "slide": 1-dof slide bodies with, in equality order, the chain's joint equalities, the far pair's joint
  equality (rows that scan J), the chain's connects and the far pair's connect (typed rows): the four EDGE_WORLDS.
  bodies "free": free spheres with the chain's connects and the far pair's connect: the two typed EDGE_WORLDS."""
  chain, far = edge_pairs(ntree, "chain"), edge_pairs(ntree, "far_pair")
  opt = f'jacobian="{jacobian}"' if jacobian else ""
  if bodies == "slide":
    return wrap(slide_bodies(ntree), joint_eqs(chain) + joint_eqs(far) + welds(chain, "connect") + welds(far, "connect"), option=opt)
  return wrap(free_bodies(ntree), welds(chain, "connect") + welds(far, "connect"), option=opt)


def edge_worlds(bodies):
  return EDGE_WORLDS if bodies == "slide" else EDGE_WORLDS[2:]


def edge_eq_active(ntree, bodies):
  """(nworld, neq) eq_active: world k has the equalities of edge_worlds(bodies)[k] on and the others off."""
  nc, nf = len(edge_pairs(ntree, "chain")), len(edge_pairs(ntree, "far_pair"))
  blocks = [nc, nf, nc, nf] if bodies == "slide" else [nc, nf]
  act = np.zeros((len(blocks), sum(blocks)), dtype=np.int32)
  adr = np.concatenate([[0], np.cumsum(blocks)])
  for k in range(len(blocks)):
    act[k, adr[k]:adr[k + 1]] = 1
  return act


def edge_expected(ntree, world):
  """(nisland, tree_island, rows) of one of the EDGE_WORLDS."""
  pattern = "chain" if world.endswith("chain") else "far_pair"
  rows = len(edge_pairs(ntree, pattern)) * (1 if world.startswith("generic") else 3)
  if ntree == 1:
    return 0, [-1], 0
  if pattern == "chain":
    return 1, [0] * ntree, rows
  return 1, [-1] * (ntree - 2) + [0, 0], rows


def edge_njmax(ntree):
  return max(3 * (ntree - 1), 1)


# ---- per-world divergence: three spheres (radius .1) in a column over a plane; qpos per world closes the gap
# between the lowest sphere and the plane (a static partner) and the gap between the upper two
COLUMN_XML = wrap('<geom type="plane" size="5 5 .1"/>' + _sphere("s0", "0 0 .5", 3) + _sphere("s1", "0 0 1", 3) + _sphere("s2", "0 0 1.5", 3))
# z of the three spheres per world -> (nisland, tree_island, contacts)
COLUMN_WORLDS = [
  ((0.5, 1.0, 1.5), 0, [-1, -1, -1], 0),
  ((0.09, 1.0, 1.5), 1, [0, -1, -1], 1),
  ((0.5, 1.0, 1.18), 1, [-1, 0, 0], 1),
  ((0.09, 1.0, 1.18), 2, [0, 1, 1], 2),
]


def column_qpos(mjm):
  qpos = np.tile(np.asarray(mjm.qpos0, dtype=np.float64), (len(COLUMN_WORLDS), 1))
  for w, (z, _, _, _) in enumerate(COLUMN_WORLDS):
    qpos[w, [2, 9, 16]] = z
  return qpos
