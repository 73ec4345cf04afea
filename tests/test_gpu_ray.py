"""mjw.rays / mjw.ray on the device (csrc/mjw_ray.hip) against the float64 yardstick tests/ray_ref.py.

The yardstick casts from the geom frames the device itself computed (d.geom_xpos / d.geom_xmat read back after
one mjw.forward), so only the ray code is under test.  Only decisive rays are compared (ray_ref.cast: the
nearest two geoms more than 1e-3 apart, and the same geom / distance / normal under six 1e-4 perturbations of
the direction); every test asserts that at most 2 % of its rays are skipped that way.  Geom ids must match
exactly; distance and normal to atol = rtol = 5e-4, the bar of the reference's ray_test.py (_TOLERANCE * 10).
"""

import os

import numpy as np
import pytest

from tests import ray_ref
from tests.common import ROOT, np_
from tests.ray_scenes import ALL_TYPES_XML, aimed_rays

pytestmark = pytest.mark.gpu

TOL = 5e-4
MAX_SKIPPED = 0.02


def _device(mjm, nworld, qpos=None, **sizes):
  """Model and Data on the device after one forward, and the geom frames it computed (float64 numpy)."""
  import torch

  import mujoco_warp_amd as mjw

  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m, **sizes)
  if qpos is not None:
    d.qpos[:] = torch.as_tensor(np.asarray(qpos), dtype=torch.float32, device="cuda")
  mjw.forward(m, d)
  torch.cuda.synchronize()
  return m, d, _frames(mjm, d)


def _frames(mjm, d):
  return np_(d.geom_xpos).reshape(d.nworld, mjm.ngeom, 3), np_(d.geom_xmat).reshape(d.nworld, mjm.ngeom, 3, 3)


def _rays(m, d, pnt, vec, geomgroup=None, flg_static=True, bodyexclude=None):
  """mjw.rays from numpy inputs (pnt / vec: (nb, nray, 3)); returns geomid, dist, normal as numpy."""
  import torch

  import mujoco_warp_amd as mjw

  nray = pnt.shape[1]
  t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
  excl = t(np.full(nray, -1) if bodyexclude is None else bodyexclude, torch.int32)
  dist = torch.full((d.nworld, nray), 7.0, dtype=torch.float32, device="cuda")
  geomid = torch.full((d.nworld, nray), 7, dtype=torch.int32, device="cuda")
  normal = torch.full((d.nworld, nray, 3), 7.0, dtype=torch.float32, device="cuda")
  mjw.rays(m, d, t(pnt, torch.float32), t(vec, torch.float32), geomgroup, flg_static, excl, dist, geomid, normal)
  torch.cuda.synchronize()
  return geomid.cpu().numpy(), np_(dist), np_(normal)


class _Tally:
  """Compares device results with the yardstick on decisive rays and counts the skipped ones."""

  def __init__(self):
    self.total = self.skipped = 0
    self.hits = np.zeros(8, dtype=int)  # decisive first hits per geom type

  def world(self, mjm, xpos, xmat, pnt, vec, got, label, **kw):
    """pnt / vec: (nray, 3) as the device saw them (float32 values); got: (geomid, dist, normal) of that world."""
    pnt, vec = np.asarray(pnt, dtype=np.float32).astype(np.float64), np.asarray(vec, dtype=np.float32).astype(np.float64)
    g, x, n, ok = ray_ref.cast(mjm, xpos, xmat, pnt, vec, **kw)
    gid, dist, nrm = got
    self.total += len(g)
    self.skipped += int((~ok).sum())
    bad = np.nonzero(ok & (gid != g))[0]
    assert len(bad) == 0, f"{label}: geom id of ray {bad[0]}: device {gid[bad[0]]} (dist {dist[bad[0]]}), yardstick {g[bad[0]]} (dist {x[bad[0]]})"
    np.testing.assert_allclose(dist[ok], x[ok], rtol=TOL, atol=TOL, err_msg=f"{label}: dist")
    np.testing.assert_allclose(nrm[ok], n[ok], rtol=TOL, atol=TOL, err_msg=f"{label}: normal")
    miss = gid < 0
    assert np.all(dist[miss] == -1.0) and not nrm[miss].any(), f"{label}: a miss must give dist -1 and a zero normal"
    hit = ok & (g >= 0)
    self.hits += np.bincount(np.asarray(mjm.geom_type)[g[hit]], minlength=8)
    return g, ok

  def check_skipped(self):
    share = self.skipped / max(self.total, 1)
    print(f"skipped {self.skipped} of {self.total} rays ({share:.4f})")
    assert share <= MAX_SKIPPED, f"{self.skipped} of {self.total} rays are non-decisive"


# ---- 1. all geom types ---------------------------------------------------------------------------------
def test_gpu_rays_all_types_against_yardstick():
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  nworld = 3
  qpos = np.array([[-1.0, -1.0, 1.0, 1, 0, 0, 0], [2.0, 2.0, 1.5, 0.8, 0.6, 0, 0], [0.5, -1.0, 2.0, 0.5, 0.5, 0.5, 0.5]])
  m, d, (xpos, xmat) = _device(mjm, nworld, qpos)
  np.testing.assert_allclose(xpos[:, 8], qpos[:, :3], atol=1e-6)  # the free body sits where each world put it
  tally = _Tally()
  for nray in (1, 63, 64, 65, 300):  # a lane, under / at / over a wave, over the 256-ray tile
    pv = [aimed_rays(xpos[w], nray, seed=100 * nray + w) for w in range(nworld)]
    pnt, vec = np.stack([p for p, _ in pv]), np.stack([v for _, v in pv])
    gid, dist, nrm = _rays(m, d, pnt, vec)
    for w in range(nworld):
      tally.world(mjm, xpos[w], xmat[w], pnt[w], vec[w], (gid[w], dist[w], nrm[w]), f"nray {nray} world {w}")
  tally.check_skipped()
  print("decisive first hits per geom type", tally.hits)
  assert (tally.hits >= 10).all(), f"a geom type is the first hit of fewer than 10 decisive rays: {tally.hits}"


# ---- 2. the reference's scene and rays -------------------------------------------------------------------
# (pnt, vec before normalisation, geom id recorded by the reference's ray_test.py; None: by the yardstick)
REFERENCE_RAYS = [
  ((12.146, 1.865, 3.895), (0.0, 0.0, -1.0), -1),  # nothing
  ((2.0, 1.0, 3.0), (0.1, 0.2, -1.0), 0),  # plane
  ((0.0, 0.0, -0.5), (0.1, 0.2, -1.0), -1),  # wrong side of the plane
  ((0.0, 0.0, 1.6), (0.1, 0.2, -1.0), 1),  # sphere
  ((0.5, 1.0, 1.6), (0.0, 0.05, -1.0), 2),  # capsule from above
  ((-0.5, 1.0, 0.05), (0.0, 0.05, 1.0), 2),  # capsule from below
  ((0.0, 1.0, 0.75), (1.0, 0.0, 0.0), 2),  # capsule's cylinder from the side
  ((2.0, 0.0, 0.05), (0.0, 0.05, 1.0), None),  # cylinder
  ((1.0, 0.0, 1.6), (0.0, 0.05, -1.0), 3),  # box from above
  ((1.0, 0.0, 0.05), (0.0, 0.05, 1.0), 3),  # box from below
  ((2.0, 2.0, 2.0), (-1.0, -1.0, -1.0), 4),  # tetrahedron
  ((4.0, 2.0, 2.0), (2.0, 1.0, 1.0), -1),  # looking away from the dodecahedron
  ((4.0, 2.0, 2.0), (-2.0, -1.0, -1.0), 5),  # dodecahedron
  ((0.0, 2.0, 2.0), (0.0, 0.0, -1.0), 6),  # heightfield from straight above
]


def test_gpu_rays_reference_scene():
  from mujoco_warp_amd import mjcf

  base = os.path.join(ROOT, "tests", "golden", "ray")
  with open(os.path.join(base, "ray.xml")) as f:
    xml = f.read().replace("</worldbody>", '<body name="free" pos="-3 -3 1"><freejoint/><geom size=".1"/></body></worldbody>')
  mjm = mjcf.load_model_from_string(xml, basedir=base)
  assert mjm.ngeom == 9 and list(mjm.geom_type[:8]) == [0, 2, 3, 6, 7, 7, 1, 5]  # ids 0-7 keep their meaning
  m, d, (xpos, xmat) = _device(mjm, 1)
  pnt = np.array([p for p, _, _ in REFERENCE_RAYS], dtype=np.float64)
  vec = np.array([v for _, v, _ in REFERENCE_RAYS], dtype=np.float64)
  vec /= np.linalg.norm(vec, axis=1, keepdims=True)
  gid, dist, nrm = _rays(m, d, pnt[None], vec[None])
  p32, v32 = pnt.astype(np.float32).astype(np.float64), vec.astype(np.float32).astype(np.float64)
  g, x, n, ok = ray_ref.cast(mjm, xpos[0], xmat[0], p32, v32)
  want = np.array([g[i] if e is None else e for i, (_, _, e) in enumerate(REFERENCE_RAYS)])
  np.testing.assert_array_equal(g, want)  # the yardstick agrees with the recorded ids
  assert g[7] == 7  # the cylinder
  np.testing.assert_array_equal(gid[0], want)
  np.testing.assert_allclose(dist[0], x, rtol=TOL, atol=TOL)  # every ray, decisive or not
  np.testing.assert_allclose(nrm[0][ok], n[ok], rtol=TOL, atol=TOL)
  # the same rays one at a time through ray()
  import torch

  import mujoco_warp_amd as mjw

  for i in (1, 10, 13):
    d1, g1, n1 = mjw.ray(m, d, torch.tensor(pnt[i], dtype=torch.float32, device="cuda").reshape(1, 1, 3),
                         torch.tensor(vec[i], dtype=torch.float32, device="cuda").reshape(1, 1, 3))
    assert int(g1[0, 0]) == want[i] and abs(float(d1[0, 0]) - dist[0, i]) == 0.0


# ---- 3. filters ------------------------------------------------------------------------------------------
FILTER_XML = """<mujoco model="ray_filters">
  <asset><material name="ghost" rgba="1 1 1 0"/><material name="solid" rgba="0.3 0.3 0.3 1"/></asset>
  <worldbody>
    <geom name="plane" type="plane" size="0 0 1"/>
    <geom name="a" type="sphere" size=".3" pos="0 0 1" group="1"/>
    <geom name="b" type="sphere" size=".3" pos="2 0 1" rgba="1 0 0 0"/>
    <geom name="c" type="sphere" size=".3" pos="4 0 1" material="ghost"/>
    <geom name="e" type="sphere" size=".3" pos="6 0 1" material="solid" rgba="1 0 0 0"/>
    <body name="free" pos="-2 0 1"><freejoint/><geom name="f" type="sphere" size=".3" group="7"/></body>
  </worldbody>
</mujoco>"""


def test_gpu_rays_filters():
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(FILTER_XML)
  nworld = 2
  m, d, (xpos, xmat) = _device(mjm, nworld)
  free_body = int(mjm.geom_bodyid[5])
  assert free_body == 1 and mjm.body_weldid[free_body] != 0
  # straight down on a, b, c, e, f (a little off centre), and up at a from below it
  pnt = np.array([[0.05, 0.02, 3], [2.05, 0.02, 3], [4.05, 0.02, 3], [6.05, 0.02, 3], [-1.95, 0.02, 3], [0.05, 0.02, 0.2]], dtype=np.float64)
  vec = np.array([[0, 0, -1.0]] * 5 + [[0, 0, 1.0]])
  tally = _Tally()

  def run(label, want, **kw):
    gid, dist, nrm = _rays(m, d, pnt[None], vec[None], **kw)
    for w in range(nworld):
      tally.world(mjm, xpos[w], xmat[w], pnt, vec, (gid[w], dist[w], nrm[w]), f"{label} world {w}", **kw)
      np.testing.assert_array_equal(gid[w], want, err_msg=label)
    return dist

  # alpha 0 on the geom (b) and on the material (c) is skipped; a solid material wins over the geom's own alpha (e)
  run("no filter", [1, 0, 0, 4, 5, 1])
  run("all -1", [1, 0, 0, 4, 5, 1], geomgroup=(-1,) * 6)
  run("group 0 only", [0, 0, 0, 4, 0, -1], geomgroup=(1, 0, 0, 0, 0, 0))  # a (group 1) and f (group 7 -> 5) are filtered
  run("group 5 only", [-1, -1, -1, -1, 5, -1], geomgroup=(0, 0, 0, 0, 0, 1))  # group 7 clamps to 5
  dist = run("no group", [-1] * 6, geomgroup=(0,) * 6)
  assert np.all(dist == -1.0)
  run("not static", [-1, -1, -1, -1, 5, -1], flg_static=False)
  run("bodyexclude mix", [-1, 0, 0, -1, 0, 1], bodyexclude=np.array([0, -1, free_body, 0, free_body, -1]))
  run("bodyexclude world / free", [1, -1, 0, 4, 5, -1], bodyexclude=np.array([free_body, 0, -1, free_body, 0, 0]))
  tally.check_skipped()

  # geom_rgba batched per world: a is transparent in world 1 only, so the upward ray misses there alone
  rgba = m.geom_rgba.repeat(nworld, 1, 1).contiguous()
  assert tuple(rgba.shape) == (nworld, mjm.ngeom, 4)
  rgba[1, 1, 3] = 0.0
  keep = m.geom_rgba
  m.geom_rgba = rgba
  gid, dist, nrm = _rays(m, d, pnt[None], vec[None])
  m.geom_rgba = keep
  np.testing.assert_array_equal(gid[0], [1, 0, 0, 4, 5, 1])
  np.testing.assert_array_equal(gid[1], [0, 0, 0, 4, 5, -1])
  assert dist[1, 5] == -1.0 and not nrm[1, 5].any()
  for w in range(nworld):
    g, x, n, ok = ray_ref.cast(mjm, xpos[w], xmat[w], pnt, vec, geom_rgba=rgba[w].cpu().numpy())
    assert ok.all()
    np.testing.assert_array_equal(gid[w], g)
    np.testing.assert_allclose(dist[w], x, rtol=TOL, atol=TOL)
  # mat_rgba batched the same way: the ghost becomes solid in world 0
  mat = m.mat_rgba.repeat(nworld, 1, 1).contiguous()
  mat[0, 0, 3] = 1.0
  keep = m.mat_rgba
  m.mat_rgba = mat
  gid, _, _ = _rays(m, d, pnt[None], vec[None])
  m.mat_rgba = keep
  assert gid[0, 2] == 3 and gid[1, 2] == 0


# ---- 4. broadcast ----------------------------------------------------------------------------------------
def test_gpu_rays_broadcast_and_ray_shapes():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  nworld, nray = 4, 70
  qpos = np.tile([-1.0, -1.0, 1.0, 1, 0, 0, 0], (nworld, 1))
  qpos[:, 0] += 0.7 * np.arange(nworld)  # the free body differs per world, the rays do not
  m, d, (xpos, xmat) = _device(mjm, nworld, qpos)
  pnt, vec = aimed_rays(xpos[0], nray, seed=11)
  one = _rays(m, d, pnt[None], vec[None])
  tiled = _rays(m, d, np.tile(pnt, (nworld, 1, 1)), np.tile(vec, (nworld, 1, 1)))
  mixed = _rays(m, d, pnt[None], np.tile(vec, (nworld, 1, 1)))
  for a, b, c in zip(one, tiled, mixed):
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
  assert len({tuple(one[0][w]) for w in range(nworld)}) > 1  # the worlds do differ
  p1 = torch.tensor([[[-3.0, -1.0, 1.0]]], device="cuda")
  v1 = torch.tensor([[[1.0, 0.0, 0.0]]], device="cuda")
  dist, geomid, normal = mjw.ray(m, d, p1, v1)
  assert tuple(dist.shape) == (nworld, 1) and tuple(geomid.shape) == (nworld, 1) and tuple(normal.shape) == (nworld, 1, 3)
  assert dist.dtype == torch.float32 and geomid.dtype == torch.int32 and normal.dtype == torch.float32
  # the ball at x = -1 + 0.7 w, radius 0.2, seen from x = -3 along +x
  np.testing.assert_allclose(np_(dist)[:, 0], 2.0 + 0.7 * np.arange(nworld) - 0.2, atol=1e-5)
  np.testing.assert_array_equal(geomid.cpu().numpy()[:, 0], 8)
  np.testing.assert_allclose(np_(normal)[:, 0], np.tile([-1.0, 0, 0], (nworld, 1)), atol=1e-6)
  dist, geomid, normal = mjw.ray(m, d, p1, v1, bodyexclude=1)
  assert np.all(geomid.cpu().numpy() != 8)
  # nray == 0 is a no-op
  mjw.rays(m, d, torch.zeros(1, 0, 3, device="cuda"), torch.zeros(1, 0, 3, device="cuda"), None, True,
           torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(nworld, 0, device="cuda"),
           torch.zeros(nworld, 0, dtype=torch.int32, device="cuda"), torch.zeros(nworld, 0, 3, device="cuda"))


# ---- 5. more geoms than one LDS chunk ----------------------------------------------------------------------
def test_gpu_rays_geom_chunk_edge_and_tie():
  from mujoco_warp_amd import mjcf

  rng = np.random.default_rng(42)
  nx, ny = 15, 10
  grid = np.stack(np.meshgrid(np.arange(nx) * 0.4, np.arange(ny) * 0.4, indexing="ij"), -1).reshape(-1, 2)
  pos = np.concatenate([grid + rng.uniform(-0.03, 0.03, grid.shape), 0.5 + rng.uniform(-0.1, 0.1, (len(grid), 1))], axis=1)
  pos = pos[rng.permutation(len(pos))]  # neighbours in space lie in different 128-geom chunks
  ida, idb = 5, 140
  pos[idb] = pos[ida]  # two coincident spheres, one in each chunk
  assert len(pos) == 150
  geoms = "".join(f'<geom type="sphere" size="0.15" pos="{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}"/>' for p in pos)
  mjm = mjcf.load_model_from_string(f'<mujoco><worldbody>{geoms}<body pos="2 1.5 1.2"><freejoint/><geom type="sphere" size=".15"/></body>'
                                    "</worldbody></mujoco>")
  assert mjm.ngeom == 151
  nworld, nray = 2, 200
  qpos = np.array([[2.0, 1.5, 1.2, 1, 0, 0, 0], [1.0, 0.5, 1.0, 1, 0, 0, 0]])
  m, d, (xpos, xmat) = _device(mjm, nworld, qpos)
  tally = _Tally()
  # steep rays from 1 to 1.6 above jittered sphere centres; every seventh direction is not normalised
  tgt = np.stack([xpos[w][rng.integers(0, mjm.ngeom, nray)] for w in range(nworld)]) + rng.normal(0, 0.05, (nworld, nray, 3))
  pnt = tgt + np.concatenate([rng.uniform(-0.4, 0.4, (nworld, nray, 2)), rng.uniform(1.0, 1.6, (nworld, nray, 1))], axis=2)
  vec = tgt - pnt
  vec /= np.linalg.norm(vec, axis=2, keepdims=True)
  vec[:, ::7] *= rng.uniform(0.3, 3.0, (nworld, len(range(0, nray, 7)), 1))
  # ray 0 of every world goes straight down through the coincident pair
  pnt[:, 0] = pos[ida] + [0.01, 0.0, 2.0]
  vec[:, 0] = [0.0, 0.0, -1.0]
  gid, dist, nrm = _rays(m, d, pnt, vec)
  seen = set()
  for w in range(nworld):
    g, ok = tally.world(mjm, xpos[w], xmat[w], pnt[w], vec[w], (gid[w], dist[w], nrm[w]), f"world {w}")
    seen |= set(g[ok & (g >= 0)].tolist())
    assert gid[w, 0] == ida, f"equal distances must go to the lowest geom id: got {gid[w, 0]}"
  assert min(seen) < 128 <= max(seen) and len(seen) > 60  # hits on both sides of the chunk edge
  # the tie ray is non-decisive by construction (gap 0): leave it out of the share
  tally.skipped -= nworld
  tally.check_skipped()


# ---- 6. a sparse model with real meshes ----------------------------------------------------------------------
def test_gpu_rays_sparse_aloha_cloth():
  import torch

  import mujoco_warp_amd as mjw
  from tests.cloth_common import aloha_model, aloha_states
  from tests.common import gpu_from_state

  mjm = aloha_model()
  nworld = 2
  qpos, qvel, ctrl = aloha_states(mjm, nworld, seed=3)
  m, d = gpu_from_state(mjm, qpos, qvel, ctrl, njmax=16384, nconmax=4096)
  assert m.is_sparse and mjm.nmeshface > 1000
  mjw.forward(m, d)
  torch.cuda.synchronize()
  xpos, xmat = _frames(mjm, d)
  table = mjm.geom_names.index("table")
  c, h = xpos[0, table], np.asarray(mjm.geom_size[table])
  # an 8 x 8 grid straight down over the table, at irrational offsets from its centre
  u = (np.arange(8) - 3.5) / 4.0 * 0.97 + 0.0123
  gx, gy = np.meshgrid(c[0] + u * h[0], c[1] + (u + 0.0071) * h[1], indexing="ij")
  pnt = np.stack([gx.ravel(), gy.ravel(), np.full(64, c[2] + 1.5)], axis=1)
  vec = np.tile([0.0, 0.0, -1.0], (64, 1))
  pnt = pnt.astype(np.float32).astype(np.float64)  # the values the device sees
  # The scene's table is three surfaces within 0.9 mm of each other (the visual tabletop and tablelegs meshes,
  # group 2, top at z = 0.0008, and the collision box, group 3, top at z = 0.0009), so an unfiltered ray that
  # ends on the table is non-decisive by the 1e-3 gap rule whatever the code does.  The decisive comparison
  # therefore casts at the collision geoms (group 3: the table box and the arms' collision meshes), as a lidar
  # would; the unfiltered cast is checked below with the rule that fits near-coincident surfaces.
  collision = (0, 0, 0, 1, 0, 0)
  gid, dist, nrm = _rays(m, d, pnt[None], vec[None], geomgroup=collision)
  tally = _Tally()
  for w in range(nworld):
    g, ok = tally.world(mjm, xpos[w], xmat[w], pnt, vec, (gid[w], dist[w], nrm[w]), f"collision group, world {w}", geomgroup=collision)
    assert (g >= 0).all()  # every ray ends on the table or on something above it
    assert set(np.asarray(mjm.geom_group)[g].tolist()) == {3}
  print("decisive first hits per geom type", tally.hits)
  assert tally.hits[ray_ref.MESH] >= 10  # the arms' meshes are met
  tally.check_skipped()
  # unfiltered, every ray: the distance matches the yardstick's nearest, and the geom the device names lies within
  # the 1e-3 gap of the nearest in the yardstick's own distances
  gid, dist, nrm = _rays(m, d, pnt[None], vec[None])
  for w in range(nworld):
    every, _ = ray_ref.cast_all(mjm, xpos[w], xmat[w], pnt, vec, ray_ref.eliminated(mjm))
    g, x, _, _ = ray_ref.nearest(every, np.zeros(every.shape + (3,)))
    assert (gid[w] >= 0).all() and (g >= 0).all()
    np.testing.assert_allclose(dist[w], x, rtol=TOL, atol=TOL)
    named = every[gid[w], np.arange(64)]
    assert np.all(named >= 0) and np.all(named - x <= 1e-3)


# ---- 7. graph capture ----------------------------------------------------------------------------------------
def test_gpu_rays_graph_capture():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  nworld, nray = 3, 130
  m, d, (xpos, xmat) = _device(mjm, nworld)
  mjw.step(m, d)
  torch.cuda.synchronize()
  xpos, _ = _frames(mjm, d)
  p, v = aimed_rays(xpos[0], nray, seed=5)
  pnt = torch.as_tensor(p[None], dtype=torch.float32, device="cuda").contiguous()
  vec = torch.as_tensor(v[None], dtype=torch.float32, device="cuda").contiguous()
  excl = torch.full((nray,), -1, dtype=torch.int32, device="cuda")
  out = lambda: (torch.zeros(nworld, nray, device="cuda"), torch.zeros(nworld, nray, dtype=torch.int32, device="cuda"),
                 torch.zeros(nworld, nray, 3, device="cuda"))
  eager, graphed = out(), out()
  mjw.rays(m, d, pnt, vec, None, True, excl, *eager)
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=s):
    mjw.rays(m, d, pnt, vec, None, True, excl, *graphed)
  torch.cuda.synchronize()
  assert not graphed[1].any()  # capture records, it does not run
  for _ in range(2):
    for t in graphed:
      t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
      assert torch.equal(a, b)
  assert int((eager[1] >= 0).sum()) > nray  # the rays do hit things
