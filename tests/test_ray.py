"""Ray casting, host side: the MJCF compiler's new fields (rgba, materials, mesh faces), the float64 yardstick
tests/ray_ref.py against closed-form answers, and the argument validation of mjw.rays / mjw.ray.  The device
kernel itself is tested in tests/test_gpu_ray.py.
"""

import numpy as np
import pytest

from tests import ray_ref
from tests.ray_scenes import ALL_TYPES_XML, aimed_rays, host_frames, quat_mat

EYE = np.eye(3)


class _OneGeom:
  """The model fields ray_ref reads, for one primitive geom on the world body."""

  def __init__(self, gtype, size, rgba=(0.5, 0.5, 0.5, 1.0)):
    self.ngeom = 1
    self.geom_type = np.array([gtype])
    self.geom_size = np.array([size], dtype=np.float64)
    self.geom_bodyid = np.array([0])
    self.body_weldid = np.array([0])
    self.geom_group = np.array([0])
    self.geom_matid = np.array([-1])
    self.geom_rgba = np.array([rgba], dtype=np.float64)
    self.mat_rgba = np.zeros((0, 4))


def _cast1(gtype, size, pos, mat, pnt, vec):
  g, x, n, _ = ray_ref.cast(_OneGeom(gtype, size), np.array([pos], dtype=np.float64), np.array([mat]), np.array([pnt], dtype=np.float64),
                            np.array([vec], dtype=np.float64))
  return int(g[0]), float(x[0]), n[0]


# ---- the compiler ---------------------------------------------------------------------------------
def test_mjcf_rgba_direct_and_through_default_class():
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string("""<mujoco>
    <default><default class="red"><geom rgba="1 0 0 0.25"/></default></default>
    <worldbody>
      <geom type="plane" size="1 1 .1"/>
      <geom type="sphere" size=".1" rgba="0.1 0.2 0.3 0.4"/>
      <geom class="red" type="sphere" size=".1" pos="1 0 0"/>
      <body pos="0 0 1" childclass="red"><freejoint/><geom type="sphere" size=".1"/><geom type="sphere" size=".1" rgba="0 1 0 1"/></body>
    </worldbody></mujoco>""")
  want = [[0.5, 0.5, 0.5, 1.0], [0.1, 0.2, 0.3, 0.4], [1, 0, 0, 0.25], [1, 0, 0, 0.25], [0, 1, 0, 1]]
  np.testing.assert_allclose(mjm.geom_rgba, want)
  assert mjm.nmat == 0 and mjm.mat_rgba.shape == (0, 4)
  np.testing.assert_array_equal(mjm.geom_matid, [-1] * 5)


def test_mjcf_material_alpha_and_matid():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string("""<mujoco>
    <asset><material name="solid"/><material name="ghost" rgba="0.2 0.3 0.4 0"/></asset>
    <worldbody>
      <geom type="plane" size="1 1 .1" material="solid"/>
      <geom type="sphere" size=".1" material="ghost"/>
      <body pos="0 0 1"><freejoint/><geom type="sphere" size=".1"/></body>
    </worldbody></mujoco>""")
  assert mjm.nmat == 2
  np.testing.assert_allclose(mjm.mat_rgba, [[1, 1, 1, 1], [0.2, 0.3, 0.4, 0]])
  np.testing.assert_array_equal(mjm.geom_matid, [0, 1, -1])
  np.testing.assert_allclose(mjm.geom_rgba[1], [0.5, 0.5, 0.5, 1.0])  # a material leaves the geom's own rgba alone
  with pytest.raises(ValueError):
    mjcf.load_model_from_string('<mujoco><worldbody><geom size=".1" material="nope"/></worldbody></mujoco>')
  m = mjw.put_model(mjm, device="cpu")
  assert tuple(m.geom_rgba.shape) == (1, 3, 4) and tuple(m.mat_rgba.shape) == (1, 2, 4) and m.nmat == 2
  np.testing.assert_array_equal(m.geom_matid.numpy(), [0, 1, -1])
  np.testing.assert_array_equal(m.geom_group.numpy(), [0, 0, 0])


def test_mjcf_mesh_face_indexes_deduplicated_vertices():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  # a tetrahedron given as 4 x 3 separate corners (every vertex three times), then a second mesh
  corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
  tris = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
  soup = corners[tris.reshape(-1)]
  vert = " ".join(repr(float(x)) for x in soup.reshape(-1))
  face = " ".join(str(i) for i in range(12))
  mjm = mjcf.load_model_from_string(f"""<mujoco>
    <asset><mesh name="soup" vertex="{vert}" face="{face}"/>
           <mesh name="tet" vertex="0 0 0  2 0 0  0 2 0  0 0 2" face="0 2 1  0 1 3  0 3 2  1 2 3"/></asset>
    <worldbody><geom type="mesh" mesh="soup"/><geom type="mesh" mesh="tet" pos="3 0 0"/>
      <body pos="0 0 3"><freejoint/><geom size=".1"/></body></worldbody></mujoco>""")
  assert mjm.nmeshface == 8 and mjm.mesh_face.shape == (8, 3) and mjm.mesh_face.dtype == np.int32
  np.testing.assert_array_equal(mjm.mesh_faceadr, [0, 4])
  np.testing.assert_array_equal(mjm.mesh_facenum, [4, 4])
  assert mjm.mesh_vertnum[0] == 4  # the repeated corners collapsed
  for i in range(2):
    va, fa = mjm.mesh_vertadr[i], mjm.mesh_faceadr[i]
    v = mjm.mesh_vert[va : va + mjm.mesh_vertnum[i]]
    f = mjm.mesh_face[fa : fa + mjm.mesh_facenum[i]]
    assert f.min() >= 0 and f.max() < mjm.mesh_vertnum[i]
    np.testing.assert_allclose(v[f], (corners * (1, 2)[i])[tris])  # the same triangles, corner for corner
  m = mjw.put_model(mjm, device="cpu")
  assert m.nmeshface == 8 and tuple(m.mesh_face.shape) == (8, 3)
  np.testing.assert_array_equal(m.mesh_face.numpy(), mjm.mesh_face)
  np.testing.assert_array_equal(m.mesh_facenum.numpy(), [4, 4])


# ---- the yardstick against closed forms ---------------------------------------------------------------
def test_ref_sphere_along_axis_and_from_inside_and_unnormalised():
  D, r = 3.0, 0.5
  g, x, n = _cast1(ray_ref.SPHERE, [r, 0, 0], [0, 0, 0], EYE, [0, 0, D], [0, 0, -1])
  assert g == 0 and x == pytest.approx(D - r, abs=1e-12)
  np.testing.assert_allclose(n, [0, 0, 1], atol=1e-12)
  # origin inside: the far root, outward normal
  g, x, n = _cast1(ray_ref.SPHERE, [r, 0, 0], [0, 0, 0], EYE, [0, 0, 0.2], [0, 0, -1])
  assert g == 0 and x == pytest.approx(0.2 + r, abs=1e-12)
  np.testing.assert_allclose(n, [0, 0, -1], atol=1e-12)
  # dist is in units of |vec|
  for s in (0.25, 4.0):
    _, xs, _ = _cast1(ray_ref.SPHERE, [r, 0, 0], [0, 0, 0], EYE, [0, 0, D], [0, 0, -s])
    assert xs == pytest.approx((D - r) / s, rel=1e-12)
  # looking away
  assert _cast1(ray_ref.SPHERE, [r, 0, 0], [0, 0, 0], EYE, [0, 0, D], [0, 0, 1])[:2] == (-1, -1.0)


def test_ref_plane_angle_back_side_and_rectangle():
  th = np.deg2rad(30.0)
  v = [np.sin(th), 0.0, -np.cos(th)]
  g, x, n = _cast1(ray_ref.PLANE, [0, 0, 1], [0, 0, 0], EYE, [0, 0, 2.0], v)
  assert g == 0 and x == pytest.approx(2.0 / np.cos(th), rel=1e-12)
  np.testing.assert_allclose(n, [0, 0, 1])
  assert _cast1(ray_ref.PLANE, [0, 0, 1], [0, 0, 0], EYE, [0, 0, -0.5], [0, 0, 1])[0] == -1  # from behind
  assert _cast1(ray_ref.PLANE, [0, 0, 1], [0, 0, 0], EYE, [0, 0, -0.5], v)[0] == -1  # behind, looking away
  # a rendered rectangle of half width 1: the hit at x = 2 tan(30 deg) = 1.155 falls outside it
  assert _cast1(ray_ref.PLANE, [1, 1, 1], [0, 0, 0], EYE, [0, 0, 2.0], v)[0] == -1
  # a tilted plane: the normal is the frame's z axis
  R = quat_mat([np.cos(0.2), np.sin(0.2), 0, 0])
  g, x, n = _cast1(ray_ref.PLANE, [0, 0, 1], [0, 0, 0], R, [0, 0, 2.0], [0, 0, -1])
  np.testing.assert_allclose(n, R[:, 2], atol=1e-12)
  assert x == pytest.approx(2.0, rel=1e-12)  # the plane passes through the origin


def test_ref_box_face_and_capsule_cap_against_side():
  g, x, n = _cast1(ray_ref.BOX, [0.5, 0.25, 0.3], [1, 0, 1], EYE, [1.1, 0.05, 3.0], [0, 0, -1])
  assert g == 0 and x == pytest.approx(3.0 - 1.3, abs=1e-12)
  np.testing.assert_allclose(n, [0, 0, 1])
  g, x, n = _cast1(ray_ref.BOX, [0.5, 0.25, 0.3], [1, 0, 1], EYE, [-2.0, 0.05, 1.1], [1, 0, 0])
  assert x == pytest.approx(2.5, abs=1e-12)
  np.testing.assert_allclose(n, [-1, 0, 0])
  # capsule along z, radius 0.25, half length 0.5: the side from the side, the cap from above
  g, x, n = _cast1(ray_ref.CAPSULE, [0.25, 0.5, 0], [0, 0, 0], EYE, [2.0, 0, 0.3], [-1, 0, 0])
  assert x == pytest.approx(1.75, abs=1e-12)
  np.testing.assert_allclose(n, [1, 0, 0], atol=1e-12)
  g, x, n = _cast1(ray_ref.CAPSULE, [0.25, 0.5, 0], [0, 0, 0], EYE, [0, 0, 2.0], [0, 0, -1])
  assert x == pytest.approx(2.0 - 0.75, abs=1e-12)
  np.testing.assert_allclose(n, [0, 0, 1], atol=1e-12)
  # off-axis on the cap: the hit lies on the cap's sphere and the normal points from the cap centre
  g, x, n = _cast1(ray_ref.CAPSULE, [0.25, 0.5, 0], [0, 0, 0], EYE, [0.1, 0, 2.0], [0, 0, -1])
  zhit = 0.5 + np.sqrt(0.25**2 - 0.1**2)
  assert x == pytest.approx(2.0 - zhit, abs=1e-12)
  np.testing.assert_allclose(n, np.array([0.1, 0, zhit - 0.5]) / 0.25, atol=1e-12)
  # cylinder of the same size: the flat end instead
  g, x, n = _cast1(ray_ref.CYLINDER, [0.25, 0.5, 0], [0, 0, 0], EYE, [0.1, 0, 2.0], [0, 0, -1])
  assert x == pytest.approx(1.5, abs=1e-12)
  np.testing.assert_allclose(n, [0, 0, 1])


def test_ref_tie_goes_to_lowest_id_and_filters():
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string("""<mujoco><asset><material name="ghost" rgba="1 1 1 0"/></asset><worldbody>
    <geom type="sphere" size=".2" pos="0 0 1" group="2"/><geom type="sphere" size=".2" pos="0 0 1"/>
    <geom type="sphere" size=".2" pos="0 0 2" material="ghost"/>
    <body pos="0 0 3"><freejoint/><geom type="sphere" size=".2"/></body></worldbody></mujoco>""")
  xpos, xmat = host_frames(mjm)
  pnt, vec = np.array([[0, 0, 5.0]]), np.array([[0, 0, -1.0]])
  g, x, _, _ = ray_ref.cast(mjm, xpos, xmat, pnt, vec)
  assert g[0] == 3 and x[0] == pytest.approx(1.8)
  g, x, _, _ = ray_ref.cast(mjm, xpos, xmat, pnt, vec, bodyexclude=np.array([1]))
  assert g[0] == 0 and x[0] == pytest.approx(3.8)  # the ghost is skipped, the coincident pair goes to id 0
  g, _, _, _ = ray_ref.cast(mjm, xpos, xmat, pnt, vec, geomgroup=(1, 1, 0, 1, 1, 1), bodyexclude=np.array([1]))
  assert g[0] == 1
  g, _, _, _ = ray_ref.cast(mjm, xpos, xmat, pnt, vec, flg_static=False)
  assert g[0] == 3
  g, x, n, _ = ray_ref.cast(mjm, xpos, xmat, pnt, vec, flg_static=False, bodyexclude=np.array([1]))
  assert g[0] == -1 and x[0] == -1 and not n.any()


def test_ref_all_types_scene_is_mostly_decisive():
  """The design check of the GPU tests, on the CPU: over 4096 aimed rays of the all-types scene at most 2 % are
  non-decisive, and every geom type is the first hit of many decisive rays."""
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  xpos, xmat = host_frames(mjm)
  pnt, vec = aimed_rays(xpos, 4096, seed=0)
  g, x, n, ok = ray_ref.cast(mjm, xpos, xmat, pnt, vec)
  assert 1.0 - ok.mean() <= 0.02, f"{1.0 - ok.mean():.4f} of the rays are non-decisive"
  hits = np.bincount(mjm.geom_type[g[ok & (g >= 0)]], minlength=8)
  assert (hits >= 10).all(), hits
  nn = np.linalg.norm(n[g >= 0], axis=1)
  np.testing.assert_allclose(nn, 1.0, atol=1e-9)  # unit normals on every hit
  assert not n[g < 0].any()


# ---- the public interface ---------------------------------------------------------------------------
def test_ray_and_rays_are_exported():
  import mujoco_warp_amd as mjw

  assert callable(mjw.ray) and callable(mjw.rays)


def test_rays_argument_validation():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  m = mjw.put_model(mjm, device="cpu")
  nworld, nray = 3, 5
  d = mjw.make_data(mjm, nworld=nworld, device="cpu", m=m)

  def args(**over):
    a = dict(pnt=torch.zeros(1, nray, 3), vec=torch.ones(1, nray, 3), geomgroup=None, flg_static=True,
             bodyexclude=torch.full((nray,), -1, dtype=torch.int32), dist=torch.zeros(nworld, nray),
             geomid=torch.zeros(nworld, nray, dtype=torch.int32), normal=torch.zeros(nworld, nray, 3))
    a.update(over)
    return a

  bad = [
    dict(pnt=torch.zeros(1, nray, 3, dtype=torch.float64)),  # wrong dtype
    dict(vec=torch.ones(1, nray, 3, dtype=torch.float16)),
    dict(pnt=torch.zeros(2, nray, 3)),  # nb neither 1 nor nworld
    dict(vec=torch.ones(2, nray, 3)),
    dict(bodyexclude=torch.full((nray + 1,), -1, dtype=torch.int32)),  # wrong length
    dict(bodyexclude=torch.full((nray,), -1, dtype=torch.int64)),
    dict(dist=torch.zeros(nworld, nray + 1)),
    dict(geomid=torch.zeros(nworld, nray)),  # float geomid
    dict(normal=torch.zeros(nworld, nray, 4)),
    dict(pnt=torch.zeros(1, nray, 6)[:, :, ::2]),  # not contiguous
    dict(geomgroup=(1, 0, 0)),
  ]
  for over in bad:
    with pytest.raises(ValueError):
      mjw.rays(m, d, **args(**over))
  with pytest.raises(NotImplementedError):
    mjw.rays(m, d, **args(), rc=object())
  with pytest.raises(NotImplementedError):
    mjw.ray(m, d, torch.zeros(1, 1, 3), torch.ones(1, 1, 3), rc=object())
  with pytest.raises(ValueError):
    mjw.ray(m, d, torch.zeros(1, 2, 3), torch.ones(1, 2, 3))  # ray takes one ray per world


def test_mjw_rays_reports_null_and_negative_arguments():
  """The C entry point refuses null pointers and nray < 0 through mjw_last_error, and takes nray == 0 as a no-op
  (no launch: this runs without a GPU)."""
  import ctypes

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib, mjcf
  from mujoco_warp_amd.io import cdata, cmodel
  from mujoco_warp_amd.ray import _ray_model

  mjm = mjcf.load_model_from_string(ALL_TYPES_XML)
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=2, device="cpu", m=m)
  L = _lib.lib()
  rm = _ray_model(m)
  assert rm.ngeom == 9 and rm.nmeshface == 4 and rm.geom_rgba_nb == 1
  tail = (None, 1, None, None, None, None, None)
  assert L.mjw_rays(cmodel(m), cdata(d), ctypes.byref(rm), None, 1, None, 1, 0, *tail) == 0
  assert L.mjw_rays(cmodel(m), cdata(d), ctypes.byref(rm), None, 1, None, 1, -1, *tail) != 0
  assert b"nray" in L.mjw_last_error()
  assert L.mjw_rays(cmodel(m), cdata(d), ctypes.byref(rm), None, 1, None, 1, 4, *tail) != 0
  assert b"null" in L.mjw_last_error()
  assert L.mjw_rays(cmodel(m), cdata(d), None, None, 1, None, 1, 4, *tail) != 0
  assert b"null" in L.mjw_last_error()
