"""spd_inverse with the X = L^-1 substitution split over both wave halves (mjw_dense.h) against the retained
columns-in-lanes substitution (spd_inverse_ref, mjw_dense.hip), through mjw_selftest.

Every element of X gets the same multiply and the same FMAs in the same order in both forms, so the two
inverses must agree bit for bit, for each factor bound NB (32, 16, 28) and every matrix size up to it --
sizes 1..5, NB - 1 and NB are the edges of the four-column blocks.
"""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 96
# (NB, selftest id of spd_inverse, selftest id of spd_inverse_ref)
CASES = [(32, 1, 6), (16, 2, 7), (28, 5, 8)]


def _run(which, x):
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  from mujoco_warp_amd import _lib

  L = _lib.lib()
  n = x.shape[0]
  xin = torch.as_tensor(x, dtype=torch.float32, device="cuda").contiguous()
  out = torch.full((n * 1024,), float("nan"), dtype=torch.float32, device="cuda")
  rc = L.mjw_selftest(which, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, None)
  assert rc == 0, L.mjw_last_error()
  torch.cuda.synchronize()
  return out.cpu().numpy().reshape(n, 32, 32)


def _sizes(nb):
  """Matrix size of each of the N inputs: the block edges first, then every size 1..nb, cycling."""
  edges = [nb, 1, 2, 3, 4, 5, nb - 1, nb]  # entry 0 is the diagonal matrix (size nb)
  return edges + [1 + i % nb for i in range(N - len(edges))]


def _inputs(nb):
  rng = np.random.default_rng(100 + nb)
  sizes = _sizes(nb)
  assert len(sizes) == N and set(sizes) == set(range(1, nb + 1))
  M = np.tile(np.eye(32), (N, 1, 1))
  for i, k in enumerate(sizes):
    A = rng.normal(size=(k, k))
    M[i, :k, :k] = A @ A.T / k + np.eye(k) * 0.5
  M[0] = np.eye(32)
  M[0, :nb, :nb] = np.diag(np.arange(1, nb + 1, dtype=np.float64))
  return M.astype(np.float32)


@pytest.fixture(scope="module", params=CASES, ids=[f"nb{c[0]}" for c in CASES])
def case(request):
  nb, new_id, ref_id = request.param
  M = _inputs(nb)
  x = M.reshape(N, -1)
  return nb, M, _run(new_id, x), _run(ref_id, x)


def test_bitwise_equal_to_reference_substitution(case):
  nb, M, new, ref = case
  assert np.isfinite(ref).all()
  assert np.array_equal(new, ref), f"{int((new != ref).any(axis=(1, 2)).sum())} of {N} matrices differ"


def test_bitwise_symmetric(case):
  nb, M, new, ref = case
  assert np.array_equal(new, new.transpose(0, 2, 1))


def test_identity_past_factor_bound(case):
  nb, M, new, ref = case
  want = np.tile(np.eye(32, dtype=np.float32), (N, 1, 1))
  assert np.array_equal(new[:, nb:, :], want[:, nb:, :])
  assert np.array_equal(new[:, :, nb:], want[:, :, nb:])


def test_diagonal_matrix(case):
  nb, M, new, ref = case
  d = np.concatenate([np.arange(1, nb + 1, dtype=np.float64), np.ones(32 - nb)])
  np.testing.assert_allclose(np.diag(new[0]), 1.0 / d, rtol=1e-6)
  assert np.abs(new[0] - np.diag(np.diag(new[0]))).max() == 0.0


def test_against_numpy_inverse(case):
  nb, M, new, ref = case
  want = np.linalg.inv(M.astype(np.float64))
  err = np.abs(new - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
  assert err.max() < 1e-4, err.max()
