"""The contact ladder (tests/contact_cases.py) on the CPU oracle: every case yields the contact and survivor counts
its construction states, inside the bands that make fp32 and fp64 agree; the straddles and the njmax / pool cuts
fall where the case says; and the checker rejects a permuted contact, a shifted row address and off-by-one
counters.  No GPU."""

import copy

import numpy as np
import pytest

from tests import contact_cases as cc

BAND = 1e-3  # a contact penetrates by at least this, a near shape / bounding sphere is this far from deciding otherwise
CLEAR = 0.5  # a raised geom's bounding sphere is this far from its partner

_CACHE = {}


def _case(case):
  """(host model, derived fields, fp64 oracle, fp32 oracle) of a case, computed once."""
  if case.id not in _CACHE:
    from mujoco_warp_amd import io

    mjm = case.model()
    _CACHE[case.id] = (mjm, io.derive_model_fields(mjm), case.oracle(mjm), case.oracle(mjm, real_bits=32))
  return _CACHE[case.id]


def _lowest(kind, pos, mat):
  """Height of the lowest point of a capsule / box geom at pose (pos, mat)."""
  R = mat.reshape(3, 3)
  if kind == "C":
    return pos[2] - abs(R[2, 2]) * cc.CAP_H - cc.CAP_R
  half = {"F": cc.FLAT, "T": cc.TILT, "B": cc.BOXB}[kind]
  return pos[2] - float(np.abs(R[2]) @ np.array(half))


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_case_construction(case):
  mjm, f, o64, o32 = _case(case)
  assert f["nxn"] == case.nxn == len(case.geoms())
  assert (f["nxn_box"] > 0) == case.box and f["nxn_ccd"] == int(case.ccd)
  assert mjm.nv == case.nv
  gtype = np.asarray(mjm.geom_type)
  rb = np.asarray(mjm.geom_rbound)
  for od in (o64, o32):
    assert [int(x) for x in od.ncon[:, 0]] == case.contacts()
    assert [int(x) for x in od.ncollision[:, 0]] == case.survivors()
    for w, poses in enumerate(case.worlds):
      want = case.contact_list(poses)
      n = min(len(want), od.nconmax)
      geoms = od.con_geom[w].reshape(-1, 2)[:n]
      order = [g for g, b, k in case.geoms() if k != "B"] + [g for g, b, k in case.geoms() if k == "B"]
      assert [int(g[1]) for g in geoms] == [order[p] for p, _, _, _ in want][:n]  # pair order
      assert (od.con_dist[w, :n] <= -BAND).all(), od.con_dist[w, :n].max()
      nl, rows = case.rows(poses)
      assert int(od.nl[w, 0]) == nl and int(od.nefc[w, 0]) == nl + sum(rows[:n])
  # the bands, on the fp64 oracle's geom frames
  xpos, xmat = o64.geom_xpos.reshape(case.nworld, -1, 3), o64.geom_xmat.reshape(case.nworld, -1, 9)
  statics = [g for g in range(1, mjm.ngeom) if gtype[g] == 6 and mjm.geom_bodyid[g] == 0]
  for w, poses in enumerate(case.worlds):
    for g, b, k in case.geoms():
      pose = poses.get(b, "up")
      if k == "B":
        gap = min(np.linalg.norm(xpos[w, g] - xpos[w, s]) - rb[g] - rb[s] for s in statics)
        assert (gap >= CLEAR) if pose == "up" else (gap <= -BAND), (w, g, pose, gap)
        continue
      reach = xpos[w, g, 2] - rb[g]  # the bounding sphere against the plane
      if pose == "up":
        assert reach >= CLEAR, (w, g, reach)
      else:
        assert reach <= -BAND, (w, g, pose, reach)
      if pose == "near":
        assert k in "CFT" and _lowest(k, xpos[w, g], xmat[w, g]) >= BAND, (w, g, k)


def _expectations():
  return [(c, e) for c in cc.CASES for e in c.expect]


@pytest.mark.parametrize("case,expect", _expectations(), ids=[f"{c.id}-{'-'.join(map(str, e))}" for c, e in _expectations()])
def test_case_edges_fall_where_stated(case, expect):
  mjm, f, od, _ = _case(case)
  gtype = np.asarray(mjm.geom_type)
  C = case.cmax
  if expect[0] == "straddle":
    _, w, first, n = expect
    geoms = [tuple(g) for g in od.con_geom[w].reshape(-1, 2)[:int(od.ncon[w, 0])]]
    run = geoms[first:first + n]
    assert len(run) == n and len(set(run)) == 1, run
    assert geoms[first - 1] != run[0] and (first + n == len(geoms) or geoms[first + n] != run[0])
    kinds = {"C": 3, "F": 6, "B": 6}
    kind = next(k for g, b, k in case.geoms() if g == run[0][1])
    assert gtype[run[0][1]] == kinds[kind] and cc.NCON[kind] == n
    assert (gtype[run[0][0]] == 6) == (kind == "B")  # the pre-pass pair is box-box
    last = first + n - 1  # the stated positions: the last contact at C-1 .. C+2, the first at C, the even split over 2C
    assert last in (C - 1, C, C + 1, C + 2) or first == C or first == 2 * C - n // 2, (first, n, C)
    return
  if expect[0] == "full":
    assert int(od.nefc[expect[1], 0]) == case.njmax
    return
  if expect[0] == "pool":
    assert case.nworld == 1 and int(od.ncon[0, 0]) > od.nconmax == case.naconmax == expect[1]
    return
  _, w, kind = expect
  ncon, nj = int(od.ncon[w, 0]), case.njmax
  assert int(od.nefc[w, 0]) > nj
  nl, rows = case.rows(case.worlds[w])
  adr = od.con_efc_address[w].reshape(-1, 10)[:ncon]
  kept = [int((adr[j, :rows[j]] >= 0).sum()) for j in range(ncon)]
  partial = [j for j in range(ncon) if 0 < kept[j] < rows[j]]
  whole = [j for j in range(ncon) if kept[j] == rows[j]]
  assert all((adr[j, :kept[j]] == np.arange(kept[j]) + nl + sum(rows[:j])).all() for j in range(ncon))
  if kind == "limits":
    assert int(od.nl[w, 0]) > nj and (adr == -1).all()
  elif kind == "after":
    assert not partial and whole and adr[whole[-1], rows[whole[-1]] - 1] == nj - 1 and whole[-1] + 1 < ncon and rows[whole[-1]] > 1
  elif kind == "pyramid":
    assert len(partial) == 1 and rows[partial[0]] > 1 and od.con_dim[w, partial[0]] > 1
  elif kind == "round2":
    assert len(partial) == 1 and partial[0] >= C and rows[partial[0]] > 1
  elif kind == "round2-after":
    assert not partial and whole[-1] >= C and adr[whole[-1], rows[whole[-1]] - 1] == nj - 1 and whole[-1] + 1 < ncon
  else:
    raise AssertionError(kind)


CHECKED = ("ladder-direct-box", "straddle-direct-F", "straddle-direct-B", "cut-direct-pyramid", "cut-generic-round2", "pool-direct-box-16",
           "counters-direct-box-adjacent", "passes-generic-nxn129", "cut-direct-elliptic")


def _view(case, interleave=True):
  mjm, f, od, _ = _case(case)
  naconmax = case.naconmax if case.naconmax is not None else None
  return cc.oracle_view(od, mjm.nv, f["nmaxpyramid"], case.survivors(), naconmax=naconmax, interleave=interleave), od, mjm


def _check(case, view, od, mjm):
  cc.check(view, od, case.survivors(), mjm.nv, geom_type=np.asarray(mjm.geom_type))


@pytest.mark.parametrize("cid", CHECKED)
def test_checker_accepts_the_oracle_and_rejects_edits(cid):
  case = next(c for c in cc.CASES if c.id == cid)
  for interleave in (False, True):
    view, od, mjm = _view(case, interleave)
    _check(case, view, od, mjm)
  view, od, mjm = _view(case)
  con = view["con"]
  w = int(np.argmax(case.contacts()))
  sel = np.nonzero(con["worldid"] == w)[0]
  assert len(sel) >= 2

  def edited(fn):
    v = copy.deepcopy(view)
    fn(v)
    with pytest.raises(AssertionError):
      _check(case, v, od, mjm)

  def swap(v):  # two neighbouring contacts of a world change places
    a, b = sel[len(sel) // 2 - 1], sel[len(sel) // 2]
    for k in v["con"]:
      if k != "efc_address":
        v["con"][k][[a, b]] = v["con"][k][[b, a]]

  def shift(v):
    adr = v["con"]["efc_address"]
    rows = np.nonzero(adr[sel, 0] >= 0)[0]
    adr[sel[rows[-1]], 0] += 1

  def drop_address(v):
    adr = v["con"]["efc_address"]
    rows = np.nonzero(adr[sel, 0] >= 0)[0]
    adr[sel[rows[-1]], 0] = -1

  edited(swap)
  if (con["efc_address"][sel, 0] >= 0).any():
    edited(shift)
    edited(drop_address)
  for key, step in (("ncollision", 1), ("ncollision", -1), ("nacon", 1)):
    edited(lambda v, key=key, step=step: v.__setitem__(key, v[key] + step))
  edited(lambda v: v["counts"]["nefc"].__setitem__(w, v["counts"]["nefc"][w] + 1))
  edited(lambda v: v["con"]["dist"].__setitem__(sel[0], v["con"]["dist"][sel[0]] + 1e-5))
  edited(lambda v: v["con"]["worldid"].__setitem__(sel[-1], (w + 1) % max(case.nworld, 2)))
  n = min(int(od.nefc[w, 0]), case.njmax)
  if n:
    edited(lambda v: v["J"][w].__setitem__((n - 1, slice(None)), v["J"][w][n - 1] * (1 + 1e-4)))
    edited(lambda v: v["efc"]["aref"].__setitem__((w, n - 1), v["efc"]["aref"][w, n - 1] + 1e-4 * np.abs(od.efc_aref[w, :n]).max()))
    edited(lambda v: v["efc"]["id"].__setitem__((w, n - 1), v["efc"]["id"][w, n - 1] + 1))


def test_shared_pool_checker():
  case = next(c for c in cc.CASES if c.id == "pool-direct-shared")
  mjm, f, od, _ = _case(case)
  view = cc.oracle_view(od, mjm.nv, f["nmaxpyramid"], case.survivors(), naconmax=case.naconmax, interleave=True)
  # the oracle keeps every world's contacts: cut its rows to the stored ones, as the device does
  kept = {w: set(np.nonzero(view["con"]["worldid"] == w)[0]) for w in range(case.nworld)}
  for w in range(case.nworld):
    ids = view["efc"]["id"][w, :int(od.nefc[w, 0])]
    keep = [r for r, i in enumerate(ids) if i >= 0]
    for k in view["efc"]:
      view["efc"][k][w, :len(keep)] = view["efc"][k][w, keep]
    view["counts"]["nefc"][w] = len(keep)
    assert len(keep) == len(kept[w])
  cc.check_shared_pool(view, od, case.survivors())
  bad = copy.deepcopy(view)
  bad["nacon"] -= 1
  with pytest.raises(AssertionError):
    cc.check_shared_pool(bad, od, case.survivors())
  bad = copy.deepcopy(view)
  w = 0
  bad["efc"]["id"][w, 0] = case.naconmax
  with pytest.raises(AssertionError):
    cc.check_shared_pool(bad, od, case.survivors())


def test_paths_and_edges_are_all_present():
  ids = [c.id for c in cc.CASES]
  for path in ("direct", "fused", "generic"):
    assert f"ladder-{path}-prim" in ids and f"straddle-{path}-C" in ids and f"pool-{path}-shared" in ids
    for nxn in (63, 64, 65, 128, 129):
      assert f"passes-{path}-nxn{nxn}" in ids
    for tag in ("after", "pyramid", "limits", "round2"):
      assert f"cut-{path}-{tag}" in ids
  assert "cut-sparse-elliptic" in ids and "cut-sparse-limits" in ids
  for path in ("direct", "generic"):
    assert f"ladder-{path}-box" in ids and f"straddle-{path}-F" in ids and f"straddle-{path}-B" in ids and f"cut-{path}-elliptic" in ids
  for nxn in (63, 64, 65, 255, 256, 257):
    assert f"passes-sparse-nxn{nxn}" in ids
  assert "ladder-sparse-prim" in ids and "ladder-sparse-box" in ids
  for c in cc.CASES:
    C = c.cmax
    if c.id.startswith("ladder-") and c.path != "sparse":
      assert c.contacts() == [0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1]
    if c.id.startswith("ladder-sparse"):
      assert c.contacts() == [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("case", cc.POOL_CASES, ids=[c.id for c in cc.POOL_CASES])
def test_pool_case_oracle_of_the_edited_set(case):
  """The state whose oracle stands for the edited pool: the two cleared contacts are gone, the edited one is DEEP, and
  every other contact keeps its rows bit for bit (a contact's rows depend on its own body only)."""
  mjm = case.model()
  o1 = case.oracle(mjm)
  o2 = case.oracle(mjm, states=case.states(mjm, case.edited_worlds()))
  C, nv = case.cmax, mjm.nv
  assert any(case.edited(w) for w in range(case.nworld)) and [int(x) for x in o1.ncon[:, 0]] == case.contacts()
  assert [int(x) for x in o1.ncollision[:, 0]] == case.survivors()
  for w, cmap in enumerate(case.contact_map()):
    n1 = int(o1.ncon[w, 0])
    assert len(cmap) == n1 and int(o2.ncon[w, 0]) == n1 - (2 if case.edited(w) else 0)
    assert [i for i, j in enumerate(cmap) if j is None] == ([C - 1, C] if case.edited(w) else [])
    for i, j in enumerate(cmap):
      if j is None:
        continue
      assert tuple(o1.con_geom[w, 2 * i:2 * i + 2]) == tuple(o2.con_geom[w, 2 * j:2 * j + 2])
      r1, r2 = int(o1.con_efc_address[w, 10 * i]), int(o2.con_efc_address[w, 10 * j])
      assert (r1 < 0) == (r2 < 0) or case.edited(w)
      if case.edited(w) and i == case.EDIT:
        assert abs(o2.con_dist[w, j] + cc.DEEP) < 1e-12 and abs(o1.con_dist[w, i] + cc.PEN) < 1e-12
        assert np.array_equal(o1.efc_J[w].reshape(-1, nv)[r1], o2.efc_J[w].reshape(-1, nv)[r2])
      elif r1 >= 0 and r2 >= 0:
        for k in ("efc_D", "efc_aref", "efc_pos", "efc_vel"):
          assert getattr(o1, k)[w, r1] == getattr(o2, k)[w, r2], (w, i, k)
        assert np.array_equal(o1.efc_J[w].reshape(-1, nv)[r1], o2.efc_J[w].reshape(-1, nv)[r2])
  if case.njmax < max(case.contacts()):
    assert any(int(o2.nefc[w, 0]) > case.njmax for w in range(case.nworld))  # the rebuilt rows are cut at njmax too
