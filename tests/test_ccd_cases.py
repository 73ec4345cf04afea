"""tests/ccd_cases.py on the CPU: every case's predicate holds on the fp64 oracle's trace, every polytope route and EPA
exit the families are there for is reached, tracing changes no result, and the fp32 oracle builds -- put through the
acceptance rule in the device's place -- stay inside the cap budget, so that the caps of tests/test_gpu_ccd_edges.py are
conditions the device can meet and not measurements of it.

Budget: the ties of liborc32 and of liborc32f (each leaning on the other build for its ties) are at most half of the
family's tie cap, and their unmatched share is at most the unmatched cap.  Measured (profiles/ccd_edges.json): ties 0 .. 1.0 %
against caps of 2 % and 8 %, unmatched 0 .. 0.9 %; every family but `capacity` also keeps its unmatched share inside half
the cap.  In `capacity` that is not reachable: at the face array's last slots one fp32 build overflows (and reports no
contact) where the other and fp64 stop one face short, in about 1 % of the poses whatever the selection.
"""
import numpy as np
import pytest

from oracle import orc
from tests import ccd_cases as cc

FAMS = sorted(cc.FAMILIES)


@pytest.mark.parametrize("name", FAMS)
def test_predicates_hold_on_the_fp64_trace(name):
  bad, reach = cc.check_predicates(name)
  print(name, len(cc.family(name).recs), reach)
  assert not bad, bad[:5]
  assert sum(p is not None for p in cc.family(name).preds) > 0


def test_every_route_and_exit_is_reached():
  al = cc.reached(cc.references("aligned")["trace"])
  assert set(al["routes"]) >= {2, 3, 4, 23, 43}, al  # polytope2 / 3 / 4 and both fall-throughs
  assert al["dim_lt2"] > 0, al  # GJK's simplex is a point: ccd_raw returns the GJK answer
  tr = cc.references("capacity")["trace"]
  ids = cc.family("capacity").ids
  cap = cc.reached(tr)
  assert {cc.EXIT["converged"], cc.EXIT["iterations exhausted"], cc.EXIT["face array full"]} <= set(cap["exits"]), cap
  assert cap["peak_face_fill"] == 1.0 and cap["peak_horizon"] >= cc.HORIZON_MIN
  for it in cc.CAP_ITS:  # the last vertex slot at every iteration count
    assert any(c.startswith(f"it{it}-exhausted") for c in ids), it
    assert tr[[c.startswith(f"it{it}-") for c in ids], cc.T["nvert"]].max() == 5 + it
  for edge in ("full-1", "full", "overflow", "horizon"):
    assert any(f"-{edge}-" in c for c in ids), edge
  # what no input of the search reaches (profiles/ccd_edges.json has its size): the 24-edge horizon's overflow
  assert not any("-horizon-overflow-" in c for c in ids)
  exits = set()
  for name in FAMS:
    exits |= set(cc.reached(cc.references(name)["trace"])["exits"])
  assert exits >= {1, 2, 3, 5}, exits
  mb = cc.reached(cc.references("multibox")["trace"])
  assert set(mb["poly_np"]) >= {3, 4, 5, 6, 7, 8}, mb
  its = np.stack(cc.family("capacity").recs)[:, 34]
  assert set(its.astype(int)) == set(cc.CAP_ITS)  # one launch mixes every count


@pytest.mark.parametrize("name", FAMS)
def test_fp32_builds_stay_inside_the_cap_budget(name):
  ref = cc.references(name)
  fails = []
  for build, other in (("o32", "o32f"), ("o32f", "o32")):
    res = cc.classify(name, ref[build], [ref[other]])
    print(name, build, f"n {res['n']} pass {res['passed']:.4f} tie {res['tie']:.4f} unmatched {res['un']:.4f} worst dist {res['worst_dist']:.2e}")
    if res["tie"] > 0.5 * res["tie_cap"]:
      fails.append(f"{build}: ties {res['tie']:.4f} > half of {res['tie_cap']}")
    if res["un"] > (1.0 if name == "capacity" else 0.5) * res["un_cap"]:
      fails.append(f"{build}: unmatched {res['un']:.4f} > its share of {res['un_cap']}")
  assert not fails, fails


def test_fp64_oracle_passes_its_own_rule():
  for name in FAMS:
    res = cc.classify(name, cc.references(name)["o64"], [])
    assert res["passed"] == 1.0, name


def test_trace_changes_no_result():
  """The batch entry with and without the trace, and the single-pair entry with trace=True, agree bit for bit."""
  for name in ("types", "capacity", "multibox"):
    recs, mv = cc.family(name).arrays()
    for bits in (64, 32, "32f"):
      a = orc.kat_ccd_batch(recs, mv, real_bits=bits)
      b, _ = orc.kat_ccd_batch(recs, mv, real_bits=bits, trace=True)
      assert np.array_equal(a, b), (name, bits)
  recs, mv = cc.family("types").arrays()
  tr = cc.references("types")["trace"]
  for i in range(0, len(recs), 37):
    r = recs[i].astype(np.float64)
    args = ([int(r[0]), int(r[1])], [r[2:5], r[17:20]], [r[5:14], r[20:29]], [r[14:17], r[29:32]], r[32], r[33], int(r[34]), bool(r[35]),
            mv.astype(np.float64), (int(r[36]), int(r[38])), (int(r[37]), int(r[39])))
    plain = orc.kat_ccd(*args)
    traced = orc.kat_ccd(*args, trace=True)
    assert plain[0] == traced[0] and plain[1] == traced[1] and np.array_equal(plain[2], traced[2]) and np.array_equal(plain[3], traced[3])
    assert [traced[4][k] for k in cc.TRACE] == tr[i].tolist()
    assert orc.CCD_TRACE_FIELDS == cc.TRACE


def test_fp64_gjk_never_rescales_its_coordinates():
  """gjk scales barycentric coordinates that sum to more than 1e-4 off 1 back to sum 1 (not in the reference).  Over every
  family the fp64 build never takes that branch, so the fp64 oracle is still the reference's algorithm; the fp32 builds
  take it (that is the defect it answers)."""
  for bits in (64, 32, "32f"):
    orc.ccd_renorm_count(bits, reset=True)
  for name in FAMS:
    recs, mv = cc.family(name).arrays()
    for bits in (64, 32, "32f"):
      orc.kat_ccd_batch(recs, mv, real_bits=bits)
  assert orc.ccd_renorm_count(64) == 0
  assert orc.ccd_renorm_count(32) > 0 and orc.ccd_renorm_count("32f") > 0


def test_witness_bar_is_kept_where_the_witness_is_defined():
  """The witness bar is relaxed only where the fp64 oracle itself shows the witness (1) or the normal too (2) to jump under
  a micrometre nudge or a 2e-5 rad turn of geom2.  Generic poses keep it; exactly parallel faces lose it."""
  amb = {name: cc.references(name)["amb"] for name in FAMS}
  assert (amb["types"] == 0).mean() > 0.95 and (amb["scale"] == 0).mean() > 0.95
  assert (amb["aligned"] == 0).sum() > 1000 and (amb["meshverts"] == 0).sum() > 300
  ids = cc.family("aligned").ids
  face = [i for i, c in enumerate(ids) if c.startswith("box-box-face-yaw0-d0.004")]
  assert face and (amb["aligned"][face] >= 1).all()  # a face on a face: a whole polygon of closest points
  support = cc.support_cases()
  assert len(support[0]) > 700


def test_box_points_check_sees_a_point_off_the_face():
  """box_points_outside on made-up results: the centre of the upper box's lower face is inside both faces of the
  octagon poses; moved half a metre along x it is not."""
  fam = cc.family("multibox")
  recs, _ = fam.arrays()
  o = cc.references("multibox")["o64"]
  got = np.zeros((len(recs), cc.OUT_PTS))
  got[:, :8] = o
  got[:, 0] = 0
  sel = [c for c, cid in enumerate(fam.ids) if cid.startswith("poly8") and cid.endswith("t0.0")]
  for c in sel:
    r = recs[c].astype(np.float64)
    p = r[17:20] - r[20:29].reshape(3, 3) @ np.array([0, 0, r[31]])
    got[c, 0], got[c, 8:11], got[c, 20:23] = 1, p, p
  assert len(sel) >= 6 and not cc.box_points_outside(recs, got)
  got[sel[1], 8] += 0.5
  assert cc.box_points_outside(recs, got) == [(sel[1], 0)]


def test_meshes_are_what_the_families_say():
  assert len(cc.lattice_cube()) == 125 and len(cc.prism(48)) == 96 and len(cc.fib_sphere(129)) == 129
  v = cc.duplicated(cc.lattice_cube(), 1)
  assert len(v) == 250 and len(np.unique(v, axis=0)) == 125
  fam = cc.family("meshverts")
  assert {n for _, n in fam.pool.key.values()} >= {4, 63, 64, 65, 127, 128, 129, 200}


# ---- host: opt.ccd_iterations at the upper edge the workspace layouts support ------------------------------------------
def _pair_model(kind, it, sparse):
  from mujoco_warp_amd import mjcf

  geom = {"ellipsoid": '<geom type="ellipsoid" size=".14 .09 .06"/>', "box": '<geom type="box" size=".1 .07 .05"/>'}[kind]
  mjm = mjcf.load_model_from_string(f"""<mujoco><worldbody><body><freejoint/>{geom}</body>
  <body pos="0.15 0 0"><freejoint/>{geom}</body></worldbody></mujoco>""")
  mjm.opt.ccd_iterations = it
  mjm.opt.jacobian = 1 if sparse else 0
  return mjm


@pytest.mark.parametrize("sparse", [False, True])
def test_put_model_refuses_a_ccd_workspace_past_the_lds(sparse):
  """The pre-pass kernels' LDS is ccd_layout(opt.ccd_iterations) (+ 64 words): 64 KB on the sparse path, 160 KiB on the
  dense one.  put_model takes the largest count that fits and refuses the next.  On the sparse path that is the whole
  condition.  On the dense path the pre-pass kernel's LDS is the whole per-world layout, which depends on njmax (known
  only at make_data): put_model refuses what can never fit, and the launcher refuses the rest by name before it
  launches anything ("the convex pre-pass's per-world LDS (opt.ccd_iterations) exceeds 160 KiB", an error return, as for
  every other layout that outgrows 160 KiB).  EPA runs at most 1000 iterations (5 + 1000 polytope vertices), so the 10-bit vertex ids of a face word hold at every accepted count."""
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import io

  limit = (64 if sparse else 160) * 1024
  edge = max(it for it in range(1, 2000) if 4 * (io._ccd_words(it) + 64) <= limit)
  assert 4 * (io._ccd_words(edge + 1) + 64) > limit
  assert edge == (482 if sparse else 1226)  # 33 words per iteration + 398, + 64
  m = mjw.put_model(_pair_model("ellipsoid", edge, sparse), device="cpu")
  assert m.ccd_epa_iterations == edge and bool(m.is_sparse) == sparse
  with pytest.raises(NotImplementedError, match="ccd_iterations"):
    mjw.put_model(_pair_model("ellipsoid", edge + 1, sparse), device="cpu")
  # box-box alone runs EPA at 16 iterations whatever the option says
  assert mjw.put_model(_pair_model("box", 5000, sparse), device="cpu").ccd_epa_iterations == 16
  assert 5 + 1000 < 1 << 10


def test_ccd_words_restates_the_device_layout():
  """io._ccd_words against ccd_layout (csrc/mjw_ccd.h) written out term by term."""
  from mujoco_warp_amd import io

  for it, npoly, ndeg in ((2, 4, 3), (16, 4, 3), (35, 4, 3), (64, 12, 9), (482, 4, 3)):
    cv, cf, nclip = 10 + 2 * it, 6 + 5 * it, max(2 * npoly, 16)
    want = (cv * 3 + cv) + (cf + cf * 3 + cf) + 24 + (36 + 8 + 4) + (40 + 32) + (12 + 12) + (6 * ndeg + 2 * ndeg + 3 * ndeg) \
        + (3 * npoly * 3 + npoly) + 2 * nclip * 3
    assert io._ccd_words(it, npoly, ndeg) == want
