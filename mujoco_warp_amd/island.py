"""Constraint islands (mirror mujoco_warp/_src/island.py).

`island(m, d)` finds which kinematic trees the active constraint rows of each world couple: one HIP launch
(`mjw_island`: csrc/mjw_island.hip, dense and sparse / flex path alike), one workgroup per world, union-find over the
trees.  It reads the rows the last position stage left (`fwd_position`, `forward`, `step`) and writes `d.nisland`,
`d.tree_island`, `d.dof_island` and `d.efc_island`, nothing else; `step` and `forward` do not call it.

Two deviations from the reference: no (ntree, ntree) adjacency matrix and no allocation per call (flex models have
thousands of trees per world), and the islands are the connected components of the undirected tree graph, which the
reference's upper-triangle edges of Jacobian-scanned rows can split.
"""

from __future__ import annotations

from . import _lib
from .forward import _stream
from .io import cdata, cmodel
from .types import Data, Model

# trees per world up to which the launch keeps its union-find in LDS (csrc/mjw_island.hip ISLAND_LDS_TREES; above it
# the world's own tree_island / dof_island rows are the scratch, same results); tests sit on both sides of it
ISLAND_LDS_TREES = 2048


def _cisland(m: Model, d: Data) -> _lib.CIsland:
  """Builds (and caches on `d`) the C view of the model's tree ids and the Data's island outputs."""
  tensors = (m.body_treeid, m.dof_treeid, d.nisland, d.tree_island, d.dof_island, d.efc_island)
  cache = getattr(d, "_cisland_cache", None)
  if cache is not None and cache[1] == m.ntree and all(a is b for a, b in zip(cache[2], tensors)):
    return cache[0]
  c = _lib.CIsland()
  c.ntree = int(m.ntree)
  for name, t in zip(("body_treeid", "dof_treeid", "nisland", "tree_island", "dof_island", "efc_island"), tensors):
    if not t.is_contiguous():
      raise TypeError(f"island field {name} must be contiguous")
    setattr(c, name, t.data_ptr())
  d._cisland_cache = (c, m.ntree, tensors)
  return c


def island(m: Model, d: Data):
  """Constraint islands of every world (island.py:246-265) from the rows r < min(nefc, njmax) in `d`.

  d.nisland (nworld,): islands per world.  d.tree_island (nworld, ntree): island of each tree, -1 for a tree no row
  touches.  d.dof_island (nworld, nv) = tree_island[dof_treeid].  d.efc_island (nworld, njmax): island of each row's
  trees, -1 for a row without trees and for every row at or past min(nefc, njmax).  Islands are numbered in ascending
  order of their smallest tree.  Allocates nothing, so it can be captured in a graph after a `step`."""
  if m.ntree == 0:
    d.nisland.zero_()
    return
  _lib.check(_lib.lib().mjw_island(cmodel(m), cdata(d), _cisland(m, d), _stream(d)), "mjw_island")
