// mjw_island.hip -- constraint islands (mujoco_warp/_src/island.py `island`; MuJoCo's mj_island): the connected
// components of the kinematic trees under the active constraint rows of each world.  One workgroup per world, one
// launch per call, dense and sparse / flex path alike; union-find over the trees, no tree x tree matrix.
//
//   1 init      parent[t] = t, con[t] = 0 (con: "some row touches tree t")
//   2 edges     rows r < n = min(nefc, njmax), lane = row: the typed rows (connect / weld, dof friction, joint limit,
//               geom-geom contact) are a handful of index loads; the generic rows scan J -- on the slot-major sparse
//               layout inline (consecutive lanes along r: the layout's fast direction), on the dense layout a wave takes
//               the generic rows of its 64 lanes (a ballot) one at a time, consecutive lanes along the row.  A row joins all trees of its set:
//               union by compare-and-swap, the larger root hooked under the smaller, so a component's root is its
//               smallest tree whatever order the lanes ran in.  One tree of the row is parked in efc_island[r].
//   3 number    every tree finds its root (parent[t] = root); a root's island id is its rank among the constrained
//               roots, counted with wave ballots and a running prefix over chunks of blockDim trees; tree_island, nisland
//   4 maps      dof_island[v] = tree_island[dof_treeid[v]], efc_island[r] = tree_island[parked tree], -1 past n
//
// parent / con live in LDS (8 ntree bytes, sized by the launch) up to ISLAND_LDS_TREES trees; above that the world's
// own tree_island and dof_island rows are the scratch (a tree has at least one dof, so nv >= ntree), read and
// written with relaxed agent-scope atomics.  Every id read from a row (efc_id, the contact's geoms, a column index)
// is checked against its range before it indexes anything: rows that njmax cut may hold stale words.
#include "mjw_common.h"

namespace mjw {
namespace isl {

constexpr int ISLAND_LDS_TREES = 2048;  // 16 KiB of LDS per world at most: ten worlds per CU still fit

template <bool LDS>
__device__ __forceinline__ int ld(const int* p) {
  if (LDS) return *(const volatile int*)p;
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void st(int* p, int v) {
  if (LDS) *(volatile int*)p = v;
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ int find_root(const int* parent, int x) {
  for (;;) {  // parent[x] <= x and links only ever decrease: the walk ends at the root
    const int p = ld<LDS>(parent + x);
    if (p == x) return x;
    x = p;
  }
}

// joins the components of trees a and b: the larger root is hooked under the smaller with a compare-and-swap that
// succeeds only while it still is a root; a lost race continues from the link the winner wrote
template <bool LDS>
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root<LDS>(parent, a);
    b = find_root<LDS>(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(parent + b, b, a);
    if (old == b) return;
    b = old;
  }
}

// the tree set of a typed row as (t0, t1), -1: none; returns true for a row that takes the generic (Jacobian) path
__device__ __forceinline__ bool row_trees(const mjw_model_t& m, const mjw_data_t& d, const mjw_island_t& is, long gr, int& t0, int& t1) {
  t0 = t1 = -1;
  const int type = d.efc_type[gr], id = d.efc_id[gr];
  int b0 = -1, b1 = -1;  // bodies of a two-body row
  if (type == CNSTR_EQUALITY) {
    if (id < 0 || id >= m.neq) return false;
    const int et = m.eq_type[id];
    if (et != EQ_CONNECT && et != EQ_WELD) return true;
    b0 = m.eq_obj1id[id];
    b1 = m.eq_obj2id[id];
    if (m.eq_objtype[id] == OBJ_SITE) {
      b0 = (b0 >= 0 && b0 < m.nsite) ? m.site_bodyid[b0] : -1;
      b1 = (b1 >= 0 && b1 < m.nsite) ? m.site_bodyid[b1] : -1;
    }
  } else if (type == CNSTR_FRICTION_DOF) {
    if (id >= 0 && id < m.nv) t0 = is.dof_treeid[id];
    return false;
  } else if (type == CNSTR_LIMIT_JOINT) {
    if (id >= 0 && id < m.njnt) {
      const int v = m.jnt_dofadr[id];
      if (v >= 0 && v < m.nv) t0 = is.dof_treeid[v];
    }
    return false;
  } else if (type == CNSTR_CONTACT_FRICTIONLESS || type == CNSTR_CONTACT_PYRAMIDAL || type == CNSTR_CONTACT_ELLIPTIC) {
    if (id < 0 || id >= d.naconmax) return false;
    const int g0 = d.contact_geom[2L * id], g1 = d.contact_geom[2L * id + 1];
    if (g0 < 0 || g1 < 0) return true;  // a flex side
    b0 = g0 < m.ngeom ? m.geom_bodyid[g0] : -1;
    b1 = g1 < m.ngeom ? m.geom_bodyid[g1] : -1;
  } else {
    return true;
  }
  if (b0 >= 0 && b0 < m.nbody) t0 = is.body_treeid[b0];
  if (b1 >= 0 && b1 < m.nbody) t1 = is.body_treeid[b1];
  return false;
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
  return x;
}

template <bool LDS>
__global__ void __launch_bounds__(256) island_kernel(const mjw_model_t m, const mjw_data_t d, const mjw_island_t is) {
  extern __shared__ int s_tree[];
  __shared__ int s_wcnt[4];
  const int wid = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwave = nt >> 6;
  const int ntree = is.ntree, nv = m.nv, njmax = d.njmax;
  const int n = njmax > 0 ? max(0, min(d.nefc[wid], njmax)) : 0;
  const long gr0 = (long)wid * njmax;
  int* tree_island = is.tree_island + (long)wid * ntree;
  int* dof_island = is.dof_island + (long)wid * nv;
  int* efc_island = is.efc_island + gr0;
  int* parent = LDS ? s_tree : tree_island;
  int* con = LDS ? s_tree + ntree : dof_island;

  // ---- 1: init
  for (int t = tid; t < ntree; t += nt) {
    st<LDS>(parent + t, t);
    st<LDS>(con + t, 0);
  }
  __syncthreads();

  // ---- 2: edges, lane = row; a wave then takes the generic rows of its own 64 lanes on the dense layout
  const bool sparse = m.is_sparse != 0;
  const long P = d.njmax_pad;
  const float* J = d.efc_J + (long)wid * P * m.nv_pad;  // dense layout
  for (int r0 = 0; r0 < n; r0 += nt) {  // uniform trip count: the ballot below needs every lane
    const int r = r0 + tid;
    bool scan = false;
    if (r < n) {
      int t0, t1;
      const bool generic = row_trees(m, d, is, gr0 + r, t0, t1);
      if (t0 < 0 || t0 >= ntree) t0 = -1;
      if (t1 < 0 || t1 >= ntree) t1 = -1;
      if (t0 < 0) { t0 = t1; t1 = -1; }
      if (generic && sparse) {
        const long jb = (long)wid * m.njrow * P + r;
        const int nnz = min(d.efc_J_rownnz[gr0 + r], m.njrow);
        int last = -1;
        for (int k = 0; k < nnz; k++) {
          const int c = d.efc_J_colind[jb + k * P];
          if (d.efc_J[jb + k * P] == 0.0f || c < 0 || c >= nv) continue;
          const int t = is.dof_treeid[c];
          if (t < 0 || t >= ntree || t == last) continue;
          last = t;
          st<LDS>(con + t, 1);
          if (t0 < 0) t0 = t;
          else if (t != t0) unite<LDS>(parent, t0, t);
        }
      } else if (!generic) {
        if (t0 >= 0) st<LDS>(con + t0, 1);
        if (t1 >= 0) {
          st<LDS>(con + t1, 1);
          if (t1 != t0) unite<LDS>(parent, t0, t1);
        }
      }
      scan = generic && !sparse;
      if (!scan) efc_island[r] = t0;
    }
    // the dense layout's generic rows: the whole wave on one row, lane = dof column
    unsigned long long todo = __ballot(scan);
    while (todo) {
      const int rr = r0 + (wave << 6) + __builtin_ctzll(todo);
      todo &= todo - 1;
      int first = ntree;
      for (int c0 = 0; c0 < nv; c0 += 64) {
        const int c = c0 + lane;
        int t = ntree;
        if (c < nv && J[(long)rr * m.nv_pad + c] != 0.0f) {
          t = is.dof_treeid[c];
          if (t < 0 || t >= ntree) t = ntree;
        }
        const int lo = wave_min(t);
        if (first == ntree) first = lo;
        if (t < ntree) {
          st<LDS>(con + t, 1);
          if (t != first) unite<LDS>(parent, first, t);
        }
      }
      if (lane == 0) efc_island[rr] = first < ntree ? first : -1;
    }
  }
  __syncthreads();

  // ---- 3: every tree to its root, then the roots' ranks
  for (int t = tid; t < ntree; t += nt) st<LDS>(parent + t, find_root<LDS>(parent, t));
  __syncthreads();
  int base = 0;
  for (int c0 = 0; c0 < ntree; c0 += nt) {
    const int t = c0 + tid;
    const bool root = t < ntree && ld<LDS>(parent + t) == t;
    const bool flag = root && ld<LDS>(con + t) != 0;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_wcnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < nwave; w++) {
      const int cw = s_wcnt[w];
      if (w < wave) before += cw;
      total += cw;
    }
    if (root) st<LDS>(con + t, flag ? base + before + __popcll(b & ((1ull << lane) - 1ull)) : -1);
    base += total;
    __syncthreads();
  }
  if (tid == 0) is.nisland[wid] = base;
  // parent[t] is read by t's own lane only from here on; con[root] was written above and is only read
  for (int t = tid; t < ntree; t += nt) {
    const int isl = ld<LDS>(con + ld<LDS>(parent + t));
    st<LDS>(parent + t, isl);
    if (LDS) tree_island[t] = isl;
  }
  __syncthreads();

  // ---- 4: maps (parent now holds tree_island; con, the dof_island row beyond the LDS cap, is dead)
  for (int v = tid; v < nv; v += nt) {
    const int t = is.dof_treeid[v];
    dof_island[v] = (t >= 0 && t < ntree) ? ld<LDS>(parent + t) : -1;
  }
  for (int r = tid; r < njmax; r += nt) {
    int isl = -1;
    if (r < n) {
      const int t = efc_island[r];
      if (t >= 0 && t < ntree) isl = ld<LDS>(parent + t);
    }
    efc_island[r] = isl;
  }
}

}  // namespace isl
}  // namespace mjw

extern "C" int mjw_sizeof_island(void) { return (int)sizeof(mjw_island_t); }
extern "C" int mjw_island_lds_trees(void) { return mjw::isl::ISLAND_LDS_TREES; }

extern "C" int mjw_island(const mjw_model_t* m, const mjw_data_t* d, const mjw_island_t* is, void* stream) {
  using namespace mjw;
  if (!m || !d || !is) return set_last_error(-1, "mjw_island: null model / data / island view");
  if (d->nworld <= 0) return 0;
  if (is->ntree != m->ntree) return set_last_error(-4, "mjw_island: ntree of the island view differs from the model's");
  if (!is->nisland) return set_last_error(-1, "mjw_island: null output array");
  if (m->ntree <= 0) {
    hipError_t e = hipMemsetAsync(is->nisland, 0, sizeof(int32_t) * (size_t)d->nworld, (hipStream_t)stream);
    return e != hipSuccess ? set_last_error((int)e, hipGetErrorString(e)) : 0;
  }
  if (!is->body_treeid || !is->dof_treeid || !is->tree_island || !is->dof_island || (d->njmax > 0 && !is->efc_island))
    return set_last_error(-1, "mjw_island: null island array");
  if (m->ntree > m->nv) return set_last_error(-4, "mjw_island: more trees than dofs");
  if (!d->nefc) return set_last_error(-1, "mjw_island: null data array");
  if (d->njmax > 0) {
    if (!d->efc_type || !d->efc_id || !d->efc_J) return set_last_error(-1, "mjw_island: null constraint array");
    if (d->naconmax > 0 && !d->contact_geom) return set_last_error(-1, "mjw_island: null contact array");
    if (m->is_sparse && (!d->efc_J_colind || !d->efc_J_rownnz)) return set_last_error(-1, "mjw_island: null sparse Jacobian index");
  }
  hipStream_t s = (hipStream_t)stream;
  const int big = max(max(d->njmax, m->ntree), m->nv);
  const int threads = big <= 128 ? 64 : 256;
  if (m->ntree <= isl::ISLAND_LDS_TREES)
    hipLaunchKernelGGL(isl::island_kernel<true>, dim3(d->nworld), dim3(threads), (size_t)m->ntree * 8, s, *m, *d, *is);
  else
    hipLaunchKernelGGL(isl::island_kernel<false>, dim3(d->nworld), dim3(threads), 0, s, *m, *d, *is);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error((int)e, hipGetErrorString(e));
  return 0;
}
