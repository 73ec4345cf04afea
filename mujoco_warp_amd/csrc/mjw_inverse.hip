// mjw_inverse.hip -- inverse dynamics at the caller's acceleration (mujoco_warp/_src/inverse.py `inverse`, its
// constraint and combine steps; solver.py init_context(grad=False) + update_constraint :2154-2219, cone zones
// :1886-1942), dense path: one wavefront per world, one launch per call.
//
//   pass 1  Jaref = J qacc - aref      lane = dof column (coalesced 4 nv_pad byte row reads), one DPP wave sum per
//                                      row; two rows share a 64-lane load when nv_pad <= 32 (one half-sum each).
//                                      Lane j keeps the sum of row 64 c + j, so aref and the store are lane = row.
//   row law force, state               lane = row; the lane of an elliptic contact's first row does all its rows
//   pass 2  qfrc_constraint = J' f     lane = dof, rows in order (a fixed summation order); rows whose force is
//                                      zero are skipped (the force is wave-uniform, so is the test)
//   Ma = M qacc                        lane = dof, down the columns of the symmetric dense qM (nv_pad x nv_pad, both
//                                      triangles stored: the layout support.mul_m and the dense kernel's staging read)
//   qfrc_inverse = qfrc_bias + Ma - qfrc_passive - qfrc_constraint
//
// Jaref and then the forces of the rows live in LDS (4 njmax bytes, sized by the launch) up to INV_LDS_ROWS rows;
// above that the world's own efc_force rows are the scratch.  Nothing here depends on the fused kernels' LDS layout
// or on njmax <= 64.  d.qacc is only read.
#include "mjw_common.h"

namespace mjw {
namespace inv {

constexpr int INV_LDS_ROWS = 8192;  // 32 KiB of LDS per world at most: five worlds per CU still fit

__global__ void __launch_bounds__(64) inverse_kernel(const mjw_model_t m, const mjw_data_t d, int rows_in_lds) {
  extern __shared__ float s_rows[];
  const int wid = blockIdx.x, lane = threadIdx.x;
  const int nv = m.nv, np = m.nv_pad, njmax = d.njmax;
  const long gv = (long)wid * nv;
  const bool inl = lane < nv;
  const float qa = inl ? d.qacc[gv + lane] : 0.0f;
  const bool rows = njmax > 0 && !(m.opt_disableflags & DSBL_CONSTRAINT);
  const int n = rows ? min(d.nefc[wid], njmax) : 0;
  const long gr0 = (long)wid * njmax;
  const float* J = d.efc_J + (long)wid * d.njmax_pad * np;
  float* jf = rows_in_lds ? s_rows : d.efc_force + gr0;  // Jaref, then the force, of rows < n

  // ---- pass 1: Jaref
  const bool pair = np <= 32;
  const int half = lane >> 5, col = pair ? (lane & 31) : lane;
  const float qc = col < nv ? d.qacc[gv + col] : 0.0f;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int cn = min(64, n - c0);
    float mine = 0.0f;
    // four loads in flight before the first reduction (the wave sums are convergent, so the unroll is by hand)
    if (pair) {
      for (int j = 0; j < cn; j += 8) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int r = c0 + j + 2 * k + half;
          v[k] = (r < n && col < nv) ? J[(long)r * np + col] * qc : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          float lo, hi;
          dsum_halves(v[k], lo, hi);
          if (lane == j + 2 * k) mine = lo;
          if (lane == j + 2 * k + 1) mine = hi;
        }
      }
    } else {
      for (int j = 0; j < cn; j += 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int r = c0 + j + k;
          v[k] = (r < n && inl) ? J[(long)r * np + lane] * qa : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float sum = dsum(v[k]);
          if (lane == j + k) mine = sum;
        }
      }
    }
    const int r = c0 + lane;
    if (r < n) jf[r] = mine - d.efc_aref[gr0 + r];
  }
  __syncthreads();

  // ---- the row law
  const int ne = d.ne[wid], nf = d.nf[wid];
  const bool ell = m.opt_cone == CONE_ELLIPTIC;
  const float* Dw = d.efc_D + (long)wid * d.njmax_pad;
  int* state = d.efc_state + (long)wid * d.njmax_pad;
  for (int r = lane; r < n; r += 64) {
    const float D = Dw[r], jar = jf[r];
    float f;
    int st;
    if (r < ne) {
      f = -D * jar; st = STATE_QUADRATIC;
    } else if (r < ne + nf) {
      const float fl = d.efc_frictionloss[gr0 + r], rf = safe_div(fl, D);
      if (jar <= -rf) { f = fl; st = STATE_LINEARNEG; }
      else if (jar >= rf) { f = -fl; st = STATE_LINEARPOS; }
      else { f = -D * jar; st = STATE_QUADRATIC; }
    } else if (ell && d.efc_type[gr0 + r] == CNSTR_CONTACT_ELLIPTIC) {
      // the contact's rows r0 .. r0 + dim - 1 by the lane of its first row (nobody else touches them)
      const int con = d.efc_id[gr0 + r];
      const bool known = con >= 0 && con < d.naconmax;
      const int r0 = known ? d.contact_efc_address[(long)con * m.nmaxpyramid] : r;
      if (r0 != r) continue;
      const int dim = known ? max(1, min(d.contact_dim[con], 6)) : 1;
      if (!known || r0 + dim > n) {  // cut by njmax: contributes nothing
        for (int j = 0; j < dim && r0 + j < n; j++) { jf[r0 + j] = 0.0f; state[r0 + j] = STATE_SATISFIED; }
        continue;
      }
      const float* fr = d.contact_friction + 5L * con;
      const float mu = fr[0] * MR(opt_impratio_invsqrt)[0];
      const float N = jar * mu;
      float u[6], TT = 0.0f;
      for (int j = 1; j < dim; j++) {
        u[j] = jf[r0 + j] * fr[j - 1];
        TT += u[j] * u[j];
      }
      const float T = TT <= 0.0f ? 0.0f : sqrtf(TT);
      if (N >= mu * T || (T <= 0.0f && N >= 0.0f)) {
        for (int j = 0; j < dim; j++) { jf[r0 + j] = 0.0f; state[r0 + j] = STATE_SATISFIED; }
      } else if (mu * N + T <= 0.0f || (T <= 0.0f && N < 0.0f)) {
        for (int j = 0; j < dim; j++) { jf[r0 + j] = -Dw[r0 + j] * jf[r0 + j]; state[r0 + j] = STATE_QUADRATIC; }
      } else {
        const float dm = safe_div(D, mu * mu * (1.0f + mu * mu));
        const float f0 = -dm * (N - mu * T) * mu;
        const float ft = -safe_div(f0, T);
        jf[r0] = f0; state[r0] = STATE_CONE;
        for (int j = 1; j < dim; j++) { jf[r0 + j] = ft * (u[j] * fr[j - 1]); state[r0 + j] = STATE_CONE; }
      }
      continue;
    } else {
      if (jar >= 0.0f) { f = 0.0f; st = STATE_SATISFIED; }
      else { f = -D * jar; st = STATE_QUADRATIC; }
    }
    jf[r] = f;
    state[r] = st;
  }
  __syncthreads();
  if (rows_in_lds)
    for (int r = lane; r < n; r += 64) d.efc_force[gr0 + r] = jf[r];

  // ---- pass 2: qfrc_constraint = J' f
  float qc_sum = 0.0f;
  {
    const float* Jl = J + (inl ? lane : 0);
    int r = 0;
    for (; r + 4 <= n; r += 4) {
      const float f0 = jf[r], f1 = jf[r + 1], f2 = jf[r + 2], f3 = jf[r + 3];
      if (f0 == 0.0f && f1 == 0.0f && f2 == 0.0f && f3 == 0.0f) continue;
      const float j0 = f0 != 0.0f ? Jl[(long)r * np] : 0.0f;
      const float j1 = f1 != 0.0f ? Jl[(long)(r + 1) * np] : 0.0f;
      const float j2 = f2 != 0.0f ? Jl[(long)(r + 2) * np] : 0.0f;
      const float j3 = f3 != 0.0f ? Jl[(long)(r + 3) * np] : 0.0f;
      qc_sum += j0 * f0;
      qc_sum += j1 * f1;
      qc_sum += j2 * f2;
      qc_sum += j3 * f3;
    }
    for (; r < n; r++) {
      const float f = jf[r];
      if (f != 0.0f) qc_sum += Jl[(long)r * np] * f;
    }
  }

  // ---- Ma = M qacc and the combine
  float ma = 0.0f;
  const float* Ml = d.qM + (long)wid * np * np + (inl ? lane : 0);
  for (int j = 0; j < nv; j += 4) {
    float mv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) mv[k] = j + k < nv ? Ml[(long)(j + k) * np] : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) ma += mv[k] * rdlane(qa, (j + k) & 63);  // lanes >= nv hold 0
  }
  if (inl) {
    d.qfrc_constraint[gv + lane] = qc_sum;
    d.efc_Ma[gv + lane] = ma;
    d.qfrc_inverse[gv + lane] = d.qfrc_bias[gv + lane] + ma - d.qfrc_passive[gv + lane] - qc_sum;
  }
}

}  // namespace inv
}  // namespace mjw

extern "C" int mjw_inverse(const mjw_model_t* m, const mjw_data_t* d, void* stream) {
  using namespace mjw;
  if (!m || !d) return set_last_error(-1, "mjw_inverse: null model / data");
  if (d->nworld <= 0) return 0;
  if (m->nv <= 0) return 0;
  if (!d->qacc || !d->qM || !d->qfrc_bias || !d->qfrc_passive || !d->qfrc_constraint || !d->efc_Ma || !d->qfrc_inverse || !d->nefc ||
      !d->ne || !d->nf)
    return set_last_error(-1, "mjw_inverse: null data array");
  const bool rows = d->njmax > 0 && !(m->opt_disableflags & DSBL_CONSTRAINT);
  if (rows && (!d->efc_J || !d->efc_D || !d->efc_aref || !d->efc_frictionloss || !d->efc_force || !d->efc_state || !d->efc_type || !d->efc_id))
    return set_last_error(-1, "mjw_inverse: null constraint array");
  if (rows && m->opt_cone == CONE_ELLIPTIC && d->naconmax > 0 && (!d->contact_efc_address || !d->contact_dim || !d->contact_friction))
    return set_last_error(-1, "mjw_inverse: null contact array");
  hipStream_t s = (hipStream_t)stream;
  if (m->is_sparse) {
    if (rows && (!d->efc_J_colind || !d->efc_J_rownnz || !d->efc_JT_adr || !d->efc_JT_rowind || !d->efc_JT_val || !d->sp_idx16 || !d->sp_row ||
                 !d->sp_cnt || !d->qfrc_smooth || !d->qacc_smooth))
      return set_last_error(-1, "mjw_inverse: null sparse workspace array");
    const int rc = sparse_inverse_launch(m, d, s);
    return rc ? set_last_error(rc, hipGetErrorString((hipError_t)rc)) : 0;
  }
  if (m->nv > 64) return set_last_error(-2, "mjw_inverse: model too large for the dense world-per-wave path (nv > 64)");
  const int in_lds = d->njmax <= inv::INV_LDS_ROWS;
  const size_t lds = in_lds ? (size_t)d->njmax * 4 : 0;
  hipLaunchKernelGGL(inv::inverse_kernel, dim3(d->nworld), dim3(64), lds, s, *m, *d, in_lds);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error((int)e, hipGetErrorString(e));
  return 0;
}
