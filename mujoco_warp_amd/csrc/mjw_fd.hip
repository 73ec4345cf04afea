// mjw_fd.hip -- the two kernels around `step` of the finite-difference linearisation (MuJoCo's mjd_transitionFD;
// include/mjw_amd.h mjw_fd_t): every perturbed copy of a world is one more world of a scratch Data, slot c of world w
// at scratch world c * nworld + w.  Both kernels are data movement.
//
//   fd_perturb_kernel     one wave per scratch world: the world's state and input rows are copied bitwise with
//                         consecutive lanes on consecutive words (the source rows are shared by all slots of a world
//                         and come from L2), then, after a barrier, lane 0 applies the slot's nudge from the nominal
//                         row: one add, or one quaternion product and normalisation in registers.
//   fd_difference_kernel  a transpose: a slot's next state is contiguous along the rows of A..D, the outputs are
//                         contiguous along the columns.  One workgroup per (world, tile of FD_TILE columns): the
//                         differences are staged in LDS as [column][row], lanes along the row (coalesced loads); the
//                         quaternion log is done once per (column, joint) by the thread of the joint's first rotational
//                         dof, which writes all three rows; then the tile is read back with lanes along the column
//                         and stored.  The LDS row stride is odd: a half wave reading one row of 32 columns touches 32
//                         different banks (ds_read_b32 banks are (addr / 4) % 32 per 32-lane half).
//
// The ctrl range rule (ctrl_nudges) is evaluated by both kernels from the nominal ctrl, in float32, so that the
// difference uses exactly the slots the perturbation filled.  Plain fp32, true divisions, no atomics.
#include "mjw_common.h"

namespace mjw {
namespace fd {

constexpr int FD_TILE = 32;          // columns per workgroup of the difference kernel
constexpr int FD_LDS_WORDS = 12288;  // 48 KiB of staging per workgroup

// what the kernels need of the model, next to the fd view (the model struct itself is not passed to them)
struct fd_args {
  mjw_fd_t fd;
  int nq, nv, na, nu, nbody, nmocap, neq, nsd;
  int clamp;          // the ctrl range rule applies (CLAMPCTRL not disabled)
  int ctrlrange_nb;   // batch size of actuator_ctrlrange
  int ncp;            // columns a pass holds
  int tile, stride;   // difference kernel: columns per workgroup and LDS row stride (odd)
  float eps;
  const int32_t* jnt_type;
  const int32_t* jnt_qposadr;
  const int32_t* jnt_dofadr;
  const int32_t* dof_jntid;
  const int32_t* ctrllimited;
  const float* ctrlrange;
};

__device__ __forceinline__ void copy_words(void* dst, const void* src, long row_dst, long row_src, int n, int lane) {
  uint32_t* o = (uint32_t*)dst + row_dst * n;
  const uint32_t* s = (const uint32_t*)src + row_src * n;
  for (int i = lane; i < n; i += 64) o[i] = s[i];
}

// MuJoCo's rule for the nudges of ctrl i of world w (mjd_stepFD): which of the + and - slots are perturbed
__device__ __forceinline__ void ctrl_nudges(const fd_args& a, int w, int i, bool& plus, bool& minus) {
  plus = true;
  minus = a.fd.centered != 0;
  if (a.clamp && a.ctrllimited[i]) {
    const float c = a.fd.n_ctrl[(long)w * a.nu + i];
    const float* r = a.ctrlrange + ((long)(w % a.ctrlrange_nb) * a.nu + i) * 2;
    const float lo = r[0], hi = r[1], cp = c + a.eps, cm = c - a.eps;
    const bool in0 = c >= lo && c <= hi;
    plus = in0 && cp >= lo && cp <= hi;
    minus = (a.fd.centered || !plus) && in0 && cm >= lo && cm <= hi;
  }
}

// which rows of qpos a dof nudges: scalar (adr) or the quaternion at adr with local axis `axis`
__device__ __forceinline__ bool dof_quat(const fd_args& a, int v, int& adr, int& axis) {
  const int j = a.dof_jntid[v], t = a.jnt_type[j], qa = a.jnt_qposadr[j], off = v - a.jnt_dofadr[j];
  if (t == JNT_FREE && off >= 3) { adr = qa + 3; axis = off - 3; return true; }
  if (t == JNT_BALL) { adr = qa; axis = off; return true; }
  adr = (t == JNT_FREE) ? qa + off : qa;
  axis = 0;
  return false;
}

__global__ void __launch_bounds__(256) fd_perturb_kernel(const fd_args a) {
  const mjw_fd_t& f = a.fd;
  const int lane = threadIdx.x & 63;
  const long sw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // scratch world
  const bool live = sw < (long)f.ncol_pass * f.nworld;
  const int c = live ? (int)(sw / f.nworld) : 0, w = live ? (int)(sw % f.nworld) : 0;
  if (live) {
    copy_words(f.s_time, f.n_time, sw, w, 1, lane);
    copy_words(f.s_qpos, f.n_qpos, sw, w, a.nq, lane);
    copy_words(f.s_qvel, f.n_qvel, sw, w, a.nv, lane);
    copy_words(f.s_act, f.n_act, sw, w, a.na, lane);
    copy_words(f.s_ctrl, f.n_ctrl, sw, w, a.nu, lane);
    copy_words(f.s_qacc_warmstart, f.n_qacc_warmstart, sw, w, a.nv, lane);
    copy_words(f.s_qfrc_applied, f.n_qfrc_applied, sw, w, a.nv, lane);
    copy_words(f.s_xfrc_applied, f.n_xfrc_applied, sw, w, a.nbody * 6, lane);
    copy_words(f.s_mocap_pos, f.n_mocap_pos, sw, w, a.nmocap * 3, lane);
    copy_words(f.s_mocap_quat, f.n_mocap_quat, sw, w, a.nmocap * 4, lane);
    copy_words(f.s_eq_active, f.n_eq_active, sw, w, a.neq, lane);
  }
  __syncthreads();  // the copies of this wave are done before its lane 0 overwrites one of them
  if (!live || lane != 0 || c == 0) return;
  const int j = (c - 1) % a.ncp;
  float sgn = c > a.ncp ? -1.0f : 1.0f;
  if (j >= f.ncols) return;  // a spare slot of the last pass: nominal
  const int col = f.col0 + j, nv = a.nv;
  if (col < nv) {
    int adr, axis;
    const float* q = f.n_qpos + (long)w * a.nq;
    float* o = f.s_qpos + sw * a.nq;
    if (!dof_quat(a, col, adr, axis)) {
      o[adr] = q[adr] + sgn * a.eps;
      return;
    }
    // quat * exp(sgn eps e_axis), exp(v) = (cos(|v| / 2), sin(|v| / 2) v / |v|), then normalised
    const float half = 0.5f * a.eps, pw = cosf(half), ps = sgn * sinf(half);
    const float px = axis == 0 ? ps : 0.0f, py = axis == 1 ? ps : 0.0f, pz = axis == 2 ? ps : 0.0f;
    const float qw = q[adr], qx = q[adr + 1], qy = q[adr + 2], qz = q[adr + 3];
    float rw = qw * pw - qx * px - qy * py - qz * pz;
    float rx = qw * px + qx * pw + qy * pz - qz * py;
    float ry = qw * py - qx * pz + qy * pw + qz * px;
    float rz = qw * pz + qx * py - qy * px + qz * pw;
    const float n = sqrtf(rw * rw + rx * rx + ry * ry + rz * rz);
    if (n < 1e-15f) { rw = 1.0f; rx = ry = rz = 0.0f; }
    else { rw = rw / n; rx = rx / n; ry = ry / n; rz = rz / n; }
    o[adr] = rw; o[adr + 1] = rx; o[adr + 2] = ry; o[adr + 3] = rz;
  } else if (col < 2 * nv) {
    f.s_qvel[sw * nv + (col - nv)] = f.n_qvel[(long)w * nv + (col - nv)] + sgn * a.eps;
  } else if (col < 2 * nv + a.na) {
    const int i = col - 2 * nv;
    f.s_act[sw * a.na + i] = f.n_act[(long)w * a.na + i] + sgn * a.eps;
  } else {
    const int i = col - 2 * nv - a.na;
    bool plus, minus;
    ctrl_nudges(a, w, i, plus, minus);
    bool go = sgn > 0.0f ? plus : minus;
    if (!f.centered && !plus && minus) { go = true; sgn = -1.0f; }  // a forward context's one slot takes the - nudge
    if (go) f.s_ctrl[sw * a.nu + i] = f.n_ctrl[(long)w * a.nu + i] + sgn * a.eps;
  }
}

// log(conj(q1) * q2) / h, mj_differentiatePos for a quaternion: angle * axis, the angle wrapped into (-pi, pi]
// (2 atan2(n, w) - 2 pi for w < 0 equals -2 atan2(n, -w): no subtraction of 2 pi, and atan2 stays within pi / 2)
__device__ __forceinline__ void quat_log_diff(const float* q1, const float* q2, float h, float* res) {
  const float aw = q1[0], ax = -q1[1], ay = -q1[2], az = -q1[3];
  const float bw = q2[0], bx = q2[1], by = q2[2], bz = q2[3];
  const float w = aw * bw - ax * bx - ay * by - az * bz;
  const float x = aw * bx + ax * bw + ay * bz - az * by;
  const float y = aw * by - ax * bz + ay * bw + az * bx;
  const float z = aw * bz + ax * by - ay * bx + az * bw;
  const float n = sqrtf(x * x + y * y + z * z);
  if (n < 1e-15f) { res[0] = res[1] = res[2] = 0.0f; return; }
  float ang = 2.0f * atan2f(n, fabsf(w));
  if (w < 0.0f) ang = -ang;
  res[0] = (x / n) * ang / h;
  res[1] = (y / n) * ang / h;
  res[2] = (z / n) * ang / h;
}

__global__ void __launch_bounds__(256) fd_difference_kernel(const fd_args a, const int ntile) {
  extern __shared__ float s_y[];  // [tile][stride]
  __shared__ long s_w1[FD_TILE], s_w2[FD_TILE];
  __shared__ float s_h[FD_TILE];
  const mjw_fd_t& f = a.fd;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int w = blockIdx.x / ntile, j0 = (blockIdx.x % ntile) * a.tile;
  const int tc = min(a.tile, f.ncols - j0);  // columns of this tile
  const int nv = a.nv, ndx = 2 * nv + a.na, NR = ndx + (f.C ? a.nsd : 0), S = a.stride;

  // ---- the two slots and the step h of every column of the tile; h = 0: a column without a nudge
  if (tid < tc) {
    const int j = j0 + tid, col = f.col0 + j;
    const long sp = (long)(1 + j) * f.nworld + w, sm = (long)(1 + a.ncp + j) * f.nworld + w, s0 = w;
    long w1 = f.centered ? sm : s0, w2 = sp;
    float h = f.centered ? 2.0f * a.eps : a.eps;
    if (col >= ndx) {
      bool plus, minus;
      ctrl_nudges(a, w, col - ndx, plus, minus);
      if (plus && minus) { /* centred */ }
      else if (plus) { w1 = s0; h = a.eps; }
      else if (minus) { w1 = f.centered ? sm : sp; w2 = s0; h = a.eps; }
      else h = 0.0f;
    }
    s_w1[tid] = w1;
    s_w2[tid] = w2;
    s_h[tid] = h;
  }
  __syncthreads();

  // ---- stage: lanes along the row index
  for (int idx = tid; idx < tc * NR; idx += nt) {
    const int c = idx / NR, r = idx - c * NR;
    const long w1 = s_w1[c], w2 = s_w2[c];
    const float h = s_h[c];
    float* y = s_y + c * S;
    if (h == 0.0f) { y[r] = 0.0f; continue; }
    if (r < nv) {
      int adr, axis;
      const float* q1 = f.s_qpos + w1 * a.nq;
      const float* q2 = f.s_qpos + w2 * a.nq;
      if (!dof_quat(a, r, adr, axis)) y[r] = (q2[adr] - q1[adr]) / h;
      else if (axis == 0) quat_log_diff(q1 + adr, q2 + adr, h, y + r);  // rows r .. r + 2, once per joint
    } else if (r < 2 * nv) {
      const int i = r - nv;
      y[r] = (f.s_qvel[w2 * nv + i] - f.s_qvel[w1 * nv + i]) / h;
    } else if (r < ndx) {
      const int i = r - 2 * nv;
      y[r] = (f.s_act[w2 * a.na + i] - f.s_act[w1 * a.na + i]) / h;
    } else {
      const int i = r - ndx;
      y[r] = (f.s_sensordata[w2 * a.nsd + i] - f.s_sensordata[w1 * a.nsd + i]) / h;
    }
  }
  __syncthreads();

  // ---- store: lanes along the column index, the last dimension of A..D
  for (int idx = tid; idx < tc * NR; idx += nt) {
    const int r = idx / tc, c = idx - r * tc;
    const int col = f.col0 + j0 + c;
    const float v = s_y[c * S + r];
    if (r < ndx) {
      if (col < ndx) f.A[((long)w * ndx + r) * f.lda + col] = v;
      else f.B[((long)w * ndx + r) * f.ldb + (col - ndx)] = v;
    } else {
      const int rs = r - ndx;
      if (col < ndx) f.C[((long)w * a.nsd + rs) * f.ldc + col] = v;
      else f.D[((long)w * a.nsd + rs) * f.ldd + (col - ndx)] = v;
    }
  }
}

// the checks both entries share and the kernels' argument block; 1: nothing to do
static int make_args(const char* who, const mjw_model_t* m, const mjw_data_t* d, const mjw_fd_t* f, float eps, fd_args& a) {
  char msg[160];
#define FD_FAIL(code, text) do { snprintf(msg, sizeof msg, "%s: %s", who, text); return set_last_error(code, msg); } while (0)
  if (!m || !d || !f) FD_FAIL(-1, "null model / data / fd view");
  if (d->nworld <= 0) return 1;
  if (m->nv <= 0) FD_FAIL(-4, "a model without dofs (nv == 0) has no state to perturb");
  if (!(eps > 0.0f)) FD_FAIL(-4, "eps must be positive");
  const int K = 2 * m->nv + m->na + m->nu;
  if (f->nworld != d->nworld) FD_FAIL(-4, "nworld of the fd view differs from the Data's");
  if (f->ncol != K) FD_FAIL(-4, "ncol of the fd view is not 2 nv + na + nu of the model");
  const int cen = f->centered != 0;
  if (f->ncol_pass < (cen ? 3 : 2) || (cen && (f->ncol_pass & 1) == 0)) FD_FAIL(-4, "ncol_pass must be 1 + 2 ncp centred, 1 + ncp forward, ncp >= 1");
  const int ncp = cen ? (f->ncol_pass - 1) / 2 : f->ncol_pass - 1;
  if (f->col0 < 0 || f->ncols < 1 || f->ncols > ncp || f->col0 > K - f->ncols) FD_FAIL(-4, "the pass's column range lies outside the slots or the columns");
  if ((long)f->ncol_pass * f->nworld > 0x7fffffffL) FD_FAIL(-2, "more scratch worlds than an int holds");
  if (!m->jnt_type || !m->jnt_qposadr || !m->jnt_dofadr || !m->dof_jntid) FD_FAIL(-1, "null joint table");
  if (m->nu > 0 && (!m->actuator_ctrllimited || !m->actuator_ctrlrange || m->actuator_ctrlrange_nb < 1)) FD_FAIL(-1, "null actuator table");
  if (f->n_time != d->time || f->n_qpos != d->qpos || f->n_qvel != d->qvel || f->n_ctrl != d->ctrl || f->n_act != d->act)
    FD_FAIL(-4, "the nominal pointers of the fd view are not the Data's");
  const struct { const void* n; const void* s; int cnt; } rows[] = {
    {f->n_time, f->s_time, 1}, {f->n_qpos, f->s_qpos, m->nq}, {f->n_qvel, f->s_qvel, m->nv}, {f->n_act, f->s_act, m->na},
    {f->n_ctrl, f->s_ctrl, m->nu}, {f->n_qacc_warmstart, f->s_qacc_warmstart, m->nv}, {f->n_qfrc_applied, f->s_qfrc_applied, m->nv},
    {f->n_xfrc_applied, f->s_xfrc_applied, m->nbody * 6}, {f->n_mocap_pos, f->s_mocap_pos, m->nmocap * 3},
    {f->n_mocap_quat, f->s_mocap_quat, m->nmocap * 4}, {f->n_eq_active, f->s_eq_active, m->neq}};
  for (const auto& r : rows)
    if (r.cnt > 0 && (!r.n || !r.s)) FD_FAIL(-1, "null state array");
#undef FD_FAIL
  a.fd = *f;
  a.fd.centered = cen;
  a.nq = m->nq; a.nv = m->nv; a.na = m->na; a.nu = m->nu; a.nbody = m->nbody; a.nmocap = m->nmocap; a.neq = m->neq;
  a.nsd = m->nsensordata;
  a.clamp = (m->opt_disableflags & DSBL_CLAMPCTRL) == 0;
  a.ctrlrange_nb = m->nu > 0 ? m->actuator_ctrlrange_nb : 1;
  a.ncp = ncp;
  a.tile = a.stride = 0;
  a.eps = eps;
  a.jnt_type = m->jnt_type; a.jnt_qposadr = m->jnt_qposadr; a.jnt_dofadr = m->jnt_dofadr; a.dof_jntid = m->dof_jntid;
  a.ctrllimited = m->actuator_ctrllimited;
  a.ctrlrange = m->actuator_ctrlrange;
  return 0;
}

}  // namespace fd
}  // namespace mjw

extern "C" int mjw_sizeof_fd(void) { return (int)sizeof(mjw_fd_t); }

extern "C" int mjw_fd_perturb(const mjw_model_t* m, const mjw_data_t* d, const mjw_fd_t* f, float eps, void* stream) {
  using namespace mjw;
  fd::fd_args a;
  const int rc = fd::make_args("mjw_fd_perturb", m, d, f, eps, a);
  if (rc) return rc > 0 ? 0 : rc;
  const long total = (long)f->ncol_pass * f->nworld;
  hipLaunchKernelGGL(fd::fd_perturb_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error((int)e, hipGetErrorString(e));
  return 0;
}

extern "C" int mjw_fd_difference(const mjw_model_t* m, const mjw_data_t* d, const mjw_fd_t* f, float eps, void* stream) {
  using namespace mjw;
  fd::fd_args a;
  const int rc = fd::make_args("mjw_fd_difference", m, d, f, eps, a);
  if (rc) return rc > 0 ? 0 : rc;
  const int ndx = 2 * m->nv + m->na, K = ndx + m->nu;
  if (!f->A || (m->nu > 0 && !f->B)) return set_last_error(-1, "mjw_fd_difference: null A / B");
  if ((f->C != nullptr) != (f->D != nullptr) && m->nu > 0) return set_last_error(-1, "mjw_fd_difference: C and D are both given or both null");
  const bool sens = f->C != nullptr && m->nsensordata > 0;
  if (sens && !f->s_sensordata) return set_last_error(-1, "mjw_fd_difference: null sensordata");
  if (f->lda < ndx || (m->nu > 0 && f->ldb < m->nu) || (sens && (f->ldc < ndx || (m->nu > 0 && f->ldd < m->nu))))
    return set_last_error(-4, "mjw_fd_difference: a leading dimension is smaller than its row");
  (void)K;
  if (!sens) a.fd.C = a.fd.D = nullptr;
  const int NR = ndx + (sens ? m->nsensordata : 0);
  a.stride = NR | 1;
  a.tile = fd::FD_LDS_WORDS / a.stride < fd::FD_TILE ? fd::FD_LDS_WORDS / a.stride : fd::FD_TILE;
  if (a.tile < 1) return set_last_error(-2, "mjw_fd_difference: 2 nv + na + nsensordata > 12287: one column does not fit the staging");
  const int ntile = (f->ncols + a.tile - 1) / a.tile;
  if ((long)ntile * f->nworld > 0x7fffffffL) return set_last_error(-2, "mjw_fd_difference: more workgroups than the grid holds");
  hipLaunchKernelGGL(fd::fd_difference_kernel, dim3((unsigned)(ntile * f->nworld)), dim3(256), (size_t)a.tile * a.stride * sizeof(float),
                     (hipStream_t)stream, a, ntile);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error((int)e, hipGetErrorString(e));
  return 0;
}
