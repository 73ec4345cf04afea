// mjw_ray.hip -- batched ray casting over all geom types (mjw_rays; mujoco_warp/_src/ray.py:909-1010 `_ray`
// and :1212-1312 `rays` without a render context).
//
// Mapping: one workgroup serves one world and a tile of rays, each lane owns one ray and loops over the
// geoms.  Every lane of a wave is at the same geom at the same time, so the geom's type, frame, size and mesh
// faces are wave-uniform and only hit / miss diverges; the nearest hit needs no cross-lane reduction, and a
// strict `<` in geom order gives equal distances to the lowest geom id.  The geoms are staged in LDS in
// chunks of RAY_CHUNK records; a record's "eliminated" flag (transparent, filtered group, static) is
// worked out once per workgroup while staging, the inner loop tests only the flag and the ray's bodyexclude.
// A geom no lane's bounding test passes is skipped by the whole wave (ballot), so the mesh and heightfield
// loops run only in waves with a candidate ray.
#include "mjw_common.h"
#include "mjw_ray.h"

namespace mjw {
namespace ray {

constexpr int RAY_CHUNK = 128;  // geoms staged in LDS at a time
// words of a staged record: pos 3, mat 9, size 3, aabb 6 (centre, half extents; geom frame), bounding ball
// (world-frame centre 3, squared radius 1), then four ints: type, data id, body id, eliminated
enum : int { R_POS = 0, R_MAT = 3, R_SIZE = 12, R_AABB = 15, R_BALL = 21, R_TYPE = 25, R_DATA = 26, R_BODY = 27, R_ELIM = 28 };
constexpr int RECW = 29;

// the arrays the kernel reads (a small block instead of mjw_model_t / mjw_data_t by value)
struct RayArgs {
  int ngeom, nworld, nray, ntile, pnt_nb, vec_nb, flg_static, group_mask;  // group_mask < 0: no group filter
  int nmat, nmeshface, nmesh, nhfield;
  const float *geom_xpos, *geom_xmat;
  const float *geom_size, *geom_aabb, *geom_rgba, *mat_rgba, *mesh_vert, *hfield_size, *hfield_data;
  int size_nb, aabb_nb, rgba_nb, matrgba_nb, vert_nb, hsize_nb, hdata_nb, nmeshvert, nhfielddata, pad_;
  const int *geom_type, *geom_bodyid, *geom_dataid, *geom_group, *geom_matid, *body_weldid;
  const int *mesh_vertadr, *mesh_face, *mesh_faceadr, *mesh_facenum, *hfield_nrow, *hfield_ncol, *hfield_adr;
  const float *pnt, *vec;
  const int* bodyexclude;
  float* dist;
  int* geomid;
  float* normal;
};

__device__ __forceinline__ const float* row(const float* p, int nb, long cnt, int w) { return nb <= 1 ? p : p + (long)(w % nb) * cnt; }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

template <int NT>
__global__ void __launch_bounds__(NT) rays_kernel(const RayArgs a) {
  __shared__ float recs[RAY_CHUNK * RECW];
  const int tid = threadIdx.x;
  const int wid = blockIdx.x / a.ntile, tile = blockIdx.x - wid * a.ntile;
  const int r = tile * NT + tid;
  const bool active = r < a.nray;
  const int rr = active ? r : a.nray - 1;  // idle lanes follow the last ray and write nothing
  const float* pw = a.pnt + ((long)(wid % a.pnt_nb) * a.nray + rr) * 3;
  const float* vw = a.vec + ((long)(wid % a.vec_nb) * a.nray + rr) * 3;
  const float pnt[3] = {pw[0], pw[1], pw[2]}, vec[3] = {vw[0], vw[1], vw[2]};
  const int excl = a.bodyexclude[rr];

  const float* size_w = row(a.geom_size, a.size_nb, (long)a.ngeom * 3, wid);
  const float* aabb_w = row(a.geom_aabb, a.aabb_nb, (long)a.ngeom * 6, wid);
  const float* rgba_w = row(a.geom_rgba, a.rgba_nb, (long)a.ngeom * 4, wid);
  const float* matrgba_w = row(a.mat_rgba, a.matrgba_nb, (long)a.nmat * 4, wid);
  const float* xpos_w = a.geom_xpos + (long)wid * a.ngeom * 3;
  const float* xmat_w = a.geom_xmat + (long)wid * a.ngeom * 9;

  float best = MJW_MAXVAL, bn[3] = {0.0f, 0.0f, 0.0f};
  int bid = -1;

  for (int g0 = 0; g0 < a.ngeom; g0 += RAY_CHUNK) {
    const int n = min(RAY_CHUNK, a.ngeom - g0);
    __syncthreads();  // the previous chunk is consumed
    for (int k = tid; k < n; k += NT) {
      const int g = g0 + k;
      float* rec = recs + k * RECW;
      for (int i = 0; i < 3; i++) rec[R_POS + i] = xpos_w[3 * g + i];
      for (int i = 0; i < 9; i++) rec[R_MAT + i] = xmat_w[9 * g + i];
      for (int i = 0; i < 3; i++) rec[R_SIZE + i] = size_w[3 * g + i];
      for (int i = 0; i < 6; i++) rec[R_AABB + i] = aabb_w[6 * g + i];
      // bounding ball: centre = pos + mat aabb_centre, radius = |half extents| (a little generous, so that
      // rounding never culls a ray the exact routine would accept)
      const float* c = rec + R_AABB;
      for (int i = 0; i < 3; i++)
        rec[R_BALL + i] = rec[R_POS + i] + rec[R_MAT + 3 * i] * c[0] + rec[R_MAT + 3 * i + 1] * c[1] + rec[R_MAT + 3 * i + 2] * c[2];
      rec[R_BALL + 3] = (c[3] * c[3] + c[4] * c[4] + c[5] * c[5]) * 1.002f + 1e-12f;
      const int body = a.geom_bodyid[g], matid = a.geom_matid[g];
      // ray.py:52-102 without the per-ray body exclusion
      bool elim = matid < 0 ? rgba_w[4 * g + 3] == 0.0f : (matid < a.nmat && matrgba_w[4 * matid + 3] == 0.0f);
      if (!a.flg_static && a.body_weldid[body] == 0) elim = true;
      if (a.group_mask >= 0 && !((a.group_mask >> min(5, max(0, a.geom_group[g]))) & 1)) elim = true;
      int* ri = reinterpret_cast<int*>(rec);
      ri[R_TYPE] = a.geom_type[g];
      ri[R_DATA] = a.geom_dataid[g];
      ri[R_BODY] = body;
      ri[R_ELIM] = elim ? 1 : 0;
    }
    __syncthreads();

    for (int k = 0; k < n; k++) {
      const float* rec = recs + k * RECW;
      const int* ri = reinterpret_cast<const int*>(rec);
      if (uni(ri[R_ELIM])) continue;  // eliminated for every ray of the workgroup
      const int type = uni(ri[R_TYPE]);
      bool cand = active && ri[R_BODY] != excl;
      if (type != RG_PLANE) cand = cand && ball_test(rec + R_BALL, rec[R_BALL + 3], pnt, vec);
      if (!__any(cand)) continue;  // no ray of this wave can hit the geom

      float lp[3], lv[3], nl[3] = {0.0f, 0.0f, 0.0f};
      ray_map(rec + R_POS, rec + R_MAT, pnt, vec, lp, lv);
      float x = -1.0f;
      if (type == RG_MESH) {
        // ray.py:622-697 with the bounding box of geom_aabb (centre and half extents in the geom frame)
        const float lpc[3] = {lp[0] - rec[R_AABB], lp[1] - rec[R_AABB + 1], lp[2] - rec[R_AABB + 2]};
        cand = cand && box_test(rec + R_AABB + 3, lpc, lv);
        if (!__any(cand)) continue;
        const int mesh = uni(ri[R_DATA]);
        if (mesh < 0 || mesh >= a.nmesh) continue;
        float b0[3], b1[3];
        ray_basis(lv, b0, b1);
        // the face loop is wave-uniform: indices and vertices are read through uniform addresses
        const float* vert = row(a.mesh_vert, a.vert_nb, (long)a.nmeshvert * 3, wid) + 3 * (long)a.mesh_vertadr[mesh];
        const int f0 = a.mesh_faceadr[mesh], f1 = min(f0 + a.mesh_facenum[mesh], a.nmeshface);
        for (int f = f0; f < f1; f++) {
          const int* idx = a.mesh_face + 3 * (long)f;
          float n[3];
          const float sol = ray_triangle(vert + 3 * idx[0], vert + 3 * idx[1], vert + 3 * idx[2], lp, lv, b0, b1, n);
          if (sol >= 0.0f && (x < 0.0f || sol < x)) {
            x = sol;
            nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
          }
        }
      } else if (type == RG_HFIELD) {
        const int hid = uni(ri[R_DATA]);
        if (hid < 0 || hid >= a.nhfield) continue;
        const float* hsize = row(a.hfield_size, a.hsize_nb, (long)a.nhfield * 4, wid) + 4 * hid;
        const float* data = row(a.hfield_data, a.hdata_nb, (long)a.nhfielddata, wid) + a.hfield_adr[hid];
        if (cand) x = ray_hfield(hsize, a.hfield_nrow[hid], a.hfield_ncol[hid], data, lp, lv, nl);
      } else {
        x = ray_geom(type, rec + R_SIZE, lp, lv, nl);
      }
      if (cand && x >= 0.0f && x < best) {
        best = x;
        bid = g0 + k;
        rot_to_world(rec + R_MAT, nl, bn);
      }
    }
  }

  if (active) {
    const long o = (long)wid * a.nray + r;
    const bool hit = bid >= 0;
    a.dist[o] = hit ? best : -1.0f;
    a.geomid[o] = bid;
    for (int i = 0; i < 3; i++) a.normal[3 * o + i] = hit ? bn[i] : 0.0f;
  }
}

}  // namespace ray
}  // namespace mjw

extern "C" int mjw_rays(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb,
                        const float* vec, int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude,
                        float* dist, int* geomid, float* normal, void* stream) {
  using namespace mjw::ray;
  if (!m || !d || !rm) return mjw::set_last_error(-1, "mjw_rays: null model / data / ray model");
  if (nray < 0) return mjw::set_last_error(-4, "mjw_rays: nray < 0");
  if (nray == 0 || d->nworld <= 0) return 0;
  if (!pnt || !vec || !bodyexclude || !dist || !geomid || !normal) return mjw::set_last_error(-1, "mjw_rays: null ray / output array");
  if ((pnt_nb != 1 && pnt_nb != d->nworld) || (vec_nb != 1 && vec_nb != d->nworld))
    return mjw::set_last_error(-4, "mjw_rays: pnt / vec batch must be 1 or nworld");
  if (rm->ngeom != m->ngeom) return mjw::set_last_error(-4, "mjw_rays: ray model ngeom differs from the model's");
  if (m->ngeom > 0 && (!rm->geom_group || !rm->geom_matid || !rm->geom_rgba || rm->geom_rgba_nb < 1 || !d->geom_xpos || !d->geom_xmat))
    return mjw::set_last_error(-1, "mjw_rays: null geom array");
  if (rm->nmat > 0 && (!rm->mat_rgba || rm->mat_rgba_nb < 1)) return mjw::set_last_error(-1, "mjw_rays: null mat_rgba");
  if (rm->nmeshface > 0 && (!rm->mesh_face || !rm->mesh_faceadr || !rm->mesh_facenum)) return mjw::set_last_error(-1, "mjw_rays: null mesh face array");

  RayArgs a;
  memset(&a, 0, sizeof(a));
  a.ngeom = m->ngeom; a.nworld = d->nworld; a.nray = nray; a.pnt_nb = pnt_nb; a.vec_nb = vec_nb; a.flg_static = flg_static != 0;
  a.group_mask = -1;
  if (geomgroup) {
    bool all_unset = true;
    int mask = 0;
    for (int i = 0; i < 6; i++) {
      all_unset = all_unset && geomgroup[i] == -1;
      if (geomgroup[i] != 0) mask |= 1 << i;
    }
    if (!all_unset) a.group_mask = mask;
  }
  a.nmat = rm->nmat; a.nmeshface = rm->nmeshface; a.nmesh = rm->nmeshface > 0 ? m->nmesh : 0; a.nhfield = m->nhfield;
  a.geom_xpos = d->geom_xpos; a.geom_xmat = d->geom_xmat;
  a.geom_size = m->geom_size; a.size_nb = m->geom_size_nb;
  a.geom_aabb = m->geom_aabb; a.aabb_nb = m->geom_aabb_nb;
  a.geom_rgba = rm->geom_rgba; a.rgba_nb = rm->geom_rgba_nb;
  a.mat_rgba = rm->mat_rgba; a.matrgba_nb = rm->mat_rgba_nb;
  a.mesh_vert = m->mesh_vert; a.vert_nb = m->mesh_vert_nb; a.nmeshvert = m->nmeshvert;
  a.hfield_size = m->hfield_size; a.hsize_nb = m->hfield_size_nb;
  a.hfield_data = m->hfield_data; a.hdata_nb = m->hfield_data_nb; a.nhfielddata = m->nhfielddata;
  a.geom_type = m->geom_type; a.geom_bodyid = m->geom_bodyid; a.geom_dataid = m->geom_dataid;
  a.geom_group = rm->geom_group; a.geom_matid = rm->geom_matid; a.body_weldid = m->body_weldid;
  a.mesh_vertadr = m->mesh_vertadr; a.mesh_face = rm->mesh_face; a.mesh_faceadr = rm->mesh_faceadr; a.mesh_facenum = rm->mesh_facenum;
  a.hfield_nrow = m->hfield_nrow; a.hfield_ncol = m->hfield_ncol; a.hfield_adr = m->hfield_adr;
  a.pnt = pnt; a.vec = vec; a.bodyexclude = bodyexclude; a.dist = dist; a.geomid = geomid; a.normal = normal;

  hipStream_t s = (hipStream_t)stream;
  const int nt = nray <= 64 ? 64 : 256;
  a.ntile = (nray + nt - 1) / nt;
  const long nblock = (long)a.nworld * a.ntile;
  if (nblock > 0x7fffffffL) return mjw::set_last_error(-2, "mjw_rays: nworld x ray tiles exceeds the grid limit");
  if (nt == 64)
    hipLaunchKernelGGL(rays_kernel<64>, dim3((unsigned)nblock), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(rays_kernel<256>, dim3((unsigned)nblock), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mjw::set_last_error((int)e, hipGetErrorString(e));
  return 0;
}
