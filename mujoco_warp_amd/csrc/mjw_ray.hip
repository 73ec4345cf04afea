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
// loops run only in waves with a candidate ray.  The loop itself (staging, culling, nearest hit) is geom_loop
// of mjw_ray.h, which the render kernel (mjw_render.hip) calls too.  There is one kernel, rays_kernel<NT, BVH>;
// mjw_rays_bvh launches it with BVH = true: meshes are walked through the static trees of a render context (mesh_bvh,
// mjw_ray.h).  mjw_rays, and a context whose trees do not serve the call, launch BVH = false: every face of every mesh.
#include "mjw_common.h"
#include "mjw_ray.h"

namespace mjw {
namespace ray {

// the arrays the kernel reads: the shared geom block (mjw_ray.h) and the rays
struct RayArgs {
  GeomArgs g;
  int nworld, nray, ntile, pnt_nb, vec_nb, pad_;
  const float *pnt, *vec;
  const int* bodyexclude;
  float* dist;
  int* geomid;
  float* normal;
};

template <int NT, bool BVH>
__device__ __forceinline__ void rays_body(const RayArgs& a, const BvhArgs& bv, float* recs) {
  const int tid = threadIdx.x;
  const int wid = blockIdx.x / a.ntile, tile = blockIdx.x - wid * a.ntile;
  const int r = tile * NT + tid;
  const bool active = r < a.nray;
  const int rr = active ? r : a.nray - 1;  // idle lanes follow the last ray and write nothing
  const float* pw = a.pnt + ((long)(wid % a.pnt_nb) * a.nray + rr) * 3;
  const float* vw = a.vec + ((long)(wid % a.vec_nb) * a.nray + rr) * 3;
  const float pnt[3] = {pw[0], pw[1], pw[2]}, vec[3] = {vw[0], vw[1], vw[2]};
  const int excl = a.bodyexclude[rr];

  float best = MJW_MAXVAL, bn[3] = {0.0f, 0.0f, 0.0f};
  int bid = -1;
  geom_loop<NT, false, BVH>(a.g, bv, wid, recs, false, active, excl, pnt, vec, best, bid, bn);

  if (active) {
    const long o = (long)wid * a.nray + r;
    const bool hit = bid >= 0;
    a.dist[o] = hit ? best : -1.0f;
    a.geomid[o] = bid;
    for (int i = 0; i < 3; i++) a.normal[3 * o + i] = hit ? bn[i] : 0.0f;
  }
}

// BVH: the meshes are walked through the BVHs of a render context (bv); without it bv is never read
template <int NT, bool BVH>
__global__ void __launch_bounds__(NT) rays_kernel(const RayArgs a, const BvhArgs bv) {
  __shared__ float recs[RAY_CHUNK * RECW];
  rays_body<NT, BVH>(a, bv, recs);
}

}  // namespace ray
}  // namespace mjw

static int rays_launch(const char* who, const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb,
                       const float* vec, int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude, float* dist,
                       int* geomid, float* normal, const mjw_bvh_t* bvh, void* stream) {
  using namespace mjw::ray;
  const std::string w(who);
  if (!m || !d || !rm) return mjw::set_last_error(-1, (w + ": null model / data / ray model").c_str());
  if (nray < 0) return mjw::set_last_error(-4, (w + ": nray < 0").c_str());
  BvhArgs bv;
  memset(&bv, 0, sizeof(bv));
  int walk = 0;
  if (bvh && (walk = check_bvh_args(who, m, rm, bvh, bv)) < 0) return walk;
  if (nray == 0 || d->nworld <= 0) return 0;
  if (!pnt || !vec || !bodyexclude || !dist || !geomid || !normal) return mjw::set_last_error(-1, (w + ": null ray / output array").c_str());
  if ((pnt_nb != 1 && pnt_nb != d->nworld) || (vec_nb != 1 && vec_nb != d->nworld))
    return mjw::set_last_error(-4, (w + ": pnt / vec batch must be 1 or nworld").c_str());
  if (int e = check_geom_args(who, m, d, rm)) return e;

  RayArgs a;
  memset(&a, 0, sizeof(a));
  a.nworld = d->nworld; a.nray = nray; a.pnt_nb = pnt_nb; a.vec_nb = vec_nb;
  a.g.flg_static = flg_static != 0;
  a.g.group_mask = -1;
  if (geomgroup) {
    bool all_unset = true;
    int mask = 0;
    for (int i = 0; i < 6; i++) {
      all_unset = all_unset && geomgroup[i] == -1;
      if (geomgroup[i] != 0) mask |= 1 << i;
    }
    if (!all_unset) a.g.group_mask = mask;
  }
  fill_geom_args(a.g, m, d, rm);
  a.pnt = pnt; a.vec = vec; a.bodyexclude = bodyexclude; a.dist = dist; a.geomid = geomid; a.normal = normal;

  hipStream_t s = (hipStream_t)stream;
  const int nt = nray <= 64 ? 64 : 256;
  a.ntile = (nray + nt - 1) / nt;
  const long nblock = (long)a.nworld * a.ntile;
  if (nblock > 0x7fffffffL) return mjw::set_last_error(-2, (w + ": nworld x ray tiles exceeds the grid limit").c_str());
  with_flag(nt == 64, [&](auto small) {
    with_flag(walk != 0, [&](auto bvh_on) {
      constexpr int NT = decltype(small)::value ? 64 : 256;
      hipLaunchKernelGGL((rays_kernel<NT, decltype(bvh_on)::value>), dim3((unsigned)nblock), dim3(NT), 0, s, a, bv);
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mjw::set_last_error((int)e, hipGetErrorString(e));
  return 0;
}

extern "C" int mjw_rays(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb,
                        const float* vec, int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude,
                        float* dist, int* geomid, float* normal, void* stream) {
  return rays_launch("mjw_rays", m, d, rm, pnt, pnt_nb, vec, vec_nb, nray, geomgroup, flg_static, bodyexclude, dist, geomid, normal, nullptr,
                     stream);
}

extern "C" int mjw_rays_bvh(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb,
                            const float* vec, int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude,
                            float* dist, int* geomid, float* normal, const mjw_bvh_t* bvh, void* stream) {
  // (a null bvh is refused where it always was: after the model pointers and nray)
  if (m && d && rm && nray >= 0 && !bvh) return mjw::ray::refuse_null("mjw_rays_bvh", "bvh");
  return rays_launch("mjw_rays_bvh", m, d, rm, pnt, pnt_nb, vec, vec_nb, nray, geomgroup, flg_static, bodyexclude, dist, geomid, normal, bvh,
                     stream);
}
