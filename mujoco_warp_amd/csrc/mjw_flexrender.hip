// mjw_flexrender.hip -- mjw_flex_refit: the per-world vertex normals and bounding boxes of the flex trees of a render
// context (mujoco_warp/_src/bvh.py:843-975 `refit_flex_bvh`), the first trees of this code base whose boxes change
// every step.  The topology of a tree is static (bvh.py builds it over the rest pose); only the boxes are refit.
//
// One launch, one workgroup of 256 per (world, flex), four phases with a barrier between them:
//   1 normals   dim 2, one thread per vertex: the unit normals of the incident elements, gathered through the CSR in
//               ascending element order and summed in that order, normalised (no atomics: the result is deterministic)
//   2 leaves    one thread per leaf: the minimum / maximum of the points of its (at most four) faces, made by the
//               routine the ray loop uses (flex_face_points), so the box holds exactly what a ray can meet
//   3 inner     level by level from the deepest up, one thread per node: the union of its two children, which lie
//               after it (the level offsets come from the host)
//   4 whole     the box of the flex's vertices grown by the radius: the ray loop's first cull, and all a dim-1 flex has
// Phases 2 to 4 read what earlier phases of the same workgroup wrote to global memory (the normals, the children's
// boxes): a block-scope fence and the barrier order them.  Positions are read from global memory where they are
// needed: a vertex is read by the six elements around it and by its own thread, all of one workgroup, so the second
// and later reads hit the vector cache, and nothing caps the size of a flex the way a staging buffer in LDS would.
#include "mjw_common.h"
#include "mjw_flexrender.h"

namespace mjw {
namespace ray {

constexpr int REFIT_NT = 256;

__device__ __forceinline__ void grow(float* lo, float* hi, const float* p) {
  for (int i = 0; i < 3; i++) {
    lo[i] = fminf(lo[i], p[i]);
    hi[i] = fmaxf(hi[i], p[i]);
  }
}

__global__ void __launch_bounds__(REFIT_NT) flex_refit_kernel(const FlexArgs fx) {
  __shared__ float red[6][REFIT_NT / 64];
  const int tid = threadIdx.x;
  const int wid = blockIdx.x / fx.nflex, f = blockIdx.x - wid * fx.nflex;
  FlexView v;
  if (!flex_view(fx, wid, f, v)) return;  // (uniform over the workgroup)
  float* norm_w = fx.vert_norm + (long)wid * fx.nflexvert * 3;
  float* box_w = fx.node_box + (long)wid * (fx.nnode + fx.nflex) * 6;

  // 1 vertex normals (zero for the vertices of a dim-1 or dim-3 flex)
  for (int k = tid; k < v.vertnum; k += REFIT_NT) {
    const int vert = v.vertadr + k;
    float s[3] = {0.0f, 0.0f, 0.0f};
    if (v.dim == 2) {
      const int i0 = max(fx.inc_adr[vert], 0), i1 = min(fx.inc_adr[vert + 1], fx.ninc);
      for (int i = i0; i < i1; i++) {
        float n[3];
        flex_elem_normal(fx, v.xpos_w, fx.inc[i], n);
        s[0] += n[0]; s[1] += n[1]; s[2] += n[2];
      }
      normalize3(s);
    }
    norm_w[3 * (long)vert] = s[0]; norm_w[3 * (long)vert + 1] = s[1]; norm_w[3 * (long)vert + 2] = s[2];
  }
  __threadfence_block();
  __syncthreads();

  // 2 leaves
  const int* nodes = reinterpret_cast<const int*>(fx.node + 8 * (long)v.nodeadr);
  float* box = box_w + 6 * (long)v.nodeadr;
  const int* tri = fx.tri + v.faceadr;
  for (int node = tid; node < v.nnode; node += REFIT_NT) {
    const int ia = nodes[8 * node + 6], ib = nodes[8 * node + 7];
    if (ib > 0) continue;
    const int cnt = min(-ib, BVH_LEAF);
    float lo[3] = {MJW_MAXVAL, MJW_MAXVAL, MJW_MAXVAL}, hi[3] = {-MJW_MAXVAL, -MJW_MAXVAL, -MJW_MAXVAL};
    if (cnt == 0) {  // the empty root of a flex without faces
      lo[0] = lo[1] = lo[2] = hi[0] = hi[1] = hi[2] = 0.0f;
    } else if (ia >= 0 && ia <= v.nface - cnt) {
      for (int i = 0; i < cnt; i++) {
        const int face = tri[ia + i];
        float p0[3], p1[3], p2[3];
        if ((unsigned)face >= (unsigned)v.nface || !flex_face_points(fx, v.xpos_w, v.norm_w, v.r, (long)v.faceadr + face, p0, p1, p2)) continue;
        grow(lo, hi, p0);
        grow(lo, hi, p1);
        grow(lo, hi, p2);
      }
    }
    for (int i = 0; i < 3; i++) {
      box[6 * node + i] = lo[i];
      box[6 * node + 3 + i] = hi[i];
    }
  }
  __threadfence_block();
  __syncthreads();

  // 3 inner nodes, the deepest level first (the last level holds leaves only)
  const int* level = fx.level + v.leveladr;
  for (int l = v.depth - 2; l >= 0; l--) {
    const int n0 = max(level[l], 0), n1 = min(level[l + 1], v.nnode);
    for (int node = n0 + tid; node < n1; node += REFIT_NT) {
      const int ia = nodes[8 * node + 6], ib = nodes[8 * node + 7];
      if (ib <= 0) continue;
      const int lc = ia, rc = ib & ((1 << BVH_AXIS_SHIFT) - 1);
      if (lc <= node || lc >= v.nnode || rc <= node || rc >= v.nnode) continue;
      for (int i = 0; i < 3; i++) {
        box[6 * node + i] = fminf(box[6 * lc + i], box[6 * rc + i]);
        box[6 * node + 3 + i] = fmaxf(box[6 * lc + 3 + i], box[6 * rc + 3 + i]);
      }
    }
    __threadfence_block();
    __syncthreads();
  }

  // 4 the whole flex: its vertices, grown by the radius
  float lo[3] = {MJW_MAXVAL, MJW_MAXVAL, MJW_MAXVAL}, hi[3] = {-MJW_MAXVAL, -MJW_MAXVAL, -MJW_MAXVAL};
  for (int k = tid; k < v.vertnum; k += REFIT_NT) grow(lo, hi, v.xpos_w + 3 * (long)(v.vertadr + k));
  for (int off = 32; off > 0; off >>= 1)
    for (int i = 0; i < 3; i++) {
      lo[i] = fminf(lo[i], __shfl_xor(lo[i], off));
      hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], off));
    }
  if ((tid & 63) == 0)
    for (int i = 0; i < 3; i++) {
      red[i][tid >> 6] = lo[i];
      red[3 + i][tid >> 6] = hi[i];
    }
  __syncthreads();
  if (tid < 3) {
    float a = red[tid][0], b = red[3 + tid][0];
    for (int w = 1; w < REFIT_NT / 64; w++) {
      a = fminf(a, red[tid][w]);
      b = fmaxf(b, red[3 + tid][w]);
    }
    const float r = fmaxf(v.r, 0.0f);
    float* whole = box_w + 6 * (long)(fx.nnode + f);
    whole[tid] = a - r;
    whole[3 + tid] = b + r;
  }
}

}  // namespace ray
}  // namespace mjw

extern "C" int mjw_sizeof_flexrender(void) { return (int)sizeof(mjw_flexrender_t); }

extern "C" int mjw_flex_refit(const mjw_model_t* m, const mjw_data_t* d, const mjw_flexrender_t* fr, void* stream) {
  using namespace mjw::ray;
  if (!m || !d) return mjw::set_last_error(-1, "mjw_flex_refit: null model / data");
  FlexArgs fx;
  memset(&fx, 0, sizeof(fx));
  const int have = check_flex_args("mjw_flex_refit", m, d, fr, fx);
  if (have < 0) return have;
  if (have == 0 || d->nworld <= 0) return 0;
  const long nblock = (long)d->nworld * fx.nflex;
  if (nblock > 0x7fffffffL) return mjw::set_last_error(-2, "mjw_flex_refit: nworld x nflex exceeds the grid limit");
  hipLaunchKernelGGL(flex_refit_kernel, dim3((unsigned)nblock), dim3(REFIT_NT), 0, (hipStream_t)stream, fx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mjw::set_last_error((int)e, hipGetErrorString(e));
  return 0;
}
