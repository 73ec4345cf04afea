// mjw_flexrender.h -- what the refit kernel (mjw_flexrender.hip) and the render kernel (mjw_render.hip) share of
// flex rendering: the argument block, how a face id becomes three points, and the loop over the flexes.
//
// The surface (mujoco_warp/_src/bvh.py:608-975, render.py:218-242): a dim-2 flex is a shell of thickness 2 r around
// its elements, two faces per element at +-r along the normals and two per boundary edge closing the rim; a dim-3
// flex is its flex_shell triangles; a dim-1 flex is one capsule of radius r per edge.  The faces are never stored:
// a corner record (vertex, sign, normal source) and this world's vertex positions and vertex normals give a point
// when it is needed, in the refit and in the ray loop by the same routine, so a leaf's box holds exactly the points
// the ray meets.
#pragma once

#include "mjw_ray.h"

namespace mjw {
namespace ray {

enum : int { FI_DIM = 0, FI_VERTADR, FI_VERTNUM, FI_FACEADR, FI_NFACE, FI_NODEADR, FI_NNODE, FI_DEPTH, FI_LEVELADR, FI_EDGEADR, FI_EDGENUM, FI_W = 12 };

// mjw_flexrender_t and the vertex positions of the Data
struct FlexArgs {
  int nflex, nflexvert, nflexelem, nflexedge, nface, nnode, ninc, nlevel, min_faces;
  const int *info, *corner, *elem_vert, *edge_vert, *inc_adr, *inc, *tri, *level;
  const float *radius, *rgba, *node, *xpos;
  float *node_box, *vert_norm;
};

// host: 1 when there are flexes to refit / draw, 0 when there are none, < 0 refused
inline int check_flex_args(const char* who, const mjw_model_t* m, const mjw_data_t* d, const mjw_flexrender_t* fr, FlexArgs& fx) {
  const std::string w(who);
  if (!fr) return refuse_null(who, "flex render tables");
  if (fr->nflex != m->nflex || fr->nflexvert != m->nflexvert || fr->nflexelem != m->nflexelem || fr->nflexedge != m->nflexedge)
    return set_last_error(-4, (w + ": the flex tables were built for another model (nflex / nflexvert / nflexelem / nflexedge)").c_str());
  if (fr->nface < 0 || fr->nnode < 0 || fr->ninc < 0 || fr->nlevel < 0 || fr->leaf_size > BVH_LEAF || fr->max_depth > 32)
    return set_last_error(-4, (w + ": flex nface / nnode / ninc / nlevel / leaf_size / max_depth out of range").c_str());
  if (fr->nflex <= 0) return 0;
  if (!fr->info || !fr->flex_radius || !fr->flex_rgba || !fr->inc_adr || !fr->node_box || !fr->vert_norm || (fr->nface > 0 && (!fr->corner || !fr->tri)) ||
      (fr->nflexelem > 0 && !fr->elem_vert) || (fr->nflexedge > 0 && !fr->edge_vert) || (fr->ninc > 0 && !fr->inc) || (fr->nnode > 0 && !fr->node) ||
      (fr->nlevel > 0 && !fr->level))
    return set_last_error(-1, (w + ": null flex table").c_str());
  if (!d->flexvert_xpos) return set_last_error(-1, (w + ": null flexvert_xpos").c_str());
  fx.nflex = fr->nflex; fx.nflexvert = fr->nflexvert; fx.nflexelem = fr->nflexelem; fx.nflexedge = fr->nflexedge;
  fx.nface = fr->nface; fx.nnode = fr->nnode; fx.ninc = fr->ninc; fx.nlevel = fr->nlevel; fx.min_faces = fr->min_faces;
  fx.info = fr->info; fx.corner = fr->corner; fx.elem_vert = fr->elem_vert; fx.edge_vert = fr->edge_vert;
  fx.inc_adr = fr->inc_adr; fx.inc = fr->inc; fx.tri = fr->tri; fx.level = fr->level;
  fx.radius = fr->flex_radius; fx.rgba = fr->flex_rgba; fx.node = fr->node; fx.xpos = d->flexvert_xpos;
  fx.node_box = fr->node_box; fx.vert_norm = fr->vert_norm;
  return 1;
}

// what one (world, flex) reads: the flex's row of info checked against the table sizes, and this world's rows
struct FlexView {
  int dim, vertadr, vertnum, faceadr, nface, nodeadr, nnode, depth, leveladr, edgeadr, edgenum;
  float r;
  const float *xpos_w, *norm_w, *box_w;
};
// false (uniform over the workgroup): the row does not fit its tables, the flex is left alone
__device__ __forceinline__ bool flex_view(const FlexArgs& fx, int wid, int f, FlexView& v) {
  const int* in = fx.info + FI_W * (long)f;
  v.dim = uni(in[FI_DIM]); v.vertadr = uni(in[FI_VERTADR]); v.vertnum = uni(in[FI_VERTNUM]); v.faceadr = uni(in[FI_FACEADR]);
  v.nface = uni(in[FI_NFACE]); v.nodeadr = uni(in[FI_NODEADR]); v.nnode = uni(in[FI_NNODE]); v.depth = uni(in[FI_DEPTH]);
  v.leveladr = uni(in[FI_LEVELADR]); v.edgeadr = uni(in[FI_EDGEADR]); v.edgenum = uni(in[FI_EDGENUM]);
  if (v.vertadr < 0 || v.vertnum < 0 || v.vertadr > fx.nflexvert - v.vertnum || v.faceadr < 0 || v.nface < 0 || v.faceadr > fx.nface - v.nface ||
      v.nodeadr < 0 || v.nnode < 1 || v.nodeadr > fx.nnode - v.nnode || v.depth < 1 || v.depth > 32 || v.leveladr < 0 ||
      v.leveladr > fx.nlevel - (v.depth + 1) || v.edgeadr < 0 || v.edgenum < 0 || v.edgeadr > fx.nflexedge - v.edgenum)
    return false;
  v.r = fx.radius[f];
  v.xpos_w = fx.xpos + (long)wid * fx.nflexvert * 3;
  v.norm_w = fx.vert_norm + (long)wid * fx.nflexvert * 3;
  v.box_w = fx.node_box + (long)wid * (fx.nnode + fx.nflex) * 6;
  return true;
}

// normalize((v1 - v0) x (v2 - v0)) of dim-2 element e; zero for a zero-area element or an id outside the tables
__device__ __forceinline__ void flex_elem_normal(const FlexArgs& fx, const float* xpos_w, int e, float* n) {
  n[0] = n[1] = n[2] = 0.0f;
  if ((unsigned)e >= (unsigned)fx.nflexelem) return;
  const int* ev = fx.elem_vert + 3 * (long)e;
  const int i0 = ev[0], i1 = ev[1], i2 = ev[2];
  if ((unsigned)i0 >= (unsigned)fx.nflexvert || (unsigned)i1 >= (unsigned)fx.nflexvert || (unsigned)i2 >= (unsigned)fx.nflexvert) return;
  const float *v0 = xpos_w + 3 * (long)i0, *v1 = xpos_w + 3 * (long)i1, *v2 = xpos_w + 3 * (long)i2;
  const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  cross3(n, a, b);
  normalize3(n);
}

// the point of one corner record
__device__ __forceinline__ bool flex_corner(const FlexArgs& fx, const float* xpos_w, const float* norm_w, float r, const int* rec, float* p) {
  const int v = rec[0], sign = rec[1], src = rec[2];
  if ((unsigned)v >= (unsigned)fx.nflexvert) return false;
  const float* x = xpos_w + 3 * (long)v;
  float n[3] = {0.0f, 0.0f, 0.0f};
  if (sign != 0) {
    if (src < 0) {
      const float* nv = norm_w + 3 * (long)v;
      n[0] = nv[0]; n[1] = nv[1]; n[2] = nv[2];
    } else {
      flex_elem_normal(fx, xpos_w, src, n);
    }
  }
  const float s = (float)sign * r;
  for (int i = 0; i < 3; i++) p[i] = x[i] + s * n[i];
  return true;
}

// the three points of face `face` (an index into the whole corner table)
__device__ __forceinline__ bool flex_face_points(const FlexArgs& fx, const float* xpos_w, const float* norm_w, float r, long face, float* p0,
                                                 float* p1, float* p2) {
  const int* rec = fx.corner + 9 * face;
  return flex_corner(fx, xpos_w, norm_w, r, rec, p0) && flex_corner(fx, xpos_w, norm_w, r, rec + 3, p1) &&
         flex_corner(fx, xpos_w, norm_w, r, rec + 6, p2);
}

// bvh_walk's source for a flex: this world's refit boxes, points made on the fly
struct FlexSrc {
  const FlexArgs* fx;
  const FlexView* v;
  __device__ __forceinline__ const float* box(int node) const { return v->box_w + 6 * (long)(v->nodeadr + node); }
  __device__ __forceinline__ bool points(int f, float* p0, float* p1, float* p2) const {
    return flex_face_points(*fx, v->xpos_w, v->norm_w, v->r, (long)v->faceadr + f, p0, p1, p2);
  }
};

// the capsule of radius r between a and b (a sphere when they coincide), world frame; the normal points outwards
__device__ __forceinline__ float ray_edge_capsule(const float* a, const float* b, float r, const float* pnt, const float* vec, float* n) {
  const float mid[3] = {0.5f * (a[0] + b[0]), 0.5f * (a[1] + b[1]), 0.5f * (a[2] + b[2])};
  float ax[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float len = sqrtf(dot3(ax, ax));
  const float d[3] = {pnt[0] - mid[0], pnt[1] - mid[1], pnt[2] - mid[2]};
  if (!(len > 0.0f)) return ray_sphere(r * r, d, vec, n);
  for (int i = 0; i < 3; i++) ax[i] /= len;
  float e0[3], e1[3];
  ray_basis(ax, e0, e1);  // (e0, e1, ax): an orthonormal frame with the axis as z
  const float lp[3] = {dot3(d, e0), dot3(d, e1), dot3(d, ax)}, lv[3] = {dot3(vec, e0), dot3(vec, e1), dot3(vec, ax)};
  const float size[2] = {r, 0.5f * len};
  float nl[3] = {0.0f, 0.0f, 0.0f};
  const float x = ray_capsule(size, lp, lv, nl);
  for (int i = 0; i < 3; i++) n[i] = nl[0] * e0[i] + nl[1] * e1[i] + nl[2] * ax[i];
  return x;
}

// Every lane's ray (pnt, vec; world frame) against every flex of world wid, after the geom loop: a hit strictly nearer
// than `best` replaces best / fid (the flex id) / bn (a triangle's winding normal turned to face the ray, a capsule's
// outward normal), so a geom keeps a tie, and so does the lower flex id.  ANYHIT: a lane that has a hit (fid >= 0)
// stops looking.  It holds no barrier: everything is read through wave-uniform addresses.  Per flex the wave first
// tests its rays against the whole-flex box the refit left; then a flex of at least fx.min_faces faces is walked
// through its tree, a smaller one face by face (the same hit bit for bit: the lowest face id among equal
// distances), and a dim-1 flex edge by edge behind a bounding-ball test.
template <bool ANYHIT>
__device__ __forceinline__ void flex_loop(const FlexArgs& fx, int wid, bool active, const float* pnt, const float* vec, float& best, int& fid,
                                          float* bn) {
  if (!__any(active)) return;
  RaySlab slab;
  ray_slab(vec, slab);
  float b0[3], b1[3];
  ray_basis(vec, b0, b1);
  for (int f = 0; f < fx.nflex; f++) {
    FlexView v;
    if (!flex_view(fx, wid, f, v)) continue;  // (uniform)
    bool cand = active;
    if (ANYHIT) cand = cand && fid < 0;
    const float* whole = v.box_w + 6 * (long)(fx.nnode + f);
    float tmin;
    cand = cand && slab_test(whole, slab_pad(whole, pnt), pnt, slab, tmin) && tmin * 0.9990234375f <= best;
    if (!__any(cand)) continue;

    float x = -1.0f, n[3] = {0.0f, 0.0f, 0.0f};
    if (v.dim == 1) {
      if (!(v.r > 0.0f)) continue;  // (uniform) a rope without thickness draws nothing
      for (int e = v.edgeadr; e < v.edgeadr + v.edgenum; e++) {
        const int i0 = uni(fx.edge_vert[2 * (long)e]), i1 = uni(fx.edge_vert[2 * (long)e + 1]);
        if ((unsigned)i0 >= (unsigned)fx.nflexvert || (unsigned)i1 >= (unsigned)fx.nflexvert) continue;
        const float *a = v.xpos_w + 3 * (long)i0, *b = v.xpos_w + 3 * (long)i1;
        const float mid[3] = {0.5f * (a[0] + b[0]), 0.5f * (a[1] + b[1]), 0.5f * (a[2] + b[2])};
        const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const float rad = 0.5f * sqrtf(dot3(ab, ab)) + v.r;
        if (!__any(cand && ball_test(mid, rad * rad * 1.002f + 1e-12f, pnt, vec))) continue;
        float ne[3] = {0.0f, 0.0f, 0.0f};
        const float sol = ray_edge_capsule(a, b, v.r, pnt, vec, ne);
        if (sol >= 0.0f && (x < 0.0f || sol < x)) {
          x = sol;
          n[0] = ne[0]; n[1] = ne[1]; n[2] = ne[2];
        }
      }
    } else {
      if (v.nface >= fx.min_faces) {  // (uniform)
        x = bvh_walk<ANYHIT>(FlexSrc{&fx, &v}, fx.node + 8 * (long)v.nodeadr, v.nnode, fx.tri + v.faceadr, v.nface, cand, pnt, vec, b0, b1, best, n);
      } else {
        for (int k = 0; k < v.nface; k++) {
          float p0[3], p1[3], p2[3], nt[3];
          if (!flex_face_points(fx, v.xpos_w, v.norm_w, v.r, (long)v.faceadr + k, p0, p1, p2)) continue;
          const float sol = ray_triangle(p0, p1, p2, pnt, vec, b0, b1, nt);
          if (sol >= 0.0f && (x < 0.0f || sol < x)) {
            x = sol;
            n[0] = nt[0]; n[1] = nt[1]; n[2] = nt[2];
          }
        }
      }
      if (dot3(n, vec) > 0.0f) {  // the winding normal turned to face the ray
        n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2];
      }
    }
    if (cand && x >= 0.0f && x < best) {
      best = x;
      fid = f;
      bn[0] = n[0]; bn[1] = n[1]; bn[2] = n[2];
    }
  }
}

}  // namespace ray
}  // namespace mjw
