// mjw_ray.h -- ray / geom intersection routines (fp32, device), the per-lane part of mjw_rays.
//
// Semantics follow mujoco_warp/_src/ray.py (cited per routine).  Every routine takes the ray already mapped
// into the geom's frame (ray_map: lp = mat' (pnt - pos), lv = mat' vec), returns the distance x >= 0 along
// lv to the nearest hit (-1: no hit) and writes the surface normal in the geom's frame; the caller rotates
// it to the world frame (rot_to_world).  lv is not normalised: x is in units of |lv|.  They keep no state and
// read nothing but their arguments, so a sensor kernel can call them per lane as the ray kernel does.
//
// The geom loop at the end of the file (staging in LDS, culling, nearest / any hit) is what rays_kernel and
// render_kernel share.
//
// The touch sensor's distance-only routines (mjw_sensor.h ray_quad / ray_geom_local) are separate and
// unchanged; these live in their own namespace.
#pragma once

#include <type_traits>

#include "mjw_common.h"

namespace mjw {
namespace ray {

enum : int { RG_PLANE = 0, RG_HFIELD = 1, RG_SPHERE = 2, RG_CAPSULE = 3, RG_ELLIPSOID = 4, RG_CYLINDER = 5, RG_BOX = 6, RG_MESH = 7 };

// ray.py:33-49: the ray in the frame (pos, mat), mat row-major
__device__ __forceinline__ void ray_map(const float* pos, const float* mat, const float* pnt, const float* vec, float* lp, float* lv) {
  const float d[3] = {pnt[0] - pos[0], pnt[1] - pos[1], pnt[2] - pos[2]};
  for (int i = 0; i < 3; i++) {
    lp[i] = mat[i] * d[0] + mat[3 + i] * d[1] + mat[6 + i] * d[2];
    lv[i] = mat[i] * vec[0] + mat[3 + i] * vec[1] + mat[6 + i] * vec[2];
  }
}

__device__ __forceinline__ void rot_to_world(const float* mat, const float* nl, float* n) {
  for (int i = 0; i < 3; i++) n[i] = mat[3 * i] * nl[0] + mat[3 * i + 1] * nl[1] + mat[3 * i + 2] * nl[2];
}

// ray.py:105-125: roots of a x^2 + 2 b x + c; returns the smaller non-negative one (-1: none), x0 <= x1 both
__device__ __forceinline__ float quad_roots(float a, float b, float c, float& x0, float& x1) {
  float det = b * b - a * c;
  x0 = x1 = -1.0f;
  if (det < MJW_MINVAL) return -1.0f;
  det = sqrtf(det);
  const float den = safe_div(1.0f, a);
  x0 = (-b - det) * den;
  x1 = (-b + det) * den;
  return x0 >= 0.0f ? x0 : (x1 >= 0.0f ? x1 : -1.0f);
}

// conservative pre-test: can the ray p + x v, x >= 0, meet the ball |q - c|^2 <= r2?  (no MINVAL cut-off: a
// grazing ray passes and the exact routine decides)
__device__ __forceinline__ bool ball_test(const float* c, float r2, const float* p, const float* v) {
  const float d[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const float a = dot3(v, v), b = dot3(v, d), cc = dot3(d, d) - r2;
  if (cc <= 0.0f) return true;           // origin inside
  return b < 0.0f && b * b - a * cc >= 0.0f;  // heading towards it and the line meets it
}

// ray.py:187-208: front side only, inside the rendered rectangle when size[0] / size[1] > 0
__device__ __forceinline__ float ray_plane(const float* size, const float* lp, const float* lv, float* nl) {
  if (lv[2] > -MJW_MINVAL) return -1.0f;
  const float x = -lp[2] / lv[2];
  if (x < 0.0f) return -1.0f;
  const float p0 = lp[0] + x * lv[0], p1 = lp[1] + x * lv[1];
  if ((size[0] > 0.0f && fabsf(p0) > size[0]) || (size[1] > 0.0f && fabsf(p1) > size[1])) return -1.0f;
  nl[0] = 0.0f; nl[1] = 0.0f; nl[2] = 1.0f;
  return x;
}

// ray.py:211-225 (sphere of squared radius r2 at the frame origin)
__device__ __forceinline__ float ray_sphere(float r2, const float* lp, const float* lv, float* nl) {
  float x0, x1;
  const float x = quad_roots(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - r2, x0, x1);
  if (x >= 0.0f) {
    for (int i = 0; i < 3; i++) nl[i] = lp[i] + x * lv[i];
    normalize3(nl);
  }
  return x;
}

// ray.py:228-299: the round side between the caps, then each cap's half sphere; normal radial or the cap's
__device__ __forceinline__ float ray_capsule(const float* size, const float* lp, const float* lv, float* nl) {
  const float r2 = size[0] * size[0], h = size[1];
  float x = -1.0f, x0, x1;
  float cap = 0.0f;  // z of the cap centre the hit belongs to (0: the round side)
  bool side = true;
  const float a2 = lv[0] * lv[0] + lv[1] * lv[1];
  const float sol = quad_roots(a2, lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - r2, x0, x1);
  if (sol >= 0.0f && fabsf(lp[2] + sol * lv[2]) <= h) x = sol;
  const float a3 = a2 + lv[2] * lv[2];
  for (int s = 1; s >= -1; s -= 2) {  // top cap, then bottom cap
    const float cz = (float)s * h;
    const float dz = lp[2] - cz;
    quad_roots(a3, lv[0] * lp[0] + lv[1] * lp[1] + lv[2] * dz, lp[0] * lp[0] + lp[1] * lp[1] + dz * dz - r2, x0, x1);
    const float xs[2] = {x0, x1};
    for (int i = 0; i < 2; i++) {
      const float z = lp[2] + xs[i] * lv[2];
      if (xs[i] >= 0.0f && (s > 0 ? z >= h : z <= -h) && (x < 0.0f || xs[i] < x)) {
        x = xs[i];
        cap = cz;
        side = false;
      }
    }
  }
  if (x >= 0.0f) {
    nl[0] = lp[0] + x * lv[0];
    nl[1] = lp[1] + x * lv[1];
    nl[2] = side ? 0.0f : lp[2] + x * lv[2] - cap;
    normalize3(nl);
  }
  return x;
}

// ray.py:302-330: normal = the gradient of the ellipsoid function at the hit
__device__ __forceinline__ float ray_ellipsoid(const float* size, const float* lp, const float* lv, float* nl) {
  float s[3], a = 0.0f, b = 0.0f, c = -1.0f, x0, x1;
  for (int i = 0; i < 3; i++) {
    s[i] = safe_div(1.0f, size[i] * size[i]);
    a += s[i] * lv[i] * lv[i];
    b += s[i] * lv[i] * lp[i];
    c += s[i] * lp[i] * lp[i];
  }
  const float x = quad_roots(a, b, c, x0, x1);
  if (x >= 0.0f) {
    for (int i = 0; i < 3; i++) nl[i] = s[i] * (lp[i] + x * lv[i]);
    normalize3(nl);
  }
  return x;
}

// ray.py:333-391: the flat ends inside the radius, the round side between them; normal +-z or radial
__device__ __forceinline__ float ray_cylinder(const float* size, const float* lp, const float* lv, float* nl) {
  const float r2 = size[0] * size[0], h = size[1];
  float x = -1.0f, end = 0.0f, x0, x1;
  if (fabsf(lv[2]) > MJW_MINVAL) {
    for (int s = -1; s <= 1; s += 2) {
      const float sol = ((float)s * h - lp[2]) / lv[2];
      if (sol < 0.0f) continue;
      const float p0 = lp[0] + sol * lv[0], p1 = lp[1] + sol * lv[1];
      if (p0 * p0 + p1 * p1 <= r2 && (x < 0.0f || sol < x)) {
        x = sol;
        end = (float)s;
      }
    }
  }
  const float sol = quad_roots(lv[0] * lv[0] + lv[1] * lv[1], lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - r2, x0, x1);
  if (sol >= 0.0f && fabsf(lp[2] + sol * lv[2]) <= h && (x < 0.0f || sol < x)) {
    x = sol;
    end = 0.0f;
  }
  if (x >= 0.0f) {
    if (end == 0.0f) {
      nl[0] = lp[0] + x * lv[0];
      nl[1] = lp[1] + x * lv[1];
      nl[2] = 0.0f;
      normalize3(nl);
    } else {
      nl[0] = 0.0f; nl[1] = 0.0f; nl[2] = end;
    }
  }
  return x;
}

// ray.py:397-448: the nearest face hit with x >= 0 (from inside: the far face); normal = the face's.
// all (optional, 6 floats): the hit distance of each face, index 2 axis + (side + 1) / 2, -1 where missed.
__device__ __forceinline__ float ray_box(const float* size, const float* lp, const float* lv, float* nl, float* all) {
  float x = -1.0f;
  int face = -1;
  if (all)
    for (int i = 0; i < 6; i++) all[i] = -1.0f;
  for (int i = 0; i < 3; i++) {
    if (!(fabsf(lv[i]) > MJW_MINVAL)) continue;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    for (int s = 0; s < 2; s++) {
      const float sol = ((s ? size[i] : -size[i]) - lp[i]) / lv[i];
      if (!(sol >= 0.0f)) continue;
      if (fabsf(lp[j] + sol * lv[j]) <= size[j] && fabsf(lp[k] + sol * lv[k]) <= size[k]) {
        if (x < 0.0f || sol < x) {
          x = sol;
          face = 2 * i + s;
        }
        if (all) all[2 * i + s] = sol;
      }
    }
  }
  if (x >= 0.0f) {
    nl[0] = nl[1] = nl[2] = 0.0f;
    nl[face >> 1] = (face & 1) ? 1.0f : -1.0f;
  }
  return x;
}

// does the ray meet the box at all (ray_box without the normal; the mesh's bounding-box pre-test)
__device__ __forceinline__ bool box_test(const float* size, const float* lp, const float* lv) {
  float n[3];
  return ray_box(size, lp, lv, n, nullptr) >= 0.0f;
}

// the primitive types (ray.py:799-820); meshes and heightfields need their data (below)
__device__ __forceinline__ float ray_geom(int type, const float* size, const float* lp, const float* lv, float* nl) {
  switch (type) {
    case RG_PLANE: return ray_plane(size, lp, lv, nl);
    case RG_SPHERE: return ray_sphere(size[0] * size[0], lp, lv, nl);
    case RG_CAPSULE: return ray_capsule(size, lp, lv, nl);
    case RG_ELLIPSOID: return ray_ellipsoid(size, lp, lv, nl);
    case RG_CYLINDER: return ray_cylinder(size, lp, lv, nl);
    case RG_BOX: return ray_box(size, lp, lv, nl, nullptr);
    default: return -1.0f;
  }
}

// two unit vectors spanning the plane normal to lv (any such pair serves ray_triangle)
__device__ __forceinline__ void ray_basis(const float* lv, float* b0, float* b1) {
  const float ax = fabsf(lv[0]), ay = fabsf(lv[1]), az = fabsf(lv[2]);
  float e[3] = {0.0f, 0.0f, 0.0f};
  e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0f;  // the axis lv leans on least
  cross3(b0, lv, e);
  normalize3(b0);
  cross3(b1, lv, b0);
  normalize3(b1);
}

// ray.py:128-184: two-sided triangle; the vertices are projected on (b0, b1), the origin must lie inside the
// projected triangle (edges included); normal = normalize((v0 - v2) x (v1 - v2)), by the winding
__device__ __forceinline__ float ray_triangle(const float* v0, const float* v1, const float* v2, const float* lp, const float* lv,
                                              const float* b0, const float* b1, float* nl) {
  float px[3], py[3];
  const float* v[3] = {v0, v1, v2};
  for (int k = 0; k < 3; k++) {
    const float d[3] = {v[k][0] - lp[0], v[k][1] - lp[1], v[k][2] - lp[2]};
    px[k] = dot3(d, b0);
    py[k] = dot3(d, b1);
  }
  if ((px[0] > 0.0f && px[1] > 0.0f && px[2] > 0.0f) || (px[0] < 0.0f && px[1] < 0.0f && px[2] < 0.0f) ||
      (py[0] > 0.0f && py[1] > 0.0f && py[2] > 0.0f) || (py[0] < 0.0f && py[1] < 0.0f && py[2] < 0.0f))
    return -1.0f;
  // s e0 + t e1 = -p2 with e0 = p0 - p2, e1 = p1 - p2
  const float e0x = px[0] - px[2], e0y = py[0] - py[2], e1x = px[1] - px[2], e1y = py[1] - py[2];
  const float det = e0x * e1y - e1x * e0y;
  if (fabsf(det) < MJW_MINVAL) return -1.0f;
  const float s = (e1x * py[2] - e1y * px[2]) / det;
  const float t = (e0y * px[2] - e0x * py[2]) / det;
  if (s < 0.0f || t < 0.0f || s + t > 1.0f) return -1.0f;
  const float d0[3] = {v0[0] - v2[0], v0[1] - v2[1], v0[2] - v2[2]};
  const float d1[3] = {v1[0] - v2[0], v1[1] - v2[1], v1[2] - v2[2]};
  const float dp[3] = {lp[0] - v2[0], lp[1] - v2[1], lp[2] - v2[2]};
  float n[3];
  cross3(n, d0, d1);
  const float den = dot3(lv, n);
  if (fabsf(den) < MJW_MINVAL) return -1.0f;
  const float x = -dot3(dp, n) / den;
  if (!(x >= 0.0f)) return -1.0f;
  normalize3(n);
  nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
  return x;
}

// ray.py:451-619: heightfield = the base box (z in [-size[3], 0]), the surface triangles of the cells under
// the ray's segment through the top box (z in [0, size[2]]), and the four side walls below the elevation
// profile.  hsize = hfield_size (x, y half extents, top, base); data = the nrow x ncol elevations in [0, 1].
__device__ __forceinline__ float ray_hfield(const float* hsize, int nrow, int ncol, const float* data, const float* lp, const float* lv,
                                            float* nl) {
  const float sx = hsize[0], sy = hsize[1], top = hsize[2], base = hsize[3];
  const float bsize[3] = {sx, sy, 0.5f * base}, tsize[3] = {sx, sy, 0.5f * top};
  const float lpb[3] = {lp[0], lp[1], lp[2] + 0.5f * base}, lpt[3] = {lp[0], lp[1], lp[2] - 0.5f * top};
  float all[6], nt[3];
  float x = ray_box(bsize, lpb, lv, nl, nullptr);
  const float xt = ray_box(tsize, lpt, lv, nt, all);
  if (xt < 0.0f) return x;

  float b0[3], b1[3];
  ray_basis(lv, b0, b1);
  // the part of the ray inside the top box
  float seg0 = 0.0f, seg1 = xt;
  for (int i = 0; i < 6; i++)
    if (all[i] > seg1) {
      seg0 = xt;
      seg1 = all[i];
    }
  const float dx = safe_div(2.0f * sx, (float)(ncol - 1)), dy = safe_div(2.0f * sy, (float)(nrow - 1));
  const float cx0 = safe_div(lp[0] + seg0 * lv[0] + sx, dx), cx1 = safe_div(lp[0] + seg1 * lv[0] + sx, dx);
  const float cy0 = safe_div(lp[1] + seg0 * lv[1] + sy, dy), cy1 = safe_div(lp[1] + seg1 * lv[1] + sy, dy);
  // cell ranges with one cell of padding, clamped before the conversion to int
  const float fc = (float)(ncol - 1), fr = (float)(nrow - 1);
  const int cmin = (int)fmaxf(0.0f, fminf(fc, floorf(fminf(cx0, cx1)) - 1.0f));
  const int cmax = (int)fminf(fc, fmaxf(0.0f, ceilf(fmaxf(cx0, cx1)) + 1.0f));
  const int rmin = (int)fmaxf(0.0f, fminf(fr, floorf(fminf(cy0, cy1)) - 1.0f));
  const int rmax = (int)fminf(fr, fmaxf(0.0f, ceilf(fmaxf(cy0, cy1)) + 1.0f));
  for (int r = rmin; r < rmax; r++) {
    for (int c = cmin; c < cmax; c++) {
      const float xa = dx * (float)c - sx, xb = dx * (float)(c + 1) - sx;
      const float ya = dy * (float)r - sy, yb = dy * (float)(r + 1) - sy;
      const float v00[3] = {xa, ya, data[r * ncol + c] * top};
      const float v10[3] = {xb, ya, data[r * ncol + c + 1] * top};
      const float v11[3] = {xb, yb, data[(r + 1) * ncol + c + 1] * top};
      const float v01[3] = {xa, yb, data[(r + 1) * ncol + c] * top};
      float n[3];
      float sol = ray_triangle(v00, v10, v11, lp, lv, b0, b1, n);
      if (sol >= 0.0f && (x < 0.0f || sol < x)) {
        x = sol;
        nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
      }
      sol = ray_triangle(v00, v11, v01, lp, lv, b0, b1, n);
      if (sol >= 0.0f && (x < 0.0f || sol < x)) {
        x = sol;
        nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
      }
    }
  }
  // side walls: the x faces (0: -x, 1: +x) and y faces (2: -y, 3: +y) of the top box, where the hit lies
  // below the elevation profile along that edge
  for (int i = 0; i < 4; i++) {
    if (!(all[i] >= 0.0f && (all[i] < x || x < 0.0f))) continue;
    const float z = safe_div(lp[2] + all[i] * lv[2], top);
    float y, y0, z0, z1;
    if (i < 2) {
      y = safe_div(lp[1] + all[i] * lv[1] + sy, dy);
      y0 = fmaxf(0.0f, fminf((float)(nrow - 2), floorf(y)));
      const int k = (int)y0, c = i == 1 ? ncol - 1 : 0;
      z0 = data[k * ncol + c];
      z1 = data[(k + 1) * ncol + c];
    } else {
      y = safe_div(lp[0] + all[i] * lv[0] + sx, dx);
      y0 = fmaxf(0.0f, fminf((float)(ncol - 2), floorf(y)));
      const int k = (int)y0, r = i == 3 ? nrow - 1 : 0;
      z0 = data[r * ncol + k];
      z1 = data[r * ncol + k + 1];
    }
    if (z < z0 * (y0 + 1.0f - y) + z1 * (y - y0)) {
      x = all[i];
      nl[0] = (float)(i == 1) - (float)(i == 0);
      nl[1] = (float)(i == 3) - (float)(i == 2);
      nl[2] = 0.0f;
    }
  }
  return x;
}

// ---- the geom loop shared by rays_kernel (mjw_ray.hip) and render_kernel (mjw_render.hip) -------------------
//
// One workgroup serves one world; the geoms are staged in LDS in chunks of RAY_CHUNK records and every lane
// walks the staged chunk with its own ray, so a geom's type, frame, size and mesh faces are wave-uniform.

constexpr int RAY_CHUNK = 128;  // geoms staged in LDS at a time
// words of a staged record: pos 3, mat 9, size 3, aabb 6 (centre, half extents; geom frame), bounding ball
// (world-frame centre 3, squared radius 1), then four ints: type, data id, body id, eliminated
enum : int { R_POS = 0, R_MAT = 3, R_SIZE = 12, R_AABB = 15, R_BALL = 21, R_TYPE = 25, R_DATA = 26, R_BODY = 27, R_ELIM = 28 };
constexpr int RECW = 29;

// the geom arrays the loop reads (a small block instead of mjw_model_t / mjw_data_t by value)
struct GeomArgs {
  int ngeom, nmat, nmeshface, nmesh, nhfield, nmeshvert, nhfielddata;
  // which geoms are left out.  draw_rule 0 (rays, ray.py:52-102 without the per-ray body exclusion): alpha 0,
  // static bodies when !flg_static, and group_mask >= 0 without bit clamp(geom_group, 0, 5).  draw_rule 1
  // (render, render.py:89-253): exactly the geoms whose group is no bit of draw_groups; no alpha or static rule.
  int flg_static, group_mask, draw_rule;
  unsigned draw_groups;
  int size_nb, aabb_nb, rgba_nb, matrgba_nb, vert_nb, hsize_nb, hdata_nb;
  const float *geom_xpos, *geom_xmat;
  const float *geom_size, *geom_aabb, *geom_rgba, *mat_rgba, *mesh_vert, *hfield_size, *hfield_data;
  const int *geom_type, *geom_bodyid, *geom_dataid, *geom_group, *geom_matid, *body_weldid;
  const int *mesh_vertadr, *mesh_face, *mesh_faceadr, *mesh_facenum, *hfield_nrow, *hfield_ncol, *hfield_adr;
};

// host: the argument checks of the geom arrays (the entry point's name goes into the message) ...
inline int check_geom_args(const char* who, const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm) {
  const std::string w(who);
  if (rm->ngeom != m->ngeom) return set_last_error(-4, (w + ": ray model ngeom differs from the model's").c_str());
  if (m->ngeom > 0 && (!rm->geom_group || !rm->geom_matid || !rm->geom_rgba || rm->geom_rgba_nb < 1 || !d->geom_xpos || !d->geom_xmat))
    return set_last_error(-1, (w + ": null geom array").c_str());
  if (rm->nmat > 0 && (!rm->mat_rgba || rm->mat_rgba_nb < 1)) return set_last_error(-1, (w + ": null mat_rgba").c_str());
  if (rm->nmeshface > 0 && (!rm->mesh_face || !rm->mesh_faceadr || !rm->mesh_facenum)) return set_last_error(-1, (w + ": null mesh face array").c_str());
  return 0;
}

// ... and the block filled from the model, the data and the ray model (the draw rule's fields are the caller's)
inline void fill_geom_args(GeomArgs& a, const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm) {
  a.ngeom = m->ngeom;
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
}

// the mesh BVHs of a render context (mjw_bvh_t; bvh.py has the layout).  A block of its own, read only by
// the kernels built with BVH = true (the others get it zeroed and never load it), so that GeomArgs stays as it is.
struct BvhArgs {
  int nnode, ntri, nmesh, min_faces;  // min_faces: meshes with fewer faces keep the face loop
  const float* node;  // (nnode, 8): box min 3, box max 3, two ints
  const int* tri;     // (ntri,) face ids local to the mesh, grouped by leaf
  const int* adr;     // (nmesh, 4): first node, nodes, first tri, depth
};
constexpr int BVH_LEAF = 4;     // triangles per leaf at the most (bvh.py BVH_LEAF)
constexpr int BVH_STACK = 64;   // traversal stack entries: one per lane of a VGPR; the trees have at most 32 levels
constexpr int BVH_AXIS_SHIFT = 29;

// host: the one refusal of a null table that the entry `who` requires ("<who>: null <what>", -1)
inline int refuse_null(const char* who, const char* what) { return set_last_error(-1, (std::string(who) + ": null " + what).c_str()); }

// host: whether a call with this bvh (not null: the entries refuse that) walks the trees (1), runs the face loop (0),
// or is refused (< 0)
inline int check_bvh_args(const char* who, const mjw_model_t* m, const mjw_ray_model_t* rm, const mjw_bvh_t* bvh, BvhArgs& bv) {
  const std::string w(who);
  if (bvh->nmesh != m->nmesh || bvh->ntri != rm->nmeshface) return set_last_error(-4, (w + ": the bvh was built for another model (nmesh / nmeshface)").c_str());
  if (bvh->nnode < 0 || bvh->leaf_size > BVH_LEAF || bvh->max_depth > 32) return set_last_error(-4, (w + ": bvh nnode / leaf_size / max_depth out of range").c_str());
  if (rm->nmeshface <= 0 || m->nmesh <= 0 || bvh->nnode == 0 || m->mesh_vert_nb > 1) return 0;
  if (!bvh->node || !bvh->tri || !bvh->adr) return set_last_error(-1, (w + ": null bvh table").c_str());
  bv.nnode = bvh->nnode; bv.ntri = bvh->ntri; bv.nmesh = bvh->nmesh; bv.min_faces = bvh->min_faces;
  bv.node = bvh->node; bv.tri = bvh->tri; bv.adr = bvh->adr;
  return 1;
}

// host: a runtime flag as a compile-time constant.  f is a generic lambda and receives std::true_type or std::false_type;
// nested once per flag, the innermost body names one instantiation by the flags themselves, so that the launchers hold
// one launch each and no table of instantiations that could be indexed wrongly.
template <class F>
inline void with_flag(bool on, F&& f) {
  if (on)
    f(std::true_type{});
  else
    f(std::false_type{});
}

__device__ __forceinline__ const float* row(const float* p, int nb, long cnt, int w) { return nb <= 1 ? p : p + (long)(w % nb) * cnt; }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// stages geoms g0 .. g0 + n of world wid (the caller puts the barriers around it)
template <int NT>
__device__ __forceinline__ void stage_chunk(const GeomArgs& a, int wid, int g0, int n, float* recs) {
  const float* size_w = row(a.geom_size, a.size_nb, (long)a.ngeom * 3, wid);
  const float* aabb_w = row(a.geom_aabb, a.aabb_nb, (long)a.ngeom * 6, wid);
  const float* rgba_w = row(a.geom_rgba, a.rgba_nb, (long)a.ngeom * 4, wid);
  const float* matrgba_w = row(a.mat_rgba, a.matrgba_nb, (long)a.nmat * 4, wid);
  const float* xpos_w = a.geom_xpos + (long)wid * a.ngeom * 3;
  const float* xmat_w = a.geom_xmat + (long)wid * a.ngeom * 9;
  for (int k = threadIdx.x; k < n; k += NT) {
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
    bool elim;
    if (a.draw_rule == 0) {
      elim = matid < 0 ? rgba_w[4 * g + 3] == 0.0f : (matid < a.nmat && matrgba_w[4 * matid + 3] == 0.0f);
      if (!a.flg_static && a.body_weldid[body] == 0) elim = true;
      if (a.group_mask >= 0 && !((a.group_mask >> min(5, max(0, a.geom_group[g]))) & 1)) elim = true;
    } else {
      const int grp = a.geom_group[g];
      elim = grp < 0 || grp > 31 || !((a.draw_groups >> grp) & 1u);
    }
    int* ri = reinterpret_cast<int*>(rec);
    ri[R_TYPE] = a.geom_type[g];
    ri[R_DATA] = a.geom_dataid[g];
    ri[R_BODY] = body;
    ri[R_ELIM] = elim ? 1 : 0;
  }
}

// The mesh's BVH walked by the whole wave in place of the face loop; the result is bitwise the face loop's (the
// nearest triangle of the mesh, the lowest face id among equal distances: x, nl).
//
// The walk is wave-uniform: one node at a time, read through uniform addresses, and one traversal stack for the wave
// kept in a VGPR (entry i in lane i: a push is a select on the lane id, a pop a v_readlane at a uniform index).  A node
// is entered when any candidate lane's ray meets its box no farther than that lane's limit: its nearest triangle of
// this mesh so far, or `best`, the nearest geom so far, beyond which a hit is dropped anyway.  An inner node sends
// the walk to the child on the side the first such lane's ray comes from and pushes the other.
//
// The slab test is conservative with respect to ray_triangle.  That routine accepts a ray that passes a triangle
// within rounding, a few ulp of the distance D between the ray's origin and the triangle; the box is grown by
// 1e-5 (|lp|_1 + the root box's largest coordinates), more than ten times that, on every side.  A direction
// component of (relative) size under 1e-12 is treated as zero: that axis then only asks whether the origin lies in
// the grown slab, and no 0 * inf is formed.  The entry distance is compared after a cut of 2^-10: ray_triangle's
// distance carries a relative error of about 1e-7 / sin(grazing angle), so the comparison stays on the safe side
// down to grazing angles of 1e-4 rad.  ANYHIT: a lane leaves the walk at its first hit under `best`.
//
// The walk is one routine for every kind of tree (bvh_walk).  `nodes` is the static node table of the tree, read for
// its two ints; a source says where a node's box lies and how a leaf item becomes three points:
//   src.box(node)            six floats, the minimum and the maximum (node 0: the root, which also sets the padding)
//   src.points(f, p0, p1, p2) the triangle of item f; false: there is none (an id outside its table)
// A mesh's boxes are the static table's own and its points the vertices mesh_face names (MeshSrc); a flex's boxes are
// this world's refit rows and its points are made on the fly (mjw_flexrender.h FlexSrc).

// the reciprocal direction of a ray for the slab test; a component under 1e-12 of the largest counts as zero
struct RaySlab {
  float inv[3];
  bool par[3];
};
__device__ __forceinline__ void ray_slab(const float* lv, RaySlab& s) {
  const float vmax = fmaxf(fabsf(lv[0]), fmaxf(fabsf(lv[1]), fabsf(lv[2])));
  for (int i = 0; i < 3; i++) {
    s.par[i] = !(fabsf(lv[i]) > 1e-12f * vmax);
    s.inv[i] = s.par[i] ? 0.0f : 1.0f / lv[i];
  }
}
// the padding of the slab test for a ray from lp into a tree (or a box) whose outermost box is `root`
__device__ __forceinline__ float slab_pad(const float* root, const float* lp) {
  float pad = fabsf(lp[0]) + fabsf(lp[1]) + fabsf(lp[2]);
  for (int i = 0; i < 3; i++) pad += fmaxf(fabsf(root[i]), fabsf(root[3 + i]));
  return pad * 1e-5f + 1e-30f;
}
// does the ray meet the box nd (minimum, maximum) grown by pad, and where does it enter (tmin >= 0)
__device__ __forceinline__ bool slab_test(const float* nd, float pad, const float* lp, const RaySlab& s, float& tmin) {
  float tmax = MJW_MAXVAL;
  tmin = 0.0f;
  for (int i = 0; i < 3; i++) {
    const float a = nd[i] - pad - lp[i], b = nd[3 + i] + pad - lp[i];  // a <= 0 <= b: the origin is in the slab
    float t0, t1;
    if (s.par[i]) {
      const bool in = a <= 0.0f && b >= 0.0f;
      t0 = in ? -MJW_MAXVAL : MJW_MAXVAL;
      t1 = in ? MJW_MAXVAL : -MJW_MAXVAL;
    } else {
      t0 = fminf(a * s.inv[i], b * s.inv[i]);
      t1 = fmaxf(a * s.inv[i], b * s.inv[i]);
    }
    tmin = fmaxf(tmin, t0);
    tmax = fminf(tmax, t1);
  }
  return tmin <= tmax;
}

struct MeshSrc {
  const float* nodes;  // the mesh's first node
  const float* vert;   // the mesh's first vertex
  const int* face;     // the mesh's first face
  __device__ __forceinline__ const float* box(int node) const { return nodes + 8 * node; }
  __device__ __forceinline__ bool points(int f, float* p0, float* p1, float* p2) const {
    const int* idx = face + 3 * (long)f;
    const float *v0 = vert + 3 * idx[0], *v1 = vert + 3 * idx[1], *v2 = vert + 3 * idx[2];
    for (int i = 0; i < 3; i++) {
      p0[i] = v0[i];
      p1[i] = v1[i];
      p2[i] = v2[i];
    }
    return true;
  }
};

template <bool ANYHIT, class Src>
__device__ __forceinline__ float bvh_walk(const Src& src, const float* nodes, int nnode, const int* tri, int nface, bool cand,
                                          const float* lp, const float* lv, const float* b0, const float* b1, float best, float* nl,
                                          int* face = nullptr) {
  float x = -1.0f;
  RaySlab slab;
  ray_slab(lv, slab);
  const float pad = slab_pad(src.box(0), lp);

  int bf = 0x7fffffff;  // the face of x
  const int lane = (int)(threadIdx.x & 63u);
  int stack = 0, sp = 0, node = 0;
  for (;;) {
    const int* nd = reinterpret_cast<const int*>(nodes + 8 * node);
    const int ia = uni(nd[6]), ib = uni(nd[7]);
    float tmin;
    const bool in = slab_test(src.box(node), pad, lp, slab, tmin);
    const float lim = x >= 0.0f ? fminf(x, best) : best;
    const bool go = cand && in && tmin * 0.9990234375f <= lim;
    const unsigned long long mask = __ballot(go);
    if (mask) {
      if (ib <= 0) {  // a leaf: its triangles, by their original face ids
        const int cnt = min(-ib, BVH_LEAF);
        if (ia >= 0 && ia <= nface - cnt) {
          for (int i = 0; i < cnt; i++) {
            const int f = uni(tri[ia + i]);
            if ((unsigned)f >= (unsigned)nface) continue;
            float n[3], p0[3], p1[3], p2[3];
            if (!src.points(f, p0, p1, p2)) continue;
            const float sol = ray_triangle(p0, p1, p2, lp, lv, b0, b1, n);
            if (sol >= 0.0f && (x < 0.0f || sol < x || (sol == x && f < bf))) {
              x = sol;
              bf = f;
              nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
            }
          }
          if (ANYHIT) cand = cand && !(x >= 0.0f && x < best);
        }
      } else {
        const int axis = ib >> BVH_AXIS_SHIFT;
        int l = ia, r = ib & ((1 << BVH_AXIS_SHIFT) - 1);
        // children lie after their parent, so a walk over any table ends
        if (l > node && l < nnode && r > node && r < nnode) {
          const float dsel = axis == 0 ? lv[0] : (axis == 1 ? lv[1] : lv[2]);
          const int first = uni((int)__ffsll((long long)mask) - 1);
          const float dv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dsel), first));
          if (dv < 0.0f) {
            const int t = l;
            l = r;
            r = t;
          }
          if (sp < BVH_STACK) {  // (never full: at most one entry per level)
            stack = lane == sp ? r : stack;
            sp++;
          }
          node = l;
          continue;
        }
      }
    }
    if (sp == 0) break;
    sp--;
    node = uni(__builtin_amdgcn_readlane(stack, sp));
  }
  if (face) *face = x >= 0.0f ? bf : -1;  // (textured shading asks which face; every other caller passes none)
  return x;
}

template <bool ANYHIT>
__device__ __forceinline__ float mesh_bvh(const BvhArgs& bv, int mesh, const float* vert, const int* face, int nface, bool cand,
                                          const float* lp, const float* lv, const float* b0, const float* b1, float best, float* nl,
                                          int* face_out) {
  if (face_out) *face_out = -1;
  if (mesh >= bv.nmesh) return -1.0f;  // (uniform, like every test of the tables below: a table that does not fit hits nothing)
  const int* adr = bv.adr + 4 * (long)mesh;
  const int nadr = uni(adr[0]), nnode = uni(adr[1]), triadr = uni(adr[2]);
  if (nadr < 0 || nnode < 1 || nadr > bv.nnode - nnode || triadr < 0 || triadr > bv.ntri - nface) return -1.0f;  // (uniform)
  const float* nodes = bv.node + 8 * (long)nadr;
  return bvh_walk<ANYHIT>(MeshSrc{nodes, vert, face}, nodes, nnode, bv.tri + triadr, nface, cand, lp, lv, b0, b1, best, nl, face_out);
}

// Every lane's ray (pnt, vec; world frame) against the n staged geoms g0 ..: a hit nearer than `best` (strict
// `<`, so equal distances stay with the lowest geom id) replaces best / bid / bn (world-frame normal).  Lanes
// with !active, and geoms of body excl, are left alone.  ANYHIT: a lane that has a hit (bid >= 0) stops looking,
// so with best preset to a distance limit the result says only whether anything lies nearer than the limit.
// BVH: meshes of at least bv.min_faces faces are walked through their BVH (bv) in place of the face loop.
template <bool ANYHIT, bool BVH>
__device__ __forceinline__ void trace_chunk(const GeomArgs& a, const BvhArgs& bv, int wid, const float* recs, int g0, int n, bool active,
                                            int excl, const float* pnt, const float* vec, float& best, int& bid, float* bn) {
  for (int k = 0; k < n; k++) {
    const float* rec = recs + k * RECW;
    const int* ri = reinterpret_cast<const int*>(rec);
    if (uni(ri[R_ELIM])) continue;  // eliminated for every ray of the workgroup
    const int type = uni(ri[R_TYPE]);
    bool cand = active && ri[R_BODY] != excl;
    if (ANYHIT) cand = cand && bid < 0;
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
      if (BVH && f1 - f0 >= bv.min_faces) {  // (uniform)
        if (f0 < 0 || f1 < f0) continue;
        x = mesh_bvh<ANYHIT>(bv, mesh, vert, a.mesh_face + 3 * (long)f0, f1 - f0, cand, lp, lv, b0, b1, best, nl, nullptr);
      } else {
        for (int f = f0; f < f1; f++) {
          const int* idx = a.mesh_face + 3 * (long)f;
          float n[3];
          const float sol = ray_triangle(vert + 3 * idx[0], vert + 3 * idx[1], vert + 3 * idx[2], lp, lv, b0, b1, n);
          if (sol >= 0.0f && (x < 0.0f || sol < x)) {
            x = sol;
            nl[0] = n[0]; nl[1] = n[1]; nl[2] = n[2];
          }
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

// The whole loop: every chunk of world wid staged in `recs` (RAY_CHUNK * RECW floats of LDS) and traced.  Every
// thread of the workgroup must call it (it holds barriers); a wave without an active lane skips the tracing.
// staged: the model fits one chunk and an earlier call of this workgroup left it in `recs`.
template <int NT, bool ANYHIT, bool BVH>
__device__ __forceinline__ void geom_loop(const GeomArgs& a, const BvhArgs& bv, int wid, float* recs, bool staged, bool active, int excl,
                                          const float* pnt, const float* vec, float& best, int& bid, float* bn) {
  for (int g0 = 0; g0 < a.ngeom; g0 += RAY_CHUNK) {
    const int n = min(RAY_CHUNK, a.ngeom - g0);
    if (!staged) {
      __syncthreads();  // the previous chunk is consumed
      stage_chunk<NT>(a, wid, g0, n, recs);
      __syncthreads();
    }
    if (__any(active)) trace_chunk<ANYHIT, BVH>(a, bv, wid, recs, g0, n, active, excl, pnt, vec, best, bid, bn);
  }
}

}  // namespace ray
}  // namespace mjw
