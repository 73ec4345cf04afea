// mjw_render.hip -- batched camera rendering: segmentation, planar depth and shaded RGB images of a model's
// cameras (mjw_render; mujoco_warp/_src/render.py `render`, render_util.py:67-125 `compute_ray`).
//
// Mapping: one workgroup serves one world, one rendered camera and a 16 x 16 tile of its pixels; each of the
// four waves owns an 8 x 8 block of the tile, so the rays of a wave stay close together and the wave-wide
// ball / box culling of the shared geom loop (geom_loop, mjw_ray.h) skips most geoms.  When every rendered
// camera has at most 64 pixels the workgroup is one wave and covers a whole image, pixel = lane.  A device
// table per render context maps the tile index to the camera and the tile's origin.  The rays are made in the
// kernel from the camera frames the last position stage left and the per-world camera parameters; they never
// exist in memory.  The kernel writes every pixel of every enabled output, background included.
//
// Shading (render.py:680-769, 410-512): hemispheric ambient plus the active lights; with shadows, one any-hit
// pass of the geom loop per shadow-casting light from the hit point towards the light, traced only by the
// waves in which some lane faces the light.  Lights are read through wave-uniform addresses.
//
// Flexes (mjw_render_flex; FLEX = true): after the geom loop every ray goes through flex_loop (mjw_flexrender.h), for
// the first hit and for each shadow ray; a flex pixel has segmentation -2, the colour flex_rgba and no material.
//
// One kernel, render_kernel<NT, BVH, FLEX, TEX>, serves the four entries (mjw_render, _bvh, _flex, _tex): render_launch
// turns "the context has trees that serve this call / flexes / textures" into the three flags, NT is 64 or 256.
#include "mjw_common.h"
#include "mjw_ray.h"
#include "mjw_flexrender.h"

namespace mjw {
namespace ray {

struct RenderArgs {
  GeomArgs g;
  int nworld, ntile, nrender, ncam, nlight, use_shadows, fovy_nb, sensor_nb, intr_nb, pad_;
  long rgb_ld, depth_ld, seg_ld;
  const float *cam_xpos, *cam_xmat, *light_xpos, *light_xdir, *cam_fovy, *cam_sensorsize, *cam_intrinsic;
  const int *cam_id_map, *cam_res, *rgb_adr, *depth_adr, *seg_adr, *tile;
  const int *light_type, *light_active, *light_castshadow;
  int* rgb;
  float* depth;
  int* seg;
};

constexpr unsigned BACKGROUND = 255u << 24 | 25u << 16 | 25u << 8 | 51u;  // (0.1, 0.1, 0.2, 1) * 255, truncated

// render_util.py:67-125 at znear = 1 (it cancels in the normalisation): the direction of pixel (px, py) of a
// W x H image in the camera frame
__device__ __forceinline__ void pixel_ray(float fovy, const float* sensorsize, const float* intrinsic, int W, int H, int px, int py,
                                          float* local) {
  const float aspect = (float)W / (float)H;
  float left, right, top, bottom;
  float sensor_h = sensorsize[1];
  if (sensor_h != 0.0f) {
    const float fx = intrinsic[0], fy = intrinsic[1], cx = intrinsic[2], cy = intrinsic[3];
    float sensor_w = sensorsize[0];
    const float sensor_aspect = sensor_w / sensor_h;
    if (aspect > sensor_aspect)
      sensor_h = sensor_w / aspect;
    else if (aspect < sensor_aspect)
      sensor_w = sensor_h * aspect;
    const float ifx = 1.0f / fx, ify = 1.0f / fy;
    left = -ifx * (sensor_w * 0.5f - cx);
    right = ifx * (sensor_w * 0.5f + cx);
    top = ify * (sensor_h * 0.5f - cy);
    bottom = -ify * (sensor_h * 0.5f + cy);
  } else {
    const float half_h = tanf(0.5f * fovy * 0.017453292519943295f);
    const float half_w = half_h * aspect;
    left = -half_w; right = half_w; top = half_h; bottom = -half_h;
  }
  const float u = ((float)px + 0.5f) / (float)W, v = ((float)py + 0.5f) / (float)H;
  local[0] = left + (right - left) * u;
  local[1] = top + (bottom - top) * v;
  local[2] = -1.0f;
  normalize3(local);
}

// ---- textures (mjw_render_tex; TEX = true) ---------------------------------------------------------------------------
//
// The base colour of a pixel on a plane, or on a mesh that has texture coordinates, is multiplied by a bilinear sample
// of the 2D texture its material names in role 1 (render.py:43-84 `sample_texture`, 694-717).  The tables are those
// of mjw_texture_t; an id or address outside its table means "no texture", so a table that does not fit samples nothing.
struct TexArgs {
  int ntex, ntexdata, nmat, nmesh, ntexcoord, nmeshface, texid_nb, texrep_nb;
  const int* mat_texid;        // (texid_nb, nmat, 10)
  const float* mat_texrepeat;  // (texrep_nb, nmat, 2)
  const int *tex_data, *tex_adr, *tex_width, *tex_height;
  const float* mesh_texcoord;
  const int *mesh_texcoordadr, *mesh_facetexcoord;
};

// the texel (x, y) of a texture as three floats in [0, 1]; x, y already inside the texture
__device__ __forceinline__ void texel(const int* data, int W, int x, int y, float* c) {
  const unsigned w = (unsigned)data[(long)y * W + x];
  c[0] = (float)(w & 255u) * (1.0f / 255.0f);
  c[1] = (float)((w >> 8) & 255u) * (1.0f / 255.0f);
  c[2] = (float)((w >> 16) & 255u) * (1.0f / 255.0f);
}

// bilinear sample with repeat addressing: s = frac(uv * repeat), texel centres at (i + 0.5) / W, fp32 weights
__device__ __forceinline__ void tex_sample(const int* data, int W, int H, const float* uv, const float* rep, float* c) {
  float s0 = uv[0] * rep[0], s1 = uv[1] * rep[1];
  s0 -= floorf(s0);
  s1 -= floorf(s1);
  const float x = s0 * (float)W - 0.5f, y = s1 * (float)H - 0.5f;
  // floor(x) lies in -1 .. W - 1; the clamp also catches a uv that is not finite
  const float xf = fminf(fmaxf(floorf(x), -1.0f), (float)(W - 1)), yf = fminf(fmaxf(floorf(y), -1.0f), (float)(H - 1));
  float wx = x - xf, wy = y - yf;
  wx = wx >= 0.0f && wx <= 1.0f ? wx : 0.0f;
  wy = wy >= 0.0f && wy <= 1.0f ? wy : 0.0f;
  const int x0 = xf < 0.0f ? W - 1 : (int)xf, y0 = yf < 0.0f ? H - 1 : (int)yf;
  const int x1 = x0 + 1 < W ? x0 + 1 : 0, y1 = y0 + 1 < H ? y0 + 1 : 0;
  float t00[3], t10[3], t01[3], t11[3];
  texel(data, W, x0, y0, t00);
  texel(data, W, x1, y0, t10);
  texel(data, W, x0, y1, t01);
  texel(data, W, x1, y1, t11);
  for (int i = 0; i < 3; i++)
    c[i] = (1.0f - wy) * ((1.0f - wx) * t00[i] + wx * t10[i]) + wy * ((1.0f - wx) * t01[i] + wx * t11[i]);
}

// Multiplies base by the texel colour of the lane's first hit (geom bid at distance best along pnt + x vec) where the
// rules above give it one.  Every lane of the wave must call it: the face of a mesh hit is found again here, one hit
// mesh geom of the wave at a time, by the walk or the face loop that found it in trace_chunk (the nearest triangle,
// the lowest face id among equal distances), so the kernels without textures carry no face id.  The block is a second
// copy of trace_chunk's on purpose: one shared routine gave the same bits but slower textured launches.
// recs: the staged records of the model's only chunk (ngeom <= RAY_CHUNK: the primary rays left them in LDS), else null.
template <bool BVH>
__device__ __forceinline__ void tex_shade(const GeomArgs& g, const BvhArgs& bv, const TexArgs& tx, int wid, const float* recs, bool on, int bid,
                                          int matid, const float* pnt, const float* vec, float best, float* base) {
  // the hit geom's type and the ray in its frame, read before the texture's header so that the loads do not queue
  // behind it: from the staged record where there is one (the floats trace_chunk mapped the ray with), else from the arrays
  int gtype = -1;
  float lp[3] = {0.0f, 0.0f, 0.0f}, lv[3] = {0.0f, 0.0f, -1.0f}, uv[2] = {0.0f, 0.0f};
  if (on && matid >= 0) {
    if (recs) {
      const float* rec = recs + bid * RECW;
      gtype = reinterpret_cast<const int*>(rec)[R_TYPE];
      ray_map(rec + R_POS, rec + R_MAT, pnt, vec, lp, lv);
    } else {
      gtype = g.geom_type[bid];
      ray_map(g.geom_xpos + ((long)wid * g.ngeom + bid) * 3, g.geom_xmat + ((long)wid * g.ngeom + bid) * 9, pnt, vec, lp, lv);
    }
  }
  int texid = -1;
  float rep[2] = {1.0f, 1.0f};
  if (on && matid >= 0 && matid < g.nmat && matid < tx.nmat) {
    texid = tx.mat_texid[((long)(wid % tx.texid_nb) * tx.nmat + matid) * 10 + 1];
    const float* r = tx.mat_texrepeat + ((long)(wid % tx.texrep_nb) * tx.nmat + matid) * 2;
    rep[0] = r[0];
    rep[1] = r[1];
  }
  int adr = -1, W = 0, H = 0;
  if (texid >= 0 && texid < tx.ntex) {
    adr = tx.tex_adr[texid];
    W = tx.tex_width[texid];
    H = tx.tex_height[texid];
  }
  const bool tex = adr >= 0 && W >= 1 && H >= 1 && (long)adr + (long)W * (long)H <= (long)tx.ntexdata;
  const int type = tex ? gtype : -1;
  const float hl[3] = {lp[0] + best * lv[0], lp[1] + best * lv[1], lp[2] + best * lv[2]};  // the hit in the geom's frame
  bool have = type == RG_PLANE;
  if (have) {
    uv[0] = hl[0];
    uv[1] = hl[1];
  }
  bool pending = type == RG_MESH;
  unsigned long long mask;
  while ((mask = __ballot(pending)) != 0ull) {
    const int gsel = uni(__builtin_amdgcn_readlane(bid, (int)__ffsll((long long)mask) - 1));
    const bool mine = pending && bid == gsel;
    pending = pending && !mine;
    const int mesh = uni(g.geom_dataid[gsel]);
    if (mesh < 0 || mesh >= g.nmesh || mesh >= tx.nmesh) continue;
    const int tadr = uni(tx.mesh_texcoordadr[mesh]);
    if (tadr < 0) continue;  // a mesh without texcoords keeps its base colour
    const float* vert = row(g.mesh_vert, g.vert_nb, (long)g.nmeshvert * 3, wid) + 3 * (long)g.mesh_vertadr[mesh];
    const int f0 = uni(g.mesh_faceadr[mesh]), f1 = min(f0 + uni(g.mesh_facenum[mesh]), g.nmeshface);
    if (f0 < 0 || f1 < f0) continue;
    float b0[3], b1[3], nl[3];
    ray_basis(lv, b0, b1);
    int face = -1;
    if (BVH && f1 - f0 >= bv.min_faces) {
      mesh_bvh<false>(bv, mesh, vert, g.mesh_face + 3 * (long)f0, f1 - f0, mine, lp, lv, b0, b1, MJW_MAXVAL, nl, &face);
    } else {
      float x = -1.0f;
      for (int f = f0; f < f1; f++) {
        const int* idx = g.mesh_face + 3 * (long)f;
        const float sol = ray_triangle(vert + 3 * idx[0], vert + 3 * idx[1], vert + 3 * idx[2], lp, lv, b0, b1, nl);
        if (sol >= 0.0f && (x < 0.0f || sol < x)) {
          x = sol;
          face = f - f0;
        }
      }
    }
    // per lane from here (no `continue`: the loop's ballot needs the whole wave back together)
    if (mine && face >= 0 && face < f1 - f0 && f0 + face < tx.nmeshface) {
      const int* idx = g.mesh_face + 3 * (long)(f0 + face);
      const int* ti = tx.mesh_facetexcoord + 3 * (long)(f0 + face);
      const long t0 = (long)tadr + ti[0], t1 = (long)tadr + ti[1], t2 = (long)tadr + ti[2];
      if (ti[0] >= 0 && ti[1] >= 0 && ti[2] >= 0 && t0 < tx.ntexcoord && t1 < tx.ntexcoord && t2 < tx.ntexcoord) {
        const float *v0 = vert + 3 * idx[0], *v1 = vert + 3 * idx[1], *v2 = vert + 3 * idx[2];
        const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
        const float d0[3] = {v0[0] - hl[0], v0[1] - hl[1], v0[2] - hl[2]}, d1[3] = {v1[0] - hl[0], v1[1] - hl[1], v1[2] - hl[2]};
        const float d2[3] = {v2[0] - hl[0], v2[1] - hl[1], v2[2] - hl[2]};
        float n[3], c0[3], c1[3];
        cross3(n, e1, e2);
        const float nn = dot3(n, n);
        if (nn > 0.0f) {  // barycentrics of the hit: signed sub-triangle areas over the triangle's
          cross3(c0, d1, d2);
          cross3(c1, d2, d0);
          const float w0 = dot3(n, c0) / nn, w1 = dot3(n, c1) / nn, w2 = 1.0f - w0 - w1;
          const float *u0 = tx.mesh_texcoord + 2 * t0, *u1 = tx.mesh_texcoord + 2 * t1, *u2 = tx.mesh_texcoord + 2 * t2;
          uv[0] = w0 * u0[0] + w1 * u1[0] + w2 * u2[0];
          uv[1] = w0 * u0[1] + w1 * u1[1] + w2 * u2[1];
          have = true;
        }
      }
    }
  }
  if (have) {
    float c[3];
    tex_sample(tx.tex_data + adr, W, H, uv, rep, c);
    for (int i = 0; i < 3; i++) base[i] *= c[i];
  }
}

template <int NT, bool BVH, bool FLEX, bool TEX>
__device__ __forceinline__ void render_body(const RenderArgs& a, const BvhArgs& bv, const FlexArgs& fx, const TexArgs& tx, float* recs) {
  const int tid = threadIdx.x;
  const int wid = blockIdx.x / a.ntile, t = blockIdx.x - wid * a.ntile;
  const int ci = a.tile[4 * t], x0 = a.tile[4 * t + 1], y0 = a.tile[4 * t + 2];
  if (ci < 0 || ci >= a.nrender || x0 < 0 || y0 < 0) return;  // (uniform over the workgroup)
  const int W = a.cam_res[2 * ci], H = a.cam_res[2 * ci + 1], cam = a.cam_id_map[ci];
  if (W < 1 || H < 1 || cam < 0 || cam >= a.ncam) return;
  int lx, ly;
  if (NT == 64) {  // the whole image of at most 64 pixels
    lx = tid % W;
    ly = tid / W;
  } else {  // wave w owns the 8 x 8 block (w & 1, w >> 1) of the tile
    const int wave = tid >> 6, lane = tid & 63;
    lx = (wave & 1) * 8 + (lane & 7);
    ly = (wave >> 1) * 8 + (lane >> 3);
  }
  const int px = x0 + lx, py = y0 + ly;
  const bool active = px < W && py < H;
  const int pxc = min(px, W - 1), pyc = min(py, H - 1);  // idle lanes follow a valid pixel and write nothing

  // the ray
  const float fovy = row(a.cam_fovy, a.fovy_nb, a.ncam, wid)[cam];
  const float* ss = row(a.cam_sensorsize, a.sensor_nb, (long)a.ncam * 2, wid) + 2 * cam;
  const float* in = row(a.cam_intrinsic, a.intr_nb, (long)a.ncam * 4, wid) + 4 * cam;
  float local[3], vec[3];
  pixel_ray(fovy, ss, in, W, H, pxc, pyc, local);
  const float* cp = a.cam_xpos + ((long)wid * a.ncam + cam) * 3;
  const float* cm = a.cam_xmat + ((long)wid * a.ncam + cam) * 9;
  const float pnt[3] = {cp[0], cp[1], cp[2]};
  rot_to_world(cm, local, vec);

  float best = MJW_MAXVAL, bn[3] = {0.0f, 0.0f, 0.0f};
  int bid = -1;
  geom_loop<NT, false, BVH>(a.g, bv, wid, recs, false, active, -1, pnt, vec, best, bid, bn);
  int fid = -1;  // the flex of the hit when a flex is nearer than every geom
  if (FLEX) flex_loop<false>(fx, wid, active, pnt, vec, best, fid, bn);
  const bool hit = bid >= 0 || fid >= 0;

  const long pix = (long)py * W + px;
  const int sadr = a.seg_adr[ci], dadr = a.depth_adr[ci], cadr = a.rgb_adr[ci];
  if (active && sadr >= 0 && sadr + pix < a.seg_ld) a.seg[(long)wid * a.seg_ld + sadr + pix] = fid >= 0 ? -2 : bid;
  if (active && dadr >= 0 && dadr + pix < a.depth_ld) a.depth[(long)wid * a.depth_ld + dadr + pix] = hit ? best * -local[2] : 0.0f;
  if (cadr < 0) return;  // (uniform over the workgroup)

  // shading: every thread goes through the light loop (the shadow pass holds barriers), a lane without a hit
  // takes no part in it
  const int gid = bid >= 0 ? bid : 0;
  const int matid = a.g.ngeom > 0 ? a.g.geom_matid[gid] : -1;
  const float* col = (matid >= 0 && matid < a.g.nmat) ? row(a.g.mat_rgba, a.g.matrgba_nb, (long)a.g.nmat * 4, wid) + 4 * matid
                                                       : row(a.g.geom_rgba, a.g.rgba_nb, (long)a.g.ngeom * 4, wid) + 4 * gid;
  float base[3] = {0.0f, 0.0f, 0.0f};
  if (FLEX && fid >= 0) {
    for (int i = 0; i < 3; i++) base[i] = fx.rgba[4 * fid + i];
  } else if (bid >= 0) {
    for (int i = 0; i < 3; i++) base[i] = col[i];
  }
  if (TEX) tex_shade<BVH>(a.g, bv, tx, wid, a.g.ngeom <= RAY_CHUNK ? recs : nullptr, active && bid >= 0 && fid < 0, bid, matid, pnt, vec, best, base);
  const float hp[3] = {pnt[0] + vec[0] * best, pnt[1] + vec[1] * best, pnt[2] + vec[2] * best};
  float n[3] = {bn[0], bn[1], bn[2]};
  if (!(dot3(n, n) > 0.0f)) { n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f; }
  normalize3(n);
  const float h = 0.5f * (n[2] + 1.0f);
  float res[3] = {0.5f * base[0] * (0.4f * h + 0.1f * (1.0f - h)), 0.5f * base[1] * (0.4f * h + 0.1f * (1.0f - h)),
                  0.5f * base[2] * (0.45f * h + 0.12f * (1.0f - h))};

  for (int l = 0; l < a.nlight; l++) {
    if (!a.light_active[l]) continue;
    const int type = a.light_type[l];
    const float* lpos = a.light_xpos + ((long)wid * a.nlight + l) * 3;
    const float* ldir = a.light_xdir + ((long)wid * a.nlight + l) * 3;
    float L[3], r = MJW_MAXVAL, att = 1.0f;
    if (type == 1) {  // directional
      L[0] = -ldir[0]; L[1] = -ldir[1]; L[2] = -ldir[2];
      normalize3(L);
    } else {
      L[0] = lpos[0] - hp[0]; L[1] = lpos[1] - hp[1]; L[2] = lpos[2] - hp[2];
      r = sqrtf(dot3(L, L));
      const float inv = r > 0.0f ? 1.0f / r : 0.0f;
      L[0] *= inv; L[1] *= inv; L[2] *= inv;
      att = 1.0f / (1.0f + 0.02f * r * r);
      if (type == 0) {  // spot
        float sd[3] = {ldir[0], ldir[1], ldir[2]};
        normalize3(sd);
        const float cs = -dot3(L, sd);
        att *= fminf(1.0f, fmaxf(0.0f, (cs - 0.85f) / (0.95f - 0.85f)));
      }
    }
    const float ndotl = hit ? fmaxf(0.0f, dot3(bn, L)) : 0.0f;
    float visible = 1.0f;
    if (a.use_shadows && a.light_castshadow[l]) {
      const float so[3] = {hp[0] + bn[0] * 1e-4f, hp[1] + bn[1] * 1e-4f, hp[2] + bn[2] * 1e-4f};
      float sbest = type == 1 ? 1e8f : r - 1e-3f, sn[3];
      int sid = -1;
      geom_loop<NT, true, BVH>(a.g, bv, wid, recs, a.g.ngeom <= RAY_CHUNK, active && ndotl > 0.0f, -1, so, L, sbest, sid, sn);
      if (FLEX) {
        int sfid = -1;
        flex_loop<true>(fx, wid, active && ndotl > 0.0f && sid < 0, so, L, sbest, sfid, sn);
        if (sfid >= 0) sid = 0;
      }
      if (sid >= 0) visible = 0.3f;
    }
    const float c = ndotl * att * visible;
    for (int i = 0; i < 3; i++) res[i] += base[i] * c;
  }

  if (active && cadr + pix < a.rgb_ld) {
    unsigned packed = BACKGROUND;
    if (hit) {
      unsigned byte[3];
      for (int i = 0; i < 3; i++) byte[i] = (unsigned)(int)(fminf(1.0f, fmaxf(0.0f, res[i])) * 255.0f);
      packed = 255u << 24 | byte[0] << 16 | byte[1] << 8 | byte[2];
    }
    a.rgb[(long)wid * a.rgb_ld + cadr + pix] = (int)packed;
  }
}

// The one render kernel.  BVH: the meshes are walked through the BVHs of the render context (bv), else face by face;
// FLEX: the flexes of the context (fx) are drawn too; TEX: planes and meshes take their textures (tx).  Every
// instantiation takes all four blocks: one whose flag is off is zeroed by the host and never loaded, and costs no register.
template <int NT, bool BVH, bool FLEX, bool TEX>
__global__ void __launch_bounds__(NT) render_kernel(const RenderArgs a, const BvhArgs bv, const FlexArgs fx, const TexArgs tx) {
  __shared__ float recs[RAY_CHUNK * RECW];
  render_body<NT, BVH, FLEX, TEX>(a, bv, fx, tx, recs);
}

// host: the checks of mjw_texture_t; 1: sample, 0: nothing to sample (the call is the one without textures), < 0: refused
static int check_tex_args(const mjw_model_t* m, const mjw_ray_model_t* rm, const mjw_texture_t* t, TexArgs& tx) {
  if (t->ntex < 0 || t->ntexdata < 0 || t->nmat < 0 || t->nmesh < 0 || t->ntexcoord < 0 || t->nmeshface < 0)
    return set_last_error(-4, "mjw_render_tex: negative count");
  if (t->mat_texid_nb < 1 || t->mat_texrepeat_nb < 1) return set_last_error(-4, "mjw_render_tex: mat_texid / mat_texrepeat batch size < 1");
  if (t->nmat != rm->nmat) return set_last_error(-4, "mjw_render_tex: nmat differs from the ray model's");
  if ((t->nmesh != 0 && t->nmesh != m->nmesh) || (t->nmeshface != 0 && t->nmeshface != rm->nmeshface))
    return set_last_error(-4, "mjw_render_tex: nmesh / nmeshface differ from the model's");
  if (t->nmat > 0 && (!t->mat_texid || !t->mat_texrepeat)) return set_last_error(-1, "mjw_render_tex: null mat_texid / mat_texrepeat");
  if (t->ntex > 0 && (!t->tex_adr || !t->tex_width || !t->tex_height)) return set_last_error(-1, "mjw_render_tex: null texture table");
  if (t->ntexdata > 0 && !t->tex_data) return set_last_error(-1, "mjw_render_tex: null tex_data");
  if ((t->nmesh > 0 && !t->mesh_texcoordadr) || (t->ntexcoord > 0 && !t->mesh_texcoord) || (t->nmeshface > 0 && !t->mesh_facetexcoord))
    return set_last_error(-1, "mjw_render_tex: null texcoord table");
  if (t->ntex == 0 || t->ntexdata == 0 || t->nmat == 0) return 0;
  tx.ntex = t->ntex; tx.ntexdata = t->ntexdata; tx.nmat = t->nmat; tx.nmesh = t->nmesh; tx.ntexcoord = t->ntexcoord; tx.nmeshface = t->nmeshface;
  tx.texid_nb = t->mat_texid_nb; tx.texrep_nb = t->mat_texrepeat_nb;
  tx.mat_texid = t->mat_texid; tx.mat_texrepeat = t->mat_texrepeat;
  tx.tex_data = t->tex_data; tx.tex_adr = t->tex_adr; tx.tex_width = t->tex_width; tx.tex_height = t->tex_height;
  tx.mesh_texcoord = t->mesh_texcoord; tx.mesh_texcoordadr = t->mesh_texcoordadr; tx.mesh_facetexcoord = t->mesh_facetexcoord;
  return 1;
}

}  // namespace ray
}  // namespace mjw

// The launch every entry below ends in; who: the entry's name for the messages about its own tables.  A null bvh, fr or
// tex means "absent": no walk, no flexes, no textures.  The entries refuse a null table their contract requires.
static int render_launch(const char* who, const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc,
                         const mjw_bvh_t* bvh, const mjw_flexrender_t* fr, const mjw_texture_t* tex, void* stream) {
  using namespace mjw::ray;
  if (!m || !d || !rm || !rc) return mjw::set_last_error(-1, "mjw_render: null model / data / ray model / render context");
  TexArgs tx;
  memset(&tx, 0, sizeof(tx));
  int textured = 0;
  if (tex && (textured = check_tex_args(m, rm, tex, tx)) < 0) return textured;
  BvhArgs bv;
  memset(&bv, 0, sizeof(bv));
  int walk = 0;
  if (bvh && (walk = check_bvh_args(who, m, rm, bvh, bv)) < 0) return walk;
  FlexArgs fx;
  memset(&fx, 0, sizeof(fx));
  int flex = 0;
  if (fr && (flex = check_flex_args(who, m, d, fr, fx)) < 0) return flex;
  if (rc->ntile < 0 || rc->nrender < 0) return mjw::set_last_error(-4, "mjw_render: ntile / nrender < 0");
  if (rc->ntile == 0 || d->nworld <= 0) return 0;
  if (rc->tile_threads != 64 && rc->tile_threads != 256) return mjw::set_last_error(-4, "mjw_render: tile_threads must be 64 or 256");
  if (!rc->cam_id_map || !rc->cam_res || !rc->rgb_adr || !rc->depth_adr || !rc->seg_adr || !rc->tile)
    return mjw::set_last_error(-1, "mjw_render: null camera / tile table");
  if ((rc->rgb_ld > 0 && !rc->rgb) || (rc->depth_ld > 0 && !rc->depth) || (rc->seg_ld > 0 && !rc->seg) || rc->rgb_ld < 0 || rc->depth_ld < 0 ||
      rc->seg_ld < 0)
    return mjw::set_last_error(-1, "mjw_render: null output array");
  if (m->ncam <= 0 || !d->cam_xpos || !d->cam_xmat || !m->cam_fovy || !m->cam_sensorsize || !m->cam_intrinsic)
    return mjw::set_last_error(-1, "mjw_render: null camera array");
  if (m->nlight > 0 && (!d->light_xpos || !d->light_xdir || !rc->light_type || !rc->light_active || !rc->light_castshadow))
    return mjw::set_last_error(-1, "mjw_render: null light array");
  if (int e = check_geom_args("mjw_render", m, d, rm)) return e;

  RenderArgs a;
  memset(&a, 0, sizeof(a));
  fill_geom_args(a.g, m, d, rm);
  a.g.draw_rule = 1;
  a.g.draw_groups = rc->group_mask;
  a.nworld = d->nworld; a.ntile = rc->ntile; a.nrender = rc->nrender; a.ncam = m->ncam; a.nlight = m->nlight;
  a.use_shadows = rc->use_shadows != 0;
  a.cam_xpos = d->cam_xpos; a.cam_xmat = d->cam_xmat; a.light_xpos = d->light_xpos; a.light_xdir = d->light_xdir;
  a.cam_fovy = m->cam_fovy; a.fovy_nb = m->cam_fovy_nb;
  a.cam_sensorsize = m->cam_sensorsize; a.sensor_nb = m->cam_sensorsize_nb;
  a.cam_intrinsic = m->cam_intrinsic; a.intr_nb = m->cam_intrinsic_nb;
  a.cam_id_map = rc->cam_id_map; a.cam_res = rc->cam_res; a.rgb_adr = rc->rgb_adr; a.depth_adr = rc->depth_adr; a.seg_adr = rc->seg_adr;
  a.tile = rc->tile;
  a.light_type = rc->light_type; a.light_active = rc->light_active; a.light_castshadow = rc->light_castshadow;
  a.rgb = rc->rgb; a.depth = rc->depth; a.seg = rc->seg;
  a.rgb_ld = rc->rgb_ld; a.depth_ld = rc->depth_ld; a.seg_ld = rc->seg_ld;

  hipStream_t s = (hipStream_t)stream;
  const long nblock = (long)a.nworld * a.ntile;
  if (nblock > 0x7fffffffL) return mjw::set_last_error(-2, "mjw_render: nworld x tiles exceeds the grid limit");
  with_flag(rc->tile_threads == 64, [&](auto small) {
    with_flag(walk != 0, [&](auto bvh_on) {
      with_flag(flex != 0, [&](auto flex_on) {
        with_flag(textured != 0, [&](auto tex_on) {
          constexpr int NT = decltype(small)::value ? 64 : 256;
          hipLaunchKernelGGL((render_kernel<NT, decltype(bvh_on)::value, decltype(flex_on)::value, decltype(tex_on)::value>),
                             dim3((unsigned)nblock), dim3(NT), 0, s, a, bv, fx, tx);
        });
      });
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mjw::set_last_error((int)e, hipGetErrorString(e));
  return 0;
}

// The entries.  A null table that an entry requires is refused where it always was, after the model pointers, which are
// the launcher's to refuse; mjw_render_flex's null fr now comes before the launcher looks into the bvh.
extern "C" int mjw_render(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, void* stream) {
  return render_launch("mjw_render", m, d, rm, rc, nullptr, nullptr, nullptr, stream);
}

extern "C" int mjw_render_bvh(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc,
                              const mjw_bvh_t* bvh, void* stream) {
  if (m && d && rm && rc && !bvh) return mjw::ray::refuse_null("mjw_render_bvh", "bvh");
  return render_launch("mjw_render_bvh", m, d, rm, rc, bvh, nullptr, nullptr, stream);
}

extern "C" int mjw_render_flex(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc,
                               const mjw_bvh_t* bvh, const mjw_flexrender_t* fr, void* stream) {
  if (m && d && rm && rc && !fr) return mjw::ray::refuse_null("mjw_render_flex", "flex render tables");
  return render_launch("mjw_render_flex", m, d, rm, rc, bvh, fr, nullptr, stream);
}

extern "C" int mjw_sizeof_texture(void) { return (int)sizeof(mjw_texture_t); }

extern "C" int mjw_render_tex(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, const mjw_bvh_t* bvh,
                              const mjw_flexrender_t* fr, const mjw_texture_t* tex, void* stream) {
  if (m && d && rm && rc && !tex) return mjw::ray::refuse_null("mjw_render_tex", "texture tables");
  return render_launch("mjw_render_tex", m, d, rm, rc, bvh, fr, tex, stream);
}
