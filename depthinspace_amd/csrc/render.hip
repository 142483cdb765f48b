// Track rendering (include/dis_hip.h, section "track rendering"): a triangle-mesh scene seen by tl cameras -> im, ambient, disp and
// the exact rigid flow of every visible surface point for all ordered frame pairs, with occlusion and projector shadows.
//
// Two launches, no allocation, no float atomics, bit-identical from run to run:
//   render_setup_kernel   one thread per (frame, triangle): the triangle in the camera frame (fp64 transform, rounded once to fp32, so
//                         a vertex shared by two triangles has the same bits in both), its unit plane (n, d0 = n . A, formed in fp64),
//                         and two conservative screen boxes: where it lies in the camera image and, shifted by baseline f / z in x,
//                         where it lies in the projector image.  A triangle with a vertex nearer than RND_NEAR is not clipped: its
//                         boxes are the whole image.  A triangle wholly behind the camera plane, or of zero area, gets empty boxes.
//   render_cast_kernel    one workgroup per 16 x 16 tile and frame.  The workgroup walks the boxes of its frame 256 at a time, keeps
//                         the ones that meet the tile and compacts their indices - in increasing order, by ballot and prefix count -
//                         into an LDS list; whenever the list is nearly full, and at the end, every pixel of the tile tests the listed
//                         triangles.  Nearest camera depth wins; the list is in index order and the comparison is strict, so on equal
//                         depth the lower index wins whatever the chunking.
//                         Shadows: rectification puts a shadow ray into one image row of the camera AND makes it a single point of the
//                         projector image (u - disp, v).  So the second walk keeps the triangles whose rows meet the tile and whose
//                         projector box meets the tile's range of u - disp (LDS integer min / max over the hit pixels), and a pixel
//                         tests them with the same routine as seen from the projector centre.
//
// The ray-triangle test is the sheared edge-function form (the ray has z = 1 in its own frame, so a vertex is sheared by its depth):
// the edge function of a shared edge is computed from the same two vertices in both triangles and, without contraction, is exactly the
// negative of the other's, so no ray slips between two triangles of a consistently indexed mesh.  This rests on -ffp-contract=off (the
// Makefile's CXXFLAGS): a fused a * b - c * d rounds the two products differently and the two edge functions stop being negatives.
// rnd_hit() repeats the setting with a pragma, so that a per-file flag change cannot take the guarantee away.  A zero edge function
// counts as inside for both; the depth tie-break decides.  The hit depth comes from the plane, z = d0 / (n . ray), not from the edge
// functions.
#include "track_common.h"
#include <math.h>

#define RND_TILE 16
#define RND_BLOCK 256
#define RND_CAP 1024          // LDS candidate list (ints); flushed when fewer than RND_BLOCK slots are left
#define RND_MAX_NF (1 << 20)
#define RND_MAX_NV (1 << 24)
#define RND_NEAR 0.05         // camera-frame depth below which a vertex makes its triangle's boxes the whole image
#define RND_BOX_PAD 0.5       // pixels added to every side of a projected box
#define RND_SHADOW_EPS 1e-4f  // an occluder counts for ray parameters in (eps, 1 - eps); the hit triangle itself never does
#define RND_KA 0.5f
#define RND_KD 1.5f
#define RND_BOX_MIN (-32768)
#define RND_BOX_MAX 32767

struct RndCam {
  float fx, fy, cx, cy, baseline, blend;
};
struct RndOutDev {
  float *im, *ambient, *disp, *flow, *lit;
  int* tri_id;
};

__device__ __forceinline__ int rnd_pack(int lo, int hi) { return (int)((unsigned)(lo & 0xffff) | ((unsigned)hi << 16)); }
__device__ __forceinline__ int rnd_lo(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int rnd_hi(int v) { return v >> 16; }
__device__ __forceinline__ int rnd_box_lo(double x) {
  x = floor(x - RND_BOX_PAD);
  return (int)fmin(fmax(x, (double)RND_BOX_MIN), (double)RND_BOX_MAX);
}
__device__ __forceinline__ int rnd_box_hi(double x) {
  x = ceil(x + RND_BOX_PAD);
  return (int)fmin(fmax(x, (double)RND_BOX_MIN), (double)RND_BOX_MAX);
}

// tri: 4 float4 per (frame, triangle): (Ax, Ay, Az, nx) (Bx, By, Bz, ny) (Cx, Cy, Cz, nz) (d0, albedo, 0, 0)
// box: int4 per (frame, triangle): camera x range, row range, projector x range (pairs of int16), 0
__global__ void __launch_bounds__(RND_BLOCK) render_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 const float* __restrict__ albedo, const int nv, const int nf,
                                                                 const float* __restrict__ R, const float* __restrict__ t, const RndCam cam,
                                                                 const int tl, const int h, const int w, float4* __restrict__ tri,
                                                                 int4* __restrict__ box) {
  const long total = (long)tl * nf;
  for (long e = (long)blockIdx.x * RND_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * RND_BLOCK) {
    const int f = (int)(e / nf), k = (int)(e % nf);
    const float* Rf = R + f * 9;
    const float* tf = t + f * 3;
    double P[3][3];
    for (int v = 0; v < 3; ++v) {
      int idx = faces[3L * k + v];
      idx = idx < 0 ? 0 : (idx >= nv ? nv - 1 : idx);   // (an index outside the vertex array is clamped, never followed)
      const double X0 = verts[3L * idx], X1 = verts[3L * idx + 1], X2 = verts[3L * idx + 2];
      for (int r = 0; r < 3; ++r)
        P[v][r] = ((double)Rf[3 * r] * X0 + (double)Rf[3 * r + 1] * X1) + ((double)Rf[3 * r + 2] * X2 + (double)tf[r]);
    }
    const double e1x = P[1][0] - P[0][0], e1y = P[1][1] - P[0][1], e1z = P[1][2] - P[0][2];
    const double e2x = P[2][0] - P[0][0], e2y = P[2][1] - P[0][1], e2z = P[2][2] - P[0][2];
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    bool empty = !(len > 0.0) || !isfinite(len);
    double d0 = 0.0;
    if (!empty) {
      nx /= len; ny /= len; nz /= len;
      d0 = nx * P[0][0] + ny * P[0][1] + nz * P[0][2];
    } else {
      nx = ny = 0.0; nz = 1.0;
    }
    const double zmin = fmin(P[0][2], fmin(P[1][2], P[2][2])), zmax = fmax(P[0][2], fmax(P[1][2], P[2][2]));
    if (!(zmax > 0.0)) empty = true;   // wholly behind the camera plane: no primary ray (t > 0) and no shadow ray (0 < z <= z_hit) meets it
    int x0, x1, y0, y1, q0, q1;
    if (empty) {
      x0 = q0 = y0 = 1; x1 = q1 = y1 = 0;
    } else if (zmin < RND_NEAR) {
      x0 = q0 = RND_BOX_MIN; x1 = q1 = RND_BOX_MAX; y0 = 0; y1 = h - 1;
    } else {
      double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300, pmin = 1e300, pmax = -1e300;
      for (int v = 0; v < 3; ++v) {
        const double iz = 1.0 / P[v][2];
        const double u = (double)cam.cx + (double)cam.fx * P[v][0] * iz, vv = (double)cam.cy + (double)cam.fy * P[v][1] * iz;
        const double pu = (double)cam.cx + (double)cam.fx * (P[v][0] - (double)cam.baseline) * iz;
        umin = fmin(umin, u); umax = fmax(umax, u); vmin = fmin(vmin, vv); vmax = fmax(vmax, vv);
        pmin = fmin(pmin, pu); pmax = fmax(pmax, pu);
      }
      x0 = rnd_box_lo(umin); x1 = rnd_box_hi(umax); q0 = rnd_box_lo(pmin); q1 = rnd_box_hi(pmax);
      y0 = rnd_box_lo(vmin); y1 = rnd_box_hi(vmax);
      if (y0 < 0) y0 = 0;
      if (y1 > h - 1) y1 = h - 1;
      if (y0 > y1) { y0 = 1; y1 = 0; }
    }
    tri[4 * e + 0] = make_float4((float)P[0][0], (float)P[0][1], (float)P[0][2], (float)nx);
    tri[4 * e + 1] = make_float4((float)P[1][0], (float)P[1][1], (float)P[1][2], (float)ny);
    tri[4 * e + 2] = make_float4((float)P[2][0], (float)P[2][1], (float)P[2][2], (float)nz);
    tri[4 * e + 3] = make_float4((float)d0, albedo[k], 0.f, 0.f);
    box[e] = make_int4(rnd_pack(x0, x1), rnd_pack(y0, y1), rnd_pack(q0, q1), 0);
  }
}

// Does the ray from the origin through (dx, dy, 1) meet the triangle (vertices moved by -xoff in x)?  z: its depth along that ray.
__device__ __forceinline__ bool rnd_hit(const float4 r0, const float4 r1, const float4 r2, const float d0, const float xoff,
                                        const float dx, const float dy, float& z) {
#pragma clang fp contract(off)
  const float ax = (r0.x - xoff) - dx * r0.z, ay = r0.y - dy * r0.z;
  const float bx = (r1.x - xoff) - dx * r1.z, by = r1.y - dy * r1.z;
  const float cx = (r2.x - xoff) - dx * r2.z, cy = r2.y - dy * r2.z;
  const float U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
  const bool pos = U >= 0.f && V >= 0.f && W >= 0.f, neg = U <= 0.f && V <= 0.f && W <= 0.f;
  if (!(pos || neg) || (pos && neg)) return false;   // (all three zero: seen edge-on)
  const float den = r0.w * dx + r1.w * dy + r2.w;
  if (den == 0.f) return false;
  z = d0 / den;
  return true;
}

struct RndPixel {
  float dx, dy;        // primary ray (dx, dy, 1)
  float z;             // best depth so far (INFINITY: none)
  int id;              // its triangle (-1: none)
  float nx, ny, nz, g; // its plane normal and albedo
  float qx, pz;        // shadow pass: direction x of the projector's ray through the hit point, depth of the hit point
  bool active, lit;
};

// Walk the frame's boxes; SHADOW = false: primary rays of the tile, true: shadow rays of its hit pixels.
template <bool SHADOW>
__device__ __forceinline__ void rnd_walk(const float4* __restrict__ trif, const int4* __restrict__ boxf, const int nf, const int tx0,
                                         const int ty0, const int lo, const int hi, const float baseline, RndPixel& p, int* s_cand,
                                         int (*s_wcnt)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int count = 0, it = 0;
  for (int base = 0; base < nf; base += RND_BLOCK, ++it) {
    const int k = base + tid;
    bool keep = false;
    if (k < nf) {
      const int4 b = boxf[k];
      const bool rows = rnd_lo(b.y) <= ty0 + RND_TILE - 1 && rnd_hi(b.y) >= ty0;
      if (SHADOW) keep = rows && rnd_lo(b.z) <= hi && rnd_hi(b.z) >= lo;
      else keep = rows && rnd_lo(b.x) <= tx0 + RND_TILE - 1 && rnd_hi(b.x) >= tx0;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wcnt[it & 1][wv] = __popcll(m);
    __syncthreads();
    int off = count, tot = 0;
#pragma unroll
    for (int i = 0; i < RND_BLOCK / 64; ++i) {
      const int c = s_wcnt[it & 1][i];
      if (i < wv) off += c;
      tot += c;
    }
    if (keep) s_cand[off + __popcll(m & ((1ull << lane) - 1ull))] = k;
    count += tot;
    if (count > RND_CAP - RND_BLOCK || base + RND_BLOCK >= nf) {
      __syncthreads();
      for (int c = 0; c < count; ++c) {
        const int id = __builtin_amdgcn_readfirstlane(s_cand[c]);
        const float4 r0 = trif[4L * id], r1 = trif[4L * id + 1], r2 = trif[4L * id + 2], r3 = trif[4L * id + 3];
        float z;
        if (!SHADOW) {
          if (p.active && rnd_hit(r0, r1, r2, r3.x, 0.f, p.dx, p.dy, z) && z > 0.f && z < p.z) {
            p.z = z; p.id = id; p.nx = r0.w; p.ny = r1.w; p.nz = r2.w; p.g = r3.y;
          }
        } else {
          if (p.lit && id != p.id && rnd_hit(r0, r1, r2, r3.x - r0.w * baseline, baseline, p.qx, p.dy, z)) {
            const float s = z / p.pz;
            if (s > RND_SHADOW_EPS && s < 1.f - RND_SHADOW_EPS) p.lit = false;
          }
        }
      }
      __syncthreads();
      count = 0;
    }
  }
}

__global__ void __launch_bounds__(RND_BLOCK) render_cast_kernel(const float4* __restrict__ tri, const int4* __restrict__ box, const int nf,
                                                                const float* __restrict__ R, const float* __restrict__ t, const RndCam cam,
                                                                const float* __restrict__ pattern, const RndOutDev out, const int tl,
                                                                const int h, const int w) {
  __shared__ int s_cand[RND_CAP];
  __shared__ int s_wcnt[2][4];
  __shared__ int s_up[2];
  const int f = blockIdx.z, tid = threadIdx.x;
  const int tx0 = blockIdx.x * RND_TILE, ty0 = blockIdx.y * RND_TILE;
  const int px = tx0 + (tid & (RND_TILE - 1)), py = ty0 + tid / RND_TILE;
  const float4* trif = tri + 4L * f * nf;
  const int4* boxf = box + (long)f * nf;
  RndPixel p;
  p.active = px < w && py < h;
  p.dx = ((float)px - cam.cx) / cam.fx;
  p.dy = ((float)py - cam.cy) / cam.fy;
  p.z = INFINITY; p.id = -1; p.nx = p.ny = 0.f; p.nz = 1.f; p.g = 0.f; p.qx = 0.f; p.pz = 1.f; p.lit = false;
  if (tid == 0) { s_up[0] = RND_BOX_MAX + 1; s_up[1] = RND_BOX_MIN - 1; }
  rnd_walk<false>(trif, boxf, nf, tx0, ty0, 0, 0, cam.baseline, p, s_cand, s_wcnt);
  const bool hit = p.id >= 0;
  const float Px = p.dx * p.z, Py = p.dy * p.z, Pz = p.z;
  if (hit) {
    p.qx = (Px - cam.baseline) / Pz;
    p.pz = Pz;
    p.lit = true;
    const float up = fminf(fmaxf(cam.cx + cam.fx * p.qx, (float)RND_BOX_MIN), (float)RND_BOX_MAX);
    atomicMin(&s_up[0], (int)floorf(up));
    atomicMax(&s_up[1], (int)ceilf(up));
  }
  __syncthreads();
  const int lo = s_up[0], hi = s_up[1];
  if (lo <= hi) rnd_walk<true>(trif, boxf, nf, tx0, ty0, lo, hi, cam.baseline, p, s_cand, s_wcnt);
  if (!p.active) return;
  const long hw = (long)h * w, o = (long)py * w + px;
  float im = 0.f, amb = 0.f, disp = 0.f;
  if (hit) {
    disp = cam.baseline * cam.fx / Pz;
    float nx = p.nx, ny = p.ny, nz = p.nz;
    float cdot = -(nx * Px + ny * Py + nz * Pz) / sqrtf(Px * Px + Py * Py + Pz * Pz);
    if (cdot < 0.f) { nx = -nx; ny = -ny; nz = -nz; cdot = -cdot; }   // face normal towards the viewer
    const float qx = cam.baseline - Px, qy = -Py, qz = -Pz;
    const float pdot = (nx * qx + ny * qy + nz * qz) / sqrtf(qx * qx + qy * qy + qz * qz);
    amb = fminf(fmaxf(p.g * (RND_KA + RND_KD * fmaxf(0.f, cdot)) * 0.5f, 0.f), 1.f);
    float sx = fminf(fmaxf((float)px - disp, 0.f), (float)(w - 1));
    const int sx0 = (int)floorf(sx), sx1 = sx0 + 1 < w ? sx0 + 1 : w - 1;
    const float wx = sx - (float)sx0;
    const float pat = pattern[(long)py * w + sx0] * (1.f - wx) + pattern[(long)py * w + sx1] * wx;
    const float pr = fminf(fmaxf(p.g * (RND_KA + RND_KD * fmaxf(0.f, pdot)) * 0.5f, 0.f), 1.f) * pat * (p.lit ? 1.f : 0.f);
    im = fminf(fmaxf(cam.blend * pr + (1.f - cam.blend) * amb, 0.f), 1.f);
  }
  out.im[f * hw + o] = im;
  out.ambient[f * hw + o] = amb;
  out.disp[f * hw + o] = disp;
  if (out.tri_id) out.tri_id[f * hw + o] = p.id;
  if (out.lit) out.lit[f * hw + o] = hit && p.lit ? 1.f : 0.f;
  // flow_fj = pi_j(X_w) - (u, v):  X_w = R_f^T (X_c - t_f)
  const float* Rf = R + f * 9;
  const float cxv = Px - t[f * 3], cyv = Py - t[f * 3 + 1], czv = Pz - t[f * 3 + 2];
  const float Xw = Rf[0] * cxv + Rf[3] * cyv + Rf[6] * czv;
  const float Yw = Rf[1] * cxv + Rf[4] * cyv + Rf[7] * czv;
  const float Zw = Rf[2] * cxv + Rf[5] * cyv + Rf[8] * czv;
  for (int j = 0; j < tl; ++j) {
    float fu = 0.f, fv = 0.f;
    if (hit && j != f) {
      const float* Rj = R + j * 9;
      const float xj = Rj[0] * Xw + Rj[1] * Yw + Rj[2] * Zw + t[j * 3];
      const float yj = Rj[3] * Xw + Rj[4] * Yw + Rj[5] * Zw + t[j * 3 + 1];
      const float zj = Rj[6] * Xw + Rj[7] * Yw + Rj[8] * Zw + t[j * 3 + 2];
      fu = (cam.fx * xj / zj + cam.cx) - (float)px;
      fv = (cam.fy * yj / zj + cam.cy) - (float)py;
    }
    const long q = ((long)(f * tl + j) * 2) * hw + o;
    out.flow[q] = fu;
    out.flow[q + hw] = fv;
  }
}

static inline bool rnd_extents_ok(int nv, int nf, int tl, int h, int w) {
  return nv > 0 && nf > 0 && tl > 0 && tl <= TRACK_MAX_TL && nf <= RND_MAX_NF && nv <= RND_MAX_NV && track_image_ok(h, w, 1);
}

extern "C" long dis_render_workspace(int nv, int nf, int tl, int h, int w) {
  if (!rnd_extents_ok(nv, nf, tl, h, w)) return -1;
  return (long)tl * (long)nf * (long)(4 * sizeof(float4) + sizeof(int4));
}

extern "C" int dis_render_track(const float* verts, const int* faces, const float* albedo, int nv, int nf, const float* R, const float* t,
                                const float* K4_host, float baseline, float blend, const float* pattern, const DisRenderOut* out, int tl,
                                int h, int w, void* workspace, void* stream) {
  if (!verts || !faces || !albedo || !R || !t || !K4_host || !pattern || !out || !workspace) return DIS_ERR_NULL;
  if (!out->im || !out->ambient || !out->disp || !out->flow) return DIS_ERR_NULL;
  if (!rnd_extents_ok(nv, nf, tl, h, w)) return DIS_ERR_BAD_SHAPE;
  RndCam cam;
  cam.fx = K4_host[0]; cam.fy = K4_host[1]; cam.cx = K4_host[2]; cam.cy = K4_host[3];
  cam.baseline = baseline; cam.blend = blend;
  if (!track_pos_finite(cam.fx) || !track_pos_finite(cam.fy) || !track_finite(cam.cx) || !track_finite(cam.cy)) return DIS_ERR_UNSUPPORTED;
  if (!track_pos_finite(baseline) || !(blend >= 0.f && blend <= 1.f)) return DIS_ERR_UNSUPPORTED;
  if (((uintptr_t)workspace & 15) != 0) return DIS_ERR_UNSUPPORTED;
  float4* tri = (float4*)workspace;
  int4* box = (int4*)(tri + 4L * tl * nf);
  RndOutDev o;
  o.im = out->im; o.ambient = out->ambient; o.disp = out->disp; o.flow = out->flow; o.lit = out->lit; o.tri_id = out->tri_id;
  hipLaunchKernelGGL(render_setup_kernel, dim3(dis_ew_grid((long)tl * nf, RND_BLOCK)), dim3(RND_BLOCK), 0, (hipStream_t)stream, verts,
                     faces, albedo, nv, nf, R, t, cam, tl, h, w, tri, box);
  DIS_CHECK_LAUNCH();
  const dim3 grid(dis_cdiv(w, RND_TILE), dis_cdiv(h, RND_TILE), tl);
  hipLaunchKernelGGL(render_cast_kernel, grid, dim3(RND_BLOCK), 0, (hipStream_t)stream, (const float4*)tri, (const int4*)box, nf, R, t,
                     cam, pattern, o, tl, h, w);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}
