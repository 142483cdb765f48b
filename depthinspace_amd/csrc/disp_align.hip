// Flow-free pairwise poses and the flow they imply (include/dis_hip.h, section "disparity alignment").
//
// dis_disp_align_poses: the relative camera pose of every ordered frame pair of a track from its disparity maps alone - direct
// coarse-to-fine alignment of frame i's disparity map onto frame j's, Gauss-Newton on the residual in disparity, from the identity.  No
// flow is read.  Every per-pixel term is a fixed fp32 expression in the operand order of tests/disp_align_ref.py, converted to fp64 and
// added in fp64; the state and the solve are fp64.  The 30 sums, the block record, the record sum, the twist update and the 6 x 6 step are
// those of pose.hip and tsdf_align.hip (track_common.h).  Order and hand-off between launches are held by the launch boundaries alone -
// no atomics, no flags polled between workgroups - so two calls give the same bits.
//
//   dalign_down_kernel   a lane per cell of level l + 1: the mean of the near disparities of its 2 x 2 block.  One launch per level
//                        above 0, every frame of every track in the grid.
//   dalign_maps_kernel   a lane per pixel of a level: {D, Dx, Dy, good} packed into one float4, so that a bilinear tap of the accumulate
//                        kernel is one 16-byte load and the four taps of a pixel are two 32-byte runs.  One launch per level.
//   dalign_accum_kernel  the hot path.  bpp workgroups of 256 lanes per pair.  A wave owns an 8 x 8 patch of frame i and a workgroup
//                        2 x 2 of them, as in tsdf_align_accum_kernel: under a small motion the patch lands on a patch of frame j about
//                        as large, so the 4 x 64 taps of a wave fall into some 9 x 9 float4 = 18 lines of 128 bytes instead of the up to
//                        256 a row-major range of 64 pixels could touch at a rotation about the optical axis.  The workgroups of a pair
//                        take its 16 x 16 tiles in turn (tile blk, blk + bpp, ...).  30 sums in fp64 registers; then the reduction of the
//                        pose kernels, one record of 32 doubles per workgroup.
//   dalign_solve_kernel  one wave per pair: lanes 0 .. 29 add the pair's records in ascending workgroup order, lane 0 factors the 6 x 6
//                        system and updates the state - or, in the closing launch, writes R_pair, t_pair and stats, the diagonal included.
// The first accumulate launch takes the identity instead of reading the state and the first solve launch starts from it, so the
// workspace needs no initialisation.
//
// dis_rigid_flow: one launch, a lane per pixel of an ordered pair: the flow of frame i's disparities under the frame poses.
#include "track_common.h"

#define DALIGN_MAX_LEVELS 6
#define DALIGN_MIN_SIDE 8
#define DALIGN_NUDGE 0.015625f   // 2^-6
#define DALIGN_TILE 16       // pixels of a workgroup per side: 2 x 2 waves of 8 x 8

__global__ __launch_bounds__(TRACK_BLOCK) void dalign_down_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                  float* __restrict__ dbg, const int frames, const int hs, const int ws,
                                                                  const int hd, const int wd) {
  const long cell = (long)blockIdx.x * TRACK_BLOCK + threadIdx.x;
  if (cell >= (long)frames * hd * wd) return;
  const int x = (int)(cell % wd), y = (int)((cell / wd) % hd);
  const long f = cell / ((long)wd * hd);
  const float* s = src + (f * hs + 2 * y) * ws + 2 * x;    // 2 y + 1 <= hs - 1, 2 x + 1 <= ws - 1
  const float a[4] = {s[0], s[1], s[ws], s[ws + 1]};
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (track_valid(a[k]) && a[k] > m) m = a[k];
  const float thr = 0.9f * m;
  float sum = 0.f, cnt = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (track_valid(a[k]) && a[k] >= thr) sum = sum + a[k], cnt = cnt + 1.f;
  const float out = cnt > 0.f ? sum / cnt : 0.f;
  dst[cell] = out;
  if (dbg) dbg[cell] = out;
}

__global__ __launch_bounds__(TRACK_BLOCK) void dalign_maps_kernel(const float* __restrict__ src, float4* __restrict__ maps,
                                                                  float4* __restrict__ dbg, const int frames, const int h, const int w,
                                                                  const float jump) {
  const long pix = (long)blockIdx.x * TRACK_BLOCK + threadIdx.x;
  if (pix >= (long)frames * h * w) return;
  const int x = (int)(pix % w), y = (int)((pix / w) % h);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
    const float* s = src + pix;
    const float c = s[0], l = s[-1], r = s[1], up = s[-w], dn = s[w];
    const float dx = 0.5f * (r - l), dy = 0.5f * (dn - up);
    const float lim = jump * c;
    // (every comparison is false for NaN)
    if (track_valid(c) && track_valid(l) && track_valid(r) && track_valid(up) && track_valid(dn) && fabsf(dx) < lim && fabsf(dy) < lim)
      o = make_float4(c, dx, dy, 1.f);
  }
  maps[pix] = o;
  if (dbg) dbg[pix] = o;
}

struct DalignParams {
  int tl, h, w, hw, bpp, tiles_x, tiles;   // of the level
  long frame_stride;                       // h w
  TrackCamera cam;                         // the level's intrinsics; fb is that of level 0 (disparities stay in full-resolution pixels)
  float s2, jump2;                         // scale * scale, 2 * jump
};

// One pixel (u, v) of frame i with the disparity d at the state (R, t): its target in frame j's maps mj, the 30 terms at the state's fp32
// rounding, added to acc[] in fp64.  A pixel that is skipped adds nothing.
__device__ __forceinline__ void dalign_pixel(double* acc, const float4* __restrict__ mj, const float d, const int u, const int v,
                                             const DalignParams& p, const float* R, const float* t, const int unit) {
  if (!track_valid(d)) return;
  float P[3], Y[3];
  track_backproject(d, u, v, p.cam, P);
  track_to_camera(R, t, P, Y);
  if (!(Y[2] > 0.f)) return;
  const float iz = 1.f / Y[2];
  const float px = Y[0] * iz, py = Y[1] * iz;
  const float up = p.cam.fx * px + p.cam.cx, vp = p.cam.fy * py + p.cam.cy;
  // The cell is that of (u' + 2^-6, v' + 2^-6): at the identity every target lies on an integer up to rounding, and with the boundary of
  // the cells there the cell - and with it the test of the four taps - would be decided by the last bit.  ax, ay >= -2^-6: the cell's
  // own interpolant, continued by that much.  0 <= x0 <= w - 2, 0 <= y0 <= h - 2 (every comparison is false for NaN)
  const float us = up + DALIGN_NUDGE, vs = vp + DALIGN_NUDGE;
  if (!(us >= 0.f && us < (float)(p.w - 1) && vs >= 0.f && vs < (float)(p.h - 1))) return;
  const int x0 = (int)floorf(us), y0 = (int)floorf(vs);
  const float4* c = mj + y0 * p.w + x0;
  const float4 m00 = c[0], m01 = c[1], m10 = c[p.w], m11 = c[p.w + 1];
  if (!(m00.w != 0.f && m01.w != 0.f && m10.w != 0.f && m11.w != 0.f)) return;
  const float ax = up - (float)x0, ay = vp - (float)y0;
  const float bx = 1.f - ax, by = 1.f - ay;
  const float D = (m00.x * bx + m01.x * ax) * by + (m10.x * bx + m11.x * ax) * ay;
  const float Gx = (m00.y * bx + m01.y * ax) * by + (m10.y * bx + m11.y * ax) * ay;
  const float Gy = (m00.z * bx + m01.z * ax) * by + (m10.z * bx + m11.z * ax) * ay;
  const float pred = p.cam.fb * iz;
  const float e = D - pred;
  if (!(fabsf(e) < p.jump2 * pred)) return;
  const float g0 = Gx * (p.cam.fx * iz), g1 = Gy * (p.cam.fy * iz);
  const float g2 = pred * iz - (g0 * Y[0] + g1 * Y[1]) * iz;
  const float J[6] = {Y[1] * g2 - Y[2] * g1, Y[2] * g0 - Y[0] * g2, Y[0] * g1 - Y[1] * g0, g0, g1, g2};
  const int I[6] = {0, 1, 2, 3, 4, 5};
  const float e2 = e * e;
  const float q = 1.f / (1.f + e2 / p.s2);
  const float wgt = unit ? 1.f : q * q;
  pose_add_row(acc, wgt, J, I, e);
  acc[27] += (double)wgt;
  acc[28] += (double)(wgt * e2);
  acc[29] += 1.0;
}

__global__ __launch_bounds__(POSE_BLOCK) void dalign_accum_kernel(const float* __restrict__ lvl, const float4* __restrict__ maps,
                                                                  const double* __restrict__ state, double* __restrict__ partial,
                                                                  const DalignParams p, const int first, const int unit) {
  const int pair = blockIdx.x / p.bpp;             // (b tl + i) tl + j: uniform over the workgroup
  const int blk = blockIdx.x % p.bpp;
  const int tt = p.tl * p.tl;
  const int b = pair / tt, i = (pair % tt) / p.tl, j = pair % p.tl;
  if (i == j) return;                              // (the whole workgroup: no barrier is passed by a part of it)
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
  if (!first) {
    const double* s = state + (size_t)pair * POSE_STATE;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (float)s[9 + k];
  }
  const float* di = lvl + (long)(b * p.tl + i) * p.frame_stride;
  const float4* mj = maps + (long)(b * p.tl + j) * p.frame_stride;
  const int wave = threadIdx.x / DIS_WAVE, lane = threadIdx.x & (DIS_WAVE - 1);
  const int du = (wave & 1) * 8 + (lane & 7), dv = (wave >> 1) * 8 + (lane >> 3);
  double acc[POSE_SUMS];
#pragma unroll
  for (int k = 0; k < POSE_SUMS; ++k) acc[k] = 0.0;
  for (int tile = blk; tile < p.tiles; tile += p.bpp) {
    const int u = (tile % p.tiles_x) * DALIGN_TILE + du, v = (tile / p.tiles_x) * DALIGN_TILE + dv;
    if (u < p.w && v < p.h) dalign_pixel(acc, mj, di[v * p.w + u], u, v, p, R, t, unit);
  }
  pose_block_record<POSE_SUMS>(acc, partial + ((size_t)pair * p.bpp + blk) * POSE_REC);
}

struct DalignSolveParams {
  int tl, bpp, min_corr;
  double damping;
};

__global__ __launch_bounds__(DIS_WAVE) void dalign_solve_kernel(const double* __restrict__ partial, double* __restrict__ state,
                                                                float* __restrict__ R_pair, float* __restrict__ t_pair,
                                                                float* __restrict__ stats, double* __restrict__ dbg_sums,
                                                                const DalignSolveParams p, const int first, const int last) {
  __shared__ double S[POSE_REC];
  const int pair = blockIdx.x;
  const int i = (pair % (p.tl * p.tl)) / p.tl, j = pair % p.tl;
  if (i == j) {
    if (dbg_sums && threadIdx.x < POSE_SUMS) dbg_sums[(size_t)pair * POSE_SUMS + threadIdx.x] = 0.0;
    if (last && threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R_pair[(size_t)pair * 9 + k] = (k % 4 == 0) ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) t_pair[(size_t)pair * 3 + k] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) stats[(size_t)pair * 4 + k] = (k == 3) ? 1.f : 0.f;
    }
    return;
  }
  if (threadIdx.x < POSE_SUMS) {
    const double s = pose_sum_records(partial + (size_t)pair * p.bpp * POSE_REC + threadIdx.x, p.bpp);
    S[threadIdx.x] = s;
    if (dbg_sums) dbg_sums[(size_t)pair * POSE_SUMS + threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* st = state + (size_t)pair * POSE_STATE;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  bool failed = false;
  if (!first) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = st[9 + k];
    failed = st[12] != 0.0;
  }
  if (last) {
    const double nc = S[29], sw = S[27], sc = S[28];
#pragma unroll
    for (int k = 0; k < 9; ++k) R_pair[(size_t)pair * 9 + k] = (float)R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t_pair[(size_t)pair * 3 + k] = (float)t[k];
    stats[(size_t)pair * 4 + 0] = (float)nc;
    stats[(size_t)pair * 4 + 1] = nc > 0.0 ? (float)(sw / nc) : 0.f;
    stats[(size_t)pair * 4 + 2] = (nc > 0.0 && sw > 0.0) ? (float)sqrt(sc / sw) : 0.f;
    stats[(size_t)pair * 4 + 3] = failed ? 0.f : 1.f;
    return;
  }
  if (!failed) failed = !pose_gn_step(S, p.min_corr, p.damping, R, t);
#pragma unroll
  for (int k = 0; k < 9; ++k) st[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = failed ? 1.0 : 0.0;
}

struct DalignPlan {
  long pairs, frames;                    // n tl tl (the diagonal included), n tl
  int lh[DALIGN_MAX_LEVELS], lw[DALIGN_MAX_LEVELS], bpp[DALIGN_MAX_LEVELS], tiles_x[DALIGN_MAX_LEVELS], tiles[DALIGN_MAX_LEVELS];
  long off_state, off_partial, off_pyr[DALIGN_MAX_LEVELS], off_maps[DALIGN_MAX_LEVELS], bytes;
};

// the extents of dis_track_poses
static bool dalign_shape_ok(int n, int tl, int h, int w) {
  if (n < 1 || tl < 2 || tl > TRACK_MAX_TL || !track_image_ok(h, w, 2)) return false;
  return (long)n * tl * tl * 2 * h * w <= 0x7fffffffL;
}

// false: levels outside 1 .. 6 or a level below 8 x 8 (the extents are the caller's to check first)
static bool dalign_plan(int n, int tl, int h, int w, int levels, DalignPlan* pl) {
  if (levels < 1 || levels > DALIGN_MAX_LEVELS) return false;
  if ((h >> (levels - 1)) < DALIGN_MIN_SIDE || (w >> (levels - 1)) < DALIGN_MIN_SIDE) return false;
  pl->pairs = (long)n * tl * tl, pl->frames = (long)n * tl;
  TrackCarver ws = {16, 0};
  pl->off_state = ws.take(pl->pairs * POSE_STATE * 8);
  for (int l = 0; l < levels; ++l) {
    const int lh = pl->lh[l] = h >> l, lw = pl->lw[l] = w >> l;
    pl->tiles_x[l] = dis_cdiv(lw, DALIGN_TILE);
    pl->tiles[l] = pl->tiles_x[l] * dis_cdiv(lh, DALIGN_TILE);
    const int bpp = pose_bpp(lh, lw);
    pl->bpp[l] = bpp < pl->tiles[l] ? bpp : pl->tiles[l];
    pl->off_pyr[l] = l == 0 ? 0 : ws.take(pl->frames * lh * lw * 4);    // level 0 is the input
    pl->off_maps[l] = ws.take(pl->frames * lh * lw * 16);
  }
  pl->off_partial = ws.take(pl->pairs * pl->bpp[0] * POSE_REC * 8);      // bpp[0] is the largest
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_disp_align_workspace(int n, int tl, int h, int w, int levels) {
  DalignPlan pl;
  if (!dalign_shape_ok(n, tl, h, w) || !dalign_plan(n, tl, h, w, levels, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_disp_align_poses(const float* disp, const float* K4_host, float baseline, int levels, const int* iters_host, float scale,
                                    float damping, int min_corr, float jump, float* R_pair, float* t_pair, float* stats,
                                    const DisDispAlignDebug* dbg, int n, int tl, int h, int w, void* workspace, long workspace_bytes,
                                    void* stream) {
  if (!disp || !K4_host || !iters_host || !R_pair || !t_pair || !stats || !workspace) return DIS_ERR_NULL;
  if (!dalign_shape_ok(n, tl, h, w)) return DIS_ERR_BAD_SHAPE;
  DalignPlan pl;
  if (!dalign_plan(n, tl, h, w, levels, &pl)) return DIS_ERR_UNSUPPORTED;
  int passes = 1;                                  // the closing one
  for (int l = 0; l < levels; ++l) {
    if (iters_host[l] < 0 || iters_host[l] > 64) return DIS_ERR_UNSUPPORTED;
    passes += iters_host[l];
  }
  DalignParams p;
  p.s2 = scale * scale;
  p.jump2 = 2.f * jump;
  if (passes < 2 || !track_pos_finite(scale) || !(damping >= 0.f && track_finite(damping)) || min_corr < 6 || !(jump > 0.f && jump < 1.f) ||
      !track_camera(K4_host, baseline, &p.cam) || !track_pos_finite(p.s2) || workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15) ||
      (dbg && dbg->maps && (dbg->level < 0 || dbg->level >= levels)))
    return DIS_ERR_UNSUPPORTED;
  TrackCamera cams[DALIGN_MAX_LEVELS];
  cams[0] = p.cam;
  for (int l = 1; l < levels; ++l) {
    cams[l] = cams[l - 1];
    cams[l].fx = cams[l - 1].fx / 2.f, cams[l].fy = cams[l - 1].fy / 2.f;
    cams[l].cx = (cams[l - 1].cx - 0.5f) / 2.f, cams[l].cy = (cams[l - 1].cy - 0.5f) / 2.f;
    if (!track_pos_finite(cams[l].fx) || !track_pos_finite(cams[l].fy)) return DIS_ERR_UNSUPPORTED;   // (an fx that underflows)
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* state = (double*)(ws + pl.off_state);
  double* partial = (double*)(ws + pl.off_partial);
  const float* lvl[DALIGN_MAX_LEVELS];
  lvl[0] = disp;
  float* dbg_pyr = dbg ? dbg->pyr : nullptr;
  const int frames = (int)pl.frames;
  for (int l = 0; l < levels; ++l) {
    const long cells = pl.frames * pl.lh[l] * pl.lw[l];    // <= n tl h w < 2^30
    const unsigned grid = (unsigned)dis_cdiv(cells, TRACK_BLOCK);
    if (l > 0) {
      float* dst = (float*)(ws + pl.off_pyr[l]);
      hipLaunchKernelGGL(dalign_down_kernel, dim3(grid), dim3(TRACK_BLOCK), 0, st, lvl[l - 1], dst, dbg_pyr, frames, pl.lh[l - 1],
                         pl.lw[l - 1], pl.lh[l], pl.lw[l]);
      DIS_CHECK_LAUNCH();
      lvl[l] = dst;
      if (dbg_pyr) dbg_pyr += cells;
    }
    hipLaunchKernelGGL(dalign_maps_kernel, dim3(grid), dim3(TRACK_BLOCK), 0, st, lvl[l], (float4*)(ws + pl.off_maps[l]),
                       (dbg && dbg->maps && dbg->level == l) ? (float4*)dbg->maps : (float4*)nullptr, frames, pl.lh[l], pl.lw[l], jump);
    DIS_CHECK_LAUNCH();
  }
  DalignSolveParams sp;
  sp.tl = tl, sp.min_corr = min_corr, sp.damping = (double)damping;
  double* dbg_sums = dbg ? dbg->sums : nullptr;
  p.tl = tl;
  int pass = 0;
  for (int l = levels - 1; l >= -1; --l) {         // -1: the closing pass, at level 0
    const int lv = l < 0 ? 0 : l, steps = l < 0 ? 1 : iters_host[l];
    p.h = pl.lh[lv], p.w = pl.lw[lv], p.hw = p.h * p.w, p.frame_stride = (long)p.h * p.w;
    p.bpp = sp.bpp = pl.bpp[lv], p.tiles_x = pl.tiles_x[lv], p.tiles = pl.tiles[lv];
    p.cam = cams[lv];
    const unsigned grid = (unsigned)(pl.pairs * p.bpp);    // <= 2^31 / (2 * 4): as in dis_track_poses
    for (int s = 0; s < steps; ++s, ++pass) {
      hipLaunchKernelGGL(dalign_accum_kernel, dim3(grid), dim3(POSE_BLOCK), 0, st, lvl[lv], (const float4*)(ws + pl.off_maps[lv]),
                         (const double*)state, partial, p, pass == 0 ? 1 : 0, (l == levels - 1 && s == 0) ? 1 : 0);
      DIS_CHECK_LAUNCH();
      hipLaunchKernelGGL(dalign_solve_kernel, dim3((unsigned)pl.pairs), dim3(DIS_WAVE), 0, st, (const double*)partial, state, R_pair, t_pair,
                         stats, dbg_sums ? dbg_sums + (size_t)pass * pl.pairs * POSE_SUMS : (double*)nullptr, sp, pass == 0 ? 1 : 0,
                         l < 0 ? 1 : 0);
      DIS_CHECK_LAUNCH();
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ rigid flow
struct RigidParams {
  int tl, h, w, hw, bpi;                 // bpi = workgroups per image
  TrackCamera cam;
  float tol;
};

__global__ __launch_bounds__(TRACK_BLOCK) void rigid_flow_kernel(const float* __restrict__ disp, const float* __restrict__ R,
                                                                 const float* __restrict__ t, float* __restrict__ flow,
                                                                 unsigned char* __restrict__ visible, const RigidParams p) {
  const int pair = blockIdx.x / p.bpi;             // (b tl + i) tl + j: uniform over the workgroup
  const int pix = (blockIdx.x % p.bpi) * TRACK_BLOCK + (int)threadIdx.x;
  if (pix >= p.hw) return;
  const int tt = p.tl * p.tl;
  const int b = pair / tt, i = (pair % tt) / p.tl, j = pair % p.tl;
  float* fo = flow + (size_t)pair * 2 * p.hw + pix;          // n tl tl 2 h w < 2^31: checked on the host
  float f0 = 0.f, f1 = 0.f;
  unsigned char vis = 0;
  const int v = pix / p.w, u = pix % p.w;
  const float d = disp[(b * p.tl + i) * p.hw + pix];
  if (i != j && track_valid(d)) {
    float P[3], X[3], Y[3];
    track_backproject(d, u, v, p.cam, P);
    track_to_world(R + (b * p.tl + i) * 9, t + (b * p.tl + i) * 3, P, X);
    track_to_camera(R + (b * p.tl + j) * 9, t + (b * p.tl + j) * 3, X, Y);
    if (Y[2] > 0.f) {
      const float uj = (p.cam.fx * Y[0]) / Y[2] + p.cam.cx, vj = (p.cam.fy * Y[1]) / Y[2] + p.cam.cy;
      f0 = uj - (float)u, f1 = vj - (float)v;
      const float ur = uj + 0.5f, vr = vj + 0.5f;
      if (ur >= 0.f && ur < (float)p.w && vr >= 0.f && vr < (float)p.h) {    // (false for NaN)
        const float dj = disp[(b * p.tl + j) * p.hw + (int)floorf(vr) * p.w + (int)floorf(ur)];
        const float pred = p.cam.fb / Y[2];
        vis = (track_valid(dj) && fabsf(dj - pred) <= p.tol * pred) ? 1 : 0;
      }
    }
  }
  fo[0] = f0, fo[p.hw] = f1;
  if (visible) visible[(size_t)pair * p.hw + pix] = vis;
}

extern "C" int dis_rigid_flow(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, float tol,
                              float* flow, unsigned char* visible, int n, int tl, int h, int w, void* stream) {
  if (!disp || !R || !t || !K4_host || !flow) return DIS_ERR_NULL;
  if (!dalign_shape_ok(n, tl, h, w)) return DIS_ERR_BAD_SHAPE;
  RigidParams p;
  if (!(tol > 0.f && tol < 1.f) || !track_camera(K4_host, baseline, &p.cam)) return DIS_ERR_UNSUPPORTED;
  p.tl = tl, p.h = h, p.w = w, p.hw = h * w, p.bpi = dis_cdiv((long)h * w, TRACK_BLOCK), p.tol = tol;
  const unsigned grid = (unsigned)((long)n * tl * tl * p.bpi);   // <= 2^31 / (2 * 4) / 256 + n tl tl
  hipLaunchKernelGGL(rigid_flow_kernel, dim3(grid), dim3(TRACK_BLOCK), 0, (hipStream_t)stream, disp, R, t, flow, visible, p);
  DIS_CHECK_LAUNCH();
  return 0;
}
