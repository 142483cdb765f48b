// The relative camera pose of every ordered frame pair of a track from its disparities and flows (include/dis_hip.h, section "track
// poses"): Gauss-Newton on the residual in (u, v, disparity) of frame j.  Every per-pixel term is a fixed fp32 expression in the
// operand order of tests/pose_ref.py, converted to fp64 and added in fp64; the state and the solve are fp64.  Two kernels, launched in
// turn iters + 1 times; order and hand-off between them are held by the launch boundaries alone - no atomics, no flags polled between
// workgroups - so nothing depends on where workgroups are placed and two calls give the same bits.
//
//   pose_accum_kernel  bpp workgroups of 256 lanes per pair (the diagonal pairs leave at once), each lane a grid-stride range of the
//                      frame's pixels.  A lane recomputes its pixel's target in frame j (its disparity, its flow, four gathered
//                      disparities of frame j), forms the 30 terms at the state's fp32 rounding and adds them to 30 fp64 registers;
//                      then a DPP sum over the wave, the four waves through LDS, and one record of 32 doubles per workgroup.
//   pose_solve_kernel  one wave per pair: lanes 0 .. 29 add the pair's records in ascending workgroup order (32 loads in flight: with
//                      one load per addition the launch took as long as the accumulation, profiles/pose_rate.md), lane 0 factors the
//                      6 x 6 system, updates the state - or, in the closing launch, writes R_pair, t_pair and stats, the diagonal included.
// The first accumulate launch takes the identity instead of reading the state and the first solve launch starts from it, so the
// workspace needs no initialisation.
#include "track_common.h"

#define POSE_BLOCK 256
#define POSE_WAVES (POSE_BLOCK / DIS_WAVE)
#define POSE_SUMS 30     // H_pq (p <= q, row by row) 0 .. 20, g_p 21 .. 26, S_w 27, S_c 28, n 29
#define POSE_REC 32      // doubles per record of partial sums
#define POSE_STATE 16    // doubles per pair: R (9, row-major), t (3), failed (1), 3 unused
#define POSE_MAX_BPP 128
#define POSE_BATCH 32    // records in flight per lane of the solve launch

struct PoseParams {
  int n, tl, h, w, hw, bpp;              // bpp = workgroups per pair
  TrackCamera cam;
  float s2;                              // scale * scale
};

__device__ __forceinline__ constexpr int pose_hidx(int p, int q) { return p * 6 - p * (p - 1) / 2 + (q - p); }

// the terms of one residual row: J[] at the indices idx[0 .. m) (the other entries are structurally zero and are skipped)
template <int M>
__device__ __forceinline__ void pose_add_row(double* acc, const float wgt, const float* J, const int (&idx)[M], const float e) {
#pragma unroll
  for (int a = 0; a < M; ++a) {
    const float wJ = wgt * J[a];
#pragma unroll
    for (int b = a; b < M; ++b) acc[pose_hidx(idx[a], idx[b])] += (double)(wJ * J[b]);
    acc[21 + idx[a]] += (double)(wJ * e);
  }
}

__global__ __launch_bounds__(POSE_BLOCK) void pose_accum_kernel(const float* __restrict__ disp, const float* __restrict__ flow,
                                                                const double* __restrict__ state, double* __restrict__ partial,
                                                                const PoseParams p, const int first) {
  __shared__ double wave_part[POSE_WAVES][POSE_REC];
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
  const float* di = disp + (b * p.tl + i) * p.hw;          // n tl tl 2 h w < 2^31: checked on the host
  const float* dj = disp + (b * p.tl + j) * p.hw;
  const float* fl = flow + pair * 2 * p.hw;
  double acc[POSE_SUMS];
#pragma unroll
  for (int k = 0; k < POSE_SUMS; ++k) acc[k] = 0.0;
  for (int pix = blk * POSE_BLOCK + (int)threadIdx.x; pix < p.hw; pix += p.bpp * POSE_BLOCK) {
    const int v = pix / p.w, u = pix % p.w;
    const float d = di[pix];
    const float uj = (float)u + fl[pix], vj = (float)v + fl[p.hw + pix];
    // (every comparison is false for NaN)
    const bool in = track_valid(d) && uj >= 0.f && uj <= (float)(p.w - 1) && vj >= 0.f && vj <= (float)(p.h - 1);
    // 0 <= x0 <= w - 2, 0 <= y0 <= h - 2; a pixel without a target reads the cell at the origin and drops it
    const int x0 = in ? min((int)floorf(uj), p.w - 2) : 0;
    const int y0 = in ? min((int)floorf(vj), p.h - 2) : 0;
    const float* c = dj + y0 * p.w + x0;
    const float d00 = c[0], d01 = c[1], d10 = c[p.w], d11 = c[p.w + 1];
    if (!(in && track_valid(d00) && track_valid(d01) && track_valid(d10) && track_valid(d11))) continue;   // not matched: nothing is added
    const float ax = uj - (float)x0, ay = vj - (float)y0;
    const float gx = 1.f - ax, gy = 1.f - ay;
    const float ds = (d00 * gx + d01 * ax) * gy + (d10 * gx + d11 * ax) * ay;
    float P[3], X[3];
    track_backproject(d, u, v, p.cam, P);
    track_to_camera(R, t, P, X);
    const float X0 = X[0], X1 = X[1], X2 = X[2];
    if (!(X2 > 0.f)) continue;                     // not used
    // this projection is pose's own: fuse has (fx * X0) / X2 + cx, tsdf fx * (x / zs) + cx, rounded
    const float iz = 1.f / X2;
    const float px = X0 * iz, py = X1 * iz;
    const float e0 = (p.cam.fx * px + p.cam.cx) - uj, e1 = (p.cam.fy * py + p.cam.cy) - vj, e2 = p.cam.fb * iz - ds;
    const float r2 = (e0 * e0 + e1 * e1) + e2 * e2;
    const float g = 1.f / (1.f + r2 / p.s2);
    const float wgt = first ? 1.f : g * g;
    const float a = p.cam.fx * iz, bb = p.cam.fy * iz, cc = p.cam.fb * iz;
    const float g0 = -(a * px), g1 = -(bb * py), g2 = -(cc * iz);
    const float J0[5] = {g0 * X1, a * X2 - g0 * X0, -(a * X1), a, g0};
    const float J1[5] = {g1 * X1 - bb * X2, -(g1 * X0), bb * X0, bb, g1};
    const float J2[3] = {g2 * X1, -(g2 * X0), g2};
    const int I0[5] = {0, 1, 2, 3, 5}, I1[5] = {0, 1, 2, 4, 5}, I2[3] = {0, 1, 5};
    pose_add_row(acc, wgt, J0, I0, e0);
    pose_add_row(acc, wgt, J1, I1, e1);
    pose_add_row(acc, wgt, J2, I2, e2);
    acc[27] += (double)wgt;
    acc[28] += (double)(wgt * r2);
    acc[29] += 1.0;
  }
  const int lane = threadIdx.x & (DIS_WAVE - 1), wid = threadIdx.x / DIS_WAVE;
#pragma unroll
  for (int k = 0; k < POSE_SUMS; ++k) {
    const double s = wave_sum_d(acc[k]);           // valid in every lane
    if (lane == 0) wave_part[wid][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < POSE_REC) {
    double s = 0.0;
    if (threadIdx.x < POSE_SUMS) s = (wave_part[0][threadIdx.x] + wave_part[1][threadIdx.x]) + (wave_part[2][threadIdx.x] + wave_part[3][threadIdx.x]);
    partial[((size_t)pair * p.bpp + blk) * POSE_REC + threadIdx.x] = s;
  }
}

struct PoseSolveParams {
  int tl, bpp, min_corr;
  double damping;
};

__global__ __launch_bounds__(DIS_WAVE) void pose_solve_kernel(const double* __restrict__ partial, double* __restrict__ state,
                                                              float* __restrict__ R_pair, float* __restrict__ t_pair,
                                                              float* __restrict__ stats, const PoseSolveParams p, const int first,
                                                              const int last) {
  __shared__ double S[POSE_REC];
  const int pair = blockIdx.x;
  const int i = (pair % (p.tl * p.tl)) / p.tl, j = pair % p.tl;
  if (i == j) {
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
    // ascending workgroup order; the records are asked for POSE_BATCH at a time, so that the additions do not wait for one load each
    const double* rec = partial + (size_t)pair * p.bpp * POSE_REC + threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < p.bpp; k += POSE_BATCH) {
      double v[POSE_BATCH];
#pragma unroll
      for (int m = 0; m < POSE_BATCH; ++m) v[m] = rec[(size_t)min(k + m, p.bpp - 1) * POSE_REC];
#pragma unroll
      for (int m = 0; m < POSE_BATCH; ++m)
        if (k + m < p.bpp) s += v[m];
    }
    S[threadIdx.x] = s;
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
  if (!failed) {
    failed = S[29] < (double)p.min_corr;
    double L[6][6], d[6];
    if (!failed) {
      // Cholesky of H + damping diag(H), column by column; a pivot that is not > 0 or not finite ends the pair
      // (a bad pivot lets the remaining columns run on: their values are not used)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double hcc = S[pose_hidx(c, c)];
        double s = hcc + p.damping * hcc;
#pragma unroll
        for (int k = 0; k < c; ++k) s = s - L[c][k] * L[c][k];
        if (!(s > 0.0 && s <= 1.7976931348623157e308)) failed = true;
        L[c][c] = sqrt(s);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
          double q = S[pose_hidx(c, r)];
#pragma unroll
          for (int k = 0; k < c; ++k) q = q - L[r][k] * L[c][k];
          L[r][c] = q / L[c][c];
        }
      }
    }
    if (!failed) {
      double y[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s = -S[21 + r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - L[r][k] * y[k];
        y[r] = s / L[r][r];
      }
#pragma unroll
      for (int r = 5; r >= 0; --r) {
        double s = y[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s = s - L[k][r] * d[k];
        d[r] = s / L[r][r];
      }
      const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
      double ca = 1.0, cb = 0.5;
      if (!(th2 < 1e-16)) {
        const double th = sqrt(th2);
        ca = sin(th) / th;
        cb = (1.0 - cos(th)) / th2;
      }
      // dR = I + ca [w]x + cb [w]x^2, [w]x^2 = w w^T - th2 I
      double dR[9];
      const double Wx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          dR[3 * r + c] = ((r == c ? 1.0 : 0.0) + ca * Wx[3 * r + c]) + cb * (d[r] * d[c] - (r == c ? th2 : 0.0));
      double Rn[9], tn[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (dR[3 * r] * R[c] + dR[3 * r + 1] * R[3 + c]) + dR[3 * r + 2] * R[6 + c];
        tn[r] = ((dR[3 * r] * t[0] + dR[3 * r + 1] * t[1]) + dR[3 * r + 2] * t[2]) + d[3 + r];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = tn[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) st[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = failed ? 1.0 : 0.0;
}

struct PosePlan {
  long pairs;     // n tl tl, the diagonal included
  int bpp;
  long off_state, off_partial, bytes;
};

// false: unsupported extents
static bool pose_plan(int n, int tl, int h, int w, PosePlan* pl) {
  if (n < 1 || tl < 2 || tl > TRACK_MAX_TL || !track_image_ok(h, w, 2)) return false;
  if ((long)n * tl * tl * 2 * h * w > 0x7fffffffL) return false;
  pl->pairs = (long)n * tl * tl;
  int bpp = dis_cdiv((long)h * w, 4 * POSE_BLOCK);   // about four pixels per lane, until the cap
  if (bpp > POSE_MAX_BPP) bpp = POSE_MAX_BPP;
  pl->bpp = bpp;
  TrackCarver ws = {16, 0};
  pl->off_state = ws.take(pl->pairs * POSE_STATE * 8);
  pl->off_partial = ws.take(pl->pairs * bpp * POSE_REC * 8);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_pose_workspace(int n, int tl, int h, int w) {
  PosePlan pl;
  if (!pose_plan(n, tl, h, w, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_track_poses(const float* disp, const float* flow, const float* K4_host, float baseline, int iters, float scale,
                               float damping, int min_corr, float* R_pair, float* t_pair, float* stats, int n, int tl, int h, int w,
                               void* workspace, long workspace_bytes, void* stream) {
  if (!disp || !flow || !K4_host || !R_pair || !t_pair || !stats || !workspace) return DIS_ERR_NULL;
  PosePlan pl;
  if (!pose_plan(n, tl, h, w, &pl)) return DIS_ERR_BAD_SHAPE;
  PoseParams p;
  p.s2 = scale * scale;
  if (iters < 1 || iters > 64 || !track_pos_finite(scale) || !(damping >= 0.f && track_finite(damping)) || min_corr < 6 ||
      !track_camera(K4_host, baseline, &p.cam) || !track_pos_finite(p.s2) || workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15))
    return DIS_ERR_UNSUPPORTED;
  p.n = n, p.tl = tl, p.h = h, p.w = w, p.hw = h * w, p.bpp = pl.bpp;
  PoseSolveParams sp;
  sp.tl = tl, sp.bpp = pl.bpp, sp.min_corr = min_corr, sp.damping = (double)damping;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* state = (double*)(ws + pl.off_state);
  double* partial = (double*)(ws + pl.off_partial);
  const unsigned grid = (unsigned)(pl.pairs * pl.bpp);   // <= 2^31 / (2 * 4): pairs * bpp * 1024 <= pairs * (h w + 1023)
  for (int k = 0; k <= iters; ++k) {
    hipLaunchKernelGGL(pose_accum_kernel, dim3(grid), dim3(POSE_BLOCK), 0, st, disp, flow, (const double*)state, partial, p, k == 0 ? 1 : 0);
    DIS_CHECK_LAUNCH();
    hipLaunchKernelGGL(pose_solve_kernel, dim3((unsigned)pl.pairs), dim3(DIS_WAVE), 0, st, (const double*)partial, state, R_pair, t_pair,
                       stats, sp, k == 0 ? 1 : 0, k == iters ? 1 : 0);
    DIS_CHECK_LAUNCH();
  }
  return 0;
}
