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
// The second half of the file is the joint refinement, dis_refine_track_poses: one pose per frame on the residuals of all pairs at once,
// through the same per-pixel function (pose_pixel) and the same reduction (pose_block_record).
// The reduction, the record sum and the 6 x 6 step (pose_hidx, pose_add_row, pose_block_record, pose_sum_records, pose_gn_step,
// pose_apply_twist) live in track_common.h: tsdf_align.hip runs its own per-pixel terms through them.
#include "track_common.h"

struct PoseParams {
  int n, tl, h, w, hw, bpp;              // bpp = workgroups per pair
  TrackCamera cam;
  float s2;                              // scale * scale
};

// One pixel of the pair (i, j) at the state (R, t): its target in frame j (its disparity, its flow, four gathered disparities of frame j),
// the 30 terms at the state's fp32 rounding, added to acc[] in fp64.  A pixel that is not matched or not used adds nothing.  The one
// statement of the per-pixel expressions: pose_accum_kernel and pose_joint_accum_kernel both call it.
__device__ __forceinline__ void pose_pixel(double* acc, const float* __restrict__ di, const float* __restrict__ dj,
                                           const float* __restrict__ fl, const int pix, const PoseParams& p, const float* R, const float* t,
                                           const int first) {
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
  if (!(in && track_valid(d00) && track_valid(d01) && track_valid(d10) && track_valid(d11))) return;   // not matched: nothing is added
  const float ax = uj - (float)x0, ay = vj - (float)y0;
  const float gx = 1.f - ax, gy = 1.f - ay;
  const float ds = (d00 * gx + d01 * ax) * gy + (d10 * gx + d11 * ax) * ay;
  float P[3], X[3];
  track_backproject(d, u, v, p.cam, P);
  track_to_camera(R, t, P, X);
  const float X0 = X[0], X1 = X[1], X2 = X[2];
  if (!(X2 > 0.f)) return;                         // not used
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

__global__ __launch_bounds__(POSE_BLOCK) void pose_accum_kernel(const float* __restrict__ disp, const float* __restrict__ flow,
                                                                const double* __restrict__ state, double* __restrict__ partial,
                                                                const PoseParams p, const int first) {
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
  for (int pix = blk * POSE_BLOCK + (int)threadIdx.x; pix < p.hw; pix += p.bpp * POSE_BLOCK) pose_pixel(acc, di, dj, fl, pix, p, R, t, first);
  pose_block_record<POSE_SUMS>(acc, partial + ((size_t)pair * p.bpp + blk) * POSE_REC);
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
  if (threadIdx.x < POSE_SUMS) S[threadIdx.x] = pose_sum_records(partial + (size_t)pair * p.bpp * POSE_REC + threadIdx.x, p.bpp);
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
  const int bpp = pl->bpp = pose_bpp(h, w);
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

// ------------------------------------------------------------------------------------------------ joint refinement
// dis_refine_track_poses: one pose per frame (frame 0 fixed), refined on the residuals of every used ordered pair at once.  The same two
// launches in turn, iters + 1 times, the hand-off again the launch boundary alone.
//
//   pose_joint_accum_kernel  the grid and the reduction of pose_accum_kernel; the pair's state is composed in fp64 from the poses of its
//                            two frames (the init in the first launch), by every lane alike, and rounded to fp32 for pose_pixel.  A
//                            pair that is not used leaves like a diagonal one and writes no record.
//   pose_joint_solve_kernel  one workgroup of sixteen waves per track.  A wave per pair adds the pair's records as pose_solve_kernel
//                            does (with four waves taking the pairs in turn the sums alone took 17 us, profiles/pose_rate.md); then every
//                            step is spread over the lanes with the operands in LDS: the pairs' transforms, the products M = H Ad,
//                            N = Ad^T M, q = Ad^T g (a lane per element, k = 0 .. 5 in order, the elements of Ad formed where they are used),
//                            the system (a lane per element of A and b, the pairs in ascending (i, j)), the factorisation (a lane per
//                            row, a column at a time, the pivot handed round the wave), the two substitutions (a lane per unknown),
//                            and the update (a lane per frame).  The closing launch stops after the sums and writes the outputs.
#define POSEJ_FRAME 16                               // doubles per frame of the state: R (9, row-major), t (3); [12] of frame 0: the track has failed
#define POSEJ_TRACK (TRACK_MAX_TL * POSEJ_FRAME)
#define POSEJ_PAIRS (TRACK_MAX_TL * TRACK_MAX_TL)
#define POSEJ_ORDER (6 * (TRACK_MAX_TL - 1))
#define POSEJ_DBL_MAX 1.7976931348623157e308
#define POSEJ_BLOCK 1024                             // lanes of the solve workgroup: a wave per pair of the longest track
#define POSEJ_WAVES (POSEJ_BLOCK / DIS_WAVE)

// R_ij = R_j R_i^T and t_ij = t_j - R_ij t_i, an element each: the operand order of tests/pose_joint_ref.py (compose)
__device__ __forceinline__ double posej_Rij(const double* Ri, const double* Rj, const int r, const int c) {
  return (Rj[3 * r] * Ri[3 * c] + Rj[3 * r + 1] * Ri[3 * c + 1]) + Rj[3 * r + 2] * Ri[3 * c + 2];
}
__device__ __forceinline__ double posej_tij(const double* Ri, const double* ti, const double* Rj, const double* tj, const int r) {
  return tj[r] - ((posej_Rij(Ri, Rj, r, 0) * ti[0] + posej_Rij(Ri, Rj, r, 1) * ti[1]) + posej_Rij(Ri, Rj, r, 2) * ti[2]);
}

// v of lane `lane` of the wave, `lane` uniform: two scalar lane reads, where __shfl would go through LDS once per use in a dependent chain
__device__ __forceinline__ double posej_lane(const double v, const int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// element (r, c) of Ad = [[R, 0], [[t]x R, R]] for the pair P = {R_ij (9, row-major), t_ij (3)}
__device__ __forceinline__ double posej_ad(const double* P, const int r, const int c) {
  const double* R = P;
  const double* t = P + 9;
  if (r / 3 == c / 3) return R[3 * (r % 3) + c % 3];
  if (r < 3) return 0.0;
  const int r1 = (r - 2) % 3, r2 = (r - 1) % 3;      // (r - 3) + 1 and (r - 3) + 2, cyclic
  return t[r1] * R[3 * r2 + c] - t[r2] * R[3 * r1 + c];
}

// element k of frame f's pose (R row-major 0 .. 8, t 9 .. 11) in fp64: the init in the first launches, the state afterwards
__device__ __forceinline__ double posej_frame(const float* __restrict__ R_init, const float* __restrict__ t_init,
                                              const double* __restrict__ state, const int b, const int tl, const int f, const int k,
                                              const int first) {
  if (!first) return state[(size_t)b * POSEJ_TRACK + f * POSEJ_FRAME + k];
  return k < 9 ? (double)R_init[((size_t)b * tl + f) * 9 + k] : (double)t_init[((size_t)b * tl + f) * 3 + (k - 9)];
}

__global__ __launch_bounds__(POSE_BLOCK) void pose_joint_accum_kernel(const float* __restrict__ disp, const float* __restrict__ flow,
                                                                      const float* __restrict__ R_init, const float* __restrict__ t_init,
                                                                      const double* __restrict__ state,
                                                                      const unsigned char* __restrict__ pair_use,
                                                                      double* __restrict__ partial, const PoseParams p, const int first) {
  const int pair = blockIdx.x / p.bpp;             // (b tl + i) tl + j: uniform over the workgroup
  const int blk = blockIdx.x % p.bpp;
  const int tt = p.tl * p.tl;
  const int b = pair / tt, i = (pair % tt) / p.tl, j = pair % p.tl;
  if (i == j || (pair_use && !pair_use[pair])) return;     // (the whole workgroup: no barrier is passed by a part of it)
  double Fi[12], Fj[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    Fi[k] = posej_frame(R_init, t_init, state, b, p.tl, i, k, first);
    Fj[k] = posej_frame(R_init, t_init, state, b, p.tl, j, k, first);
  }
  float R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (float)posej_Rij(Fi, Fj, r, c);
    t[r] = (float)posej_tij(Fi, Fi + 9, Fj, Fj + 9, r);
  }
  const float* di = disp + (b * p.tl + i) * p.hw;          // n tl tl 2 h w < 2^31: checked on the host
  const float* dj = disp + (b * p.tl + j) * p.hw;
  const float* fl = flow + pair * 2 * p.hw;
  double acc[POSE_SUMS];
#pragma unroll
  for (int k = 0; k < POSE_SUMS; ++k) acc[k] = 0.0;
  for (int pix = blk * POSE_BLOCK + (int)threadIdx.x; pix < p.hw; pix += p.bpp * POSE_BLOCK) pose_pixel(acc, di, dj, fl, pix, p, R, t, 0);
  pose_block_record<POSE_SUMS>(acc, partial + ((size_t)pair * p.bpp + blk) * POSE_REC);
}

__global__ __launch_bounds__(POSEJ_BLOCK) void pose_joint_solve_kernel(const double* __restrict__ partial, const float* __restrict__ R_init,
                                                                      const float* __restrict__ t_init,
                                                                      const unsigned char* __restrict__ pair_use, double* __restrict__ state,
                                                                      float* __restrict__ R_out, float* __restrict__ t_out,
                                                                      float* __restrict__ pair_stats, float* __restrict__ track_stats,
                                                                      const PoseSolveParams p, const int first, const int last) {
  __shared__ double S[POSEJ_PAIRS][POSE_REC];      // the sums of every pair
  __shared__ double F[TRACK_MAX_TL][12];           // the frames: R, t
  __shared__ double Pr[POSEJ_PAIRS][12];           // the pairs: R_ij, t_ij
  __shared__ double M[POSEJ_PAIRS][36], N[POSEJ_PAIRS][36], Q[POSEJ_PAIRS][6];
  __shared__ double A[POSEJ_ORDER][POSEJ_ORDER], L[POSEJ_ORDER][POSEJ_ORDER], Linv[POSEJ_ORDER], bv[POSEJ_ORDER], dv[POSEJ_ORDER];
  __shared__ int contrib[POSEJ_PAIRS];
  __shared__ int failed_s;
  const int b = blockIdx.x, tid = threadIdx.x, tl = p.tl, tt = tl * tl, m = 6 * (tl - 1);
  const int lane = tid & (DIS_WAVE - 1), wid = tid / DIS_WAVE;
  if (tid < tl * 12) F[tid / 12][tid % 12] = posej_frame(R_init, t_init, state, b, tl, tid / 12, tid % 12, first);
  if (tid == 0) failed_s = first ? 0 : (state[(size_t)b * POSEJ_TRACK + 12] != 0.0 ? 1 : 0);
  for (int pr = wid; pr < tt; pr += POSEJ_WAVES) {         // a pair per wave at a time
    const bool used = pr / tl != pr % tl && (!pair_use || pair_use[(size_t)b * tt + pr]);
    if (lane < POSE_REC) {
      double s = 0.0;
      if (used && lane < POSE_SUMS) s = pose_sum_records(partial + ((size_t)b * tt + pr) * p.bpp * POSE_REC + lane, p.bpp);
      S[pr][lane] = s;
    }
  }
  __syncthreads();
  if (tid < tt) {
    const bool used = tid / tl != tid % tl && (!pair_use || pair_use[(size_t)b * tt + tid]);
    contrib[tid] = (used && S[tid][29] >= (double)p.min_corr) ? 1 : 0;
  }
  if (last) {
    __syncthreads();
    if (tid < tl * 9) R_out[(size_t)b * tl * 9 + tid] = (float)F[tid / 9][tid % 9];
    if (tid < tl * 3) t_out[(size_t)b * tl * 3 + tid] = (float)F[tid / 3][9 + tid % 3];
    if (tid < tt) {
      const double nc = S[tid][29], sw = S[tid][27], sc = S[tid][28];    // zeros for a pair that is not used
      float* ps = pair_stats + ((size_t)b * tt + tid) * 4;
      const bool diag = tid / tl == tid % tl;
      ps[0] = (float)nc;
      ps[1] = nc > 0.0 ? (float)(sw / nc) : 0.f;
      ps[2] = (nc > 0.0 && sw > 0.0) ? (float)sqrt(sc / sw) : 0.f;
      ps[3] = (diag || contrib[tid]) ? 1.f : 0.f;
    }
    if (tid == 0) {
      double pairs = 0.0, tn = 0.0, tw = 0.0, tc = 0.0;
      for (int pr = 0; pr < tt; ++pr)              // ascending (i, j)
        if (contrib[pr]) pairs += 1.0, tn += S[pr][29], tw += S[pr][27], tc += S[pr][28];
      float* ts = track_stats + (size_t)b * 4;
      ts[0] = (float)pairs;
      ts[1] = (float)tn;
      ts[2] = tw > 0.0 ? (float)sqrt(tc / tw) : 0.f;
      ts[3] = failed_s ? 0.f : 1.f;
    }
    return;
  }
  // the pairs' transforms and adjoints at the state
  if (tid < tt * 12) {
    const int pr = tid / 12, k = tid % 12, i = pr / tl, j = pr % tl;
    Pr[pr][k] = k < 9 ? posej_Rij(F[i], F[j], k / 3, k % 3) : posej_tij(F[i], F[i] + 9, F[j], F[j] + 9, k - 9);
  }
  __syncthreads();
  bool failed = failed_s != 0;                     // uniform
  if (!failed) {
    // M = H Ad
    for (int e = tid; e < tt * 36; e += POSEJ_BLOCK) {
      const int pr = e / 36, r = (e % 36) / 6, c = e % 6;
      double a = S[pr][pose_hidx(0, r)] * posej_ad(Pr[pr], 0, c);
#pragma unroll
      for (int k = 1; k < 6; ++k) a = a + S[pr][pose_hidx(min(r, k), max(r, k))] * posej_ad(Pr[pr], k, c);
      M[pr][e % 36] = a;
    }
    __syncthreads();
    // N = Ad^T M, q = Ad^T g
    for (int e = tid; e < tt * 42; e += POSEJ_BLOCK) {
      const int pr = e / 42, x = e % 42;
      if (x < 36) {
        const int r = x / 6, c = x % 6;
        double a = posej_ad(Pr[pr], 0, r) * M[pr][c];
#pragma unroll
        for (int k = 1; k < 6; ++k) a = a + posej_ad(Pr[pr], k, r) * M[pr][6 * k + c];
        N[pr][x] = a;
      } else {
        const int r = x - 36;
        double a = posej_ad(Pr[pr], 0, r) * S[pr][21];
#pragma unroll
        for (int k = 1; k < 6; ++k) a = a + posej_ad(Pr[pr], k, r) * S[pr][21 + k];
        Q[pr][r] = a;
      }
    }
    __syncthreads();
    // the system without frame 0: an element of A or of b per lane, the contributing pairs in ascending (i, j)
    for (int e = tid; e < m * m + m; e += POSEJ_BLOCK) {
      const bool isb = e >= m * m;
      const int row = isb ? e - m * m : e / m, col = isb ? 0 : e % m;
      const int fa = row / 6 + 1, fb = col / 6 + 1, r = row % 6, c = col % 6;
      double a = 0.0;
      for (int pr = 0; pr < tt; ++pr) {
        if (!contrib[pr]) continue;
        const int i = pr / tl, j = pr % tl;
        if (isb) {
          if (fa == j) a = a + S[pr][21 + r];
          else if (fa == i) a = a - Q[pr][r];
        } else if (fa == fb) {
          if (fa == j) a = a + S[pr][pose_hidx(min(r, c), max(r, c))];
          else if (fa == i) a = a + N[pr][6 * r + c];
        } else if (fa == j && fb == i) a = a - M[pr][6 * r + c];
        else if (fa == i && fb == j) a = a - M[pr][6 * c + r];
      }
      if (isb) bv[row] = a;
      else A[row][col] = a;
    }
    __syncthreads();
    // Cholesky of A + damping diag(A): lane r holds row r; column c needs the columns before it.  A pivot that is not > 0 or not finite
    // ends the track (the remaining columns run on: their values are not used).  Only wave 0 works; the others keep the barriers.
    bool bad = false;
    for (int c = 0; c < m; ++c) {
      double s = 0.0;
      if (tid >= c && tid < m) {
        s = A[tid][c];
        if (tid == c) s = s + p.damping * s;
#pragma unroll
        for (int k = 0; k < POSEJ_ORDER; ++k) {    // every load is asked for at once; the columns from c on are dropped (a select)
          const double x = L[tid][k] * L[c][k];
          if (k < c) s = s - x;
        }
      }
      const double piv = posej_lane(s, c);
      if (!(piv > 0.0 && piv <= POSEJ_DBL_MAX)) bad = true;
      const double lcc = sqrt(piv);
      if (tid >= c && tid < m) L[tid][c] = tid == c ? lcc : s / lcc;
      if (tid == c) Linv[c] = 1.0 / lcc;
      __syncthreads();
    }
    // L y = -b with k ascending, L^T d = y with k descending: a solved unknown - its row's sum times 1 / L_kk - goes round the wave and
    // leaves the rows below / above.  Unrolled to the largest order, so that the loads of L do not wait in the chain; steps at and past
    // m change nothing.
    const int row = min(tid, POSEJ_ORDER - 1);
    double s = tid < m ? -bv[tid] : 0.0, y = 0.0, d = 0.0;
#pragma unroll
    for (int k = 0; k < POSEJ_ORDER; ++k) {
      const double lrk = L[row][k];
      const double yk = posej_lane(s, k) * Linv[k];
      if (tid == k) y = yk;
      if (k < m && tid > k && tid < m) s = s - lrk * yk;
    }
    s = y;
#pragma unroll
    for (int k = POSEJ_ORDER - 1; k >= 0; --k) {
      const double lkr = L[k][row];
      const double dk = posej_lane(s, k) * Linv[k];
      if (tid == k) d = dk;
      if (k < m && tid < k) s = s - lkr * dk;
    }
    if (tid < m) dv[tid] = d;
    if (tid == 0) failed_s = bad ? 1 : 0;          // (wave 0 holds the pivots)
    __syncthreads();
    failed = failed_s != 0;
    if (!failed && tid >= 1 && tid < tl) {
      // the update of pose_solve_kernel, frame tid
      pose_apply_twist(dv + 6 * (tid - 1), F[tid], F[tid] + 9);
    }
    __syncthreads();
  }
  if (tid < tl * 12) state[(size_t)b * POSEJ_TRACK + (tid / 12) * POSEJ_FRAME + tid % 12] = F[tid / 12][tid % 12];
  if (tid == 0) state[(size_t)b * POSEJ_TRACK + 12] = failed ? 1.0 : 0.0;
}

struct PoseJointPlan {
  long pairs;     // n tl tl, the diagonal included
  int bpp;
  long off_state, off_partial, bytes;
};

// false: unsupported extents (those of pose_plan)
static bool pose_joint_plan(int n, int tl, int h, int w, PoseJointPlan* pl) {
  PosePlan pp;
  if (!pose_plan(n, tl, h, w, &pp)) return false;
  pl->pairs = pp.pairs, pl->bpp = pp.bpp;
  TrackCarver ws = {16, 0};
  pl->off_state = ws.take((long)n * POSEJ_TRACK * 8);
  pl->off_partial = ws.take(pl->pairs * pl->bpp * POSE_REC * 8);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_pose_joint_workspace(int n, int tl, int h, int w) {
  PoseJointPlan pl;
  if (!pose_joint_plan(n, tl, h, w, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_refine_track_poses(const float* disp, const float* flow, const float* K4_host, float baseline, const float* R_init,
                                      const float* t_init, const unsigned char* pair_use, int iters, float scale, float damping,
                                      int min_corr, float* R, float* t, float* pair_stats, float* track_stats, int n, int tl, int h, int w,
                                      void* workspace, long workspace_bytes, void* stream) {
  if (!disp || !flow || !K4_host || !R_init || !t_init || !R || !t || !pair_stats || !track_stats || !workspace) return DIS_ERR_NULL;
  PoseJointPlan pl;
  if (!pose_joint_plan(n, tl, h, w, &pl)) return DIS_ERR_BAD_SHAPE;
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
  const unsigned grid = (unsigned)(pl.pairs * pl.bpp);   // as in dis_track_poses
  for (int k = 0; k <= iters; ++k) {
    hipLaunchKernelGGL(pose_joint_accum_kernel, dim3(grid), dim3(POSE_BLOCK), 0, st, disp, flow, R_init, t_init, (const double*)state,
                       pair_use, partial, p, k == 0 ? 1 : 0);
    DIS_CHECK_LAUNCH();
    hipLaunchKernelGGL(pose_joint_solve_kernel, dim3((unsigned)n), dim3(POSEJ_BLOCK), 0, st, (const double*)partial, R_init, t_init, pair_use,
                       state, R, t, pair_stats, track_stats, sp, k == 0 ? 1 : 0, k == iters ? 1 : 0);
    DIS_CHECK_LAUNCH();
  }
  return 0;
}
