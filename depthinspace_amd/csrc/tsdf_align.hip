// Frame-to-model pose refinement: the pose of every view refined against a truncated signed distance volume (include/dis_hip.h,
// section "volumetric fusion", dis_tsdf_align_poses): Gauss-Newton on the signed distance of the view's back-projected pixels to the
// surface of the volume - no flow, no second frame.  Every per-pixel term is a fixed fp32 expression in the operand order of
// tests/tsdf_align_ref.py, converted to fp64 and added in fp64; the state and the solve are fp64.  It joins the trilinear sampler of
// raycast.hip to the reduction and the 6 x 6 step of pose.hip (track_common.h holds both).  Two kernels, launched in turn iters + 1
// times; order and hand-off between them are held by the launch boundaries alone - no atomics, no flags polled between workgroups -
// so nothing depends on where workgroups are placed and two calls give the same bits.
//
//   tsdf_align_accum_kernel  bpp workgroups of 256 lanes per view.  A wave owns an 8 x 8 patch of the image and a workgroup 2 x 2 of
//                            them, as in raycast_march_kernel: the pixels of a patch land in the same or adjoining cells, so their
//                            eight weight bytes and eight tsdf floats fall into few lines.  The workgroups of a view take its 16 x 16
//                            tiles in turn (tile blk, blk + bpp, ...).  30 sums and the number of valid disparities in fp64
//                            registers; then the reduction of the pose kernels, one record of 32 doubles per workgroup.
//   tsdf_align_solve_kernel  one wave per view: lanes 0 .. 30 add the view's records in ascending workgroup order, lane 0 factors the
//                            6 x 6 system and updates the state; the opening launch also writes the opening statistics, the closing
//                            one only measures and writes R, t and the rest of stats.
// The first accumulate launch reads R_init instead of the state and the first solve launch starts from it, so the workspace needs no
// initialisation.
#include "track_common.h"

#define ALIGN_MAX_VIEWS 64
#define ALIGN_TILE 16          // pixels of a workgroup per side: 2 x 2 waves of 8 x 8
#define ALIGN_SUMS (POSE_SUMS + 1)   // [30]: the valid disparities

struct AlignParams {
  int nv, h, w, hw, nx, ny, nz, min_weight, bpp, tiles_x, tiles;
  TrackCamera cam;
  float ox, oy, oz, voxel, trunc, tv;    // tv = trunc / voxel
  float s2;                              // scale * scale
};

// One pixel of a view at the state (R, t): its point in the world, the trilinear tsdf and its gradient there, the 30 terms at the
// state's fp32 rounding, added to acc[] in fp64.  A pixel that is not used adds nothing but its valid count.
__device__ __forceinline__ void align_pixel(double* acc, const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                            const float d, const int u, const int v, const AlignParams& p, const float* R,
                                            const float* t) {
  if (!track_valid(d)) return;
  acc[30] += 1.0;
  float P[3], X[3];
  track_backproject(d, u, v, p.cam, P);
  track_to_world(R, t, P, X);
  const float gx = (X[0] - p.ox) / p.voxel, gy = (X[1] - p.oy) / p.voxel, gz = (X[2] - p.oz) / p.voxel;
  const RaySample s = ray_cell(gx, gy, gz, p);
  if (!s.inside) return;
  if (!ray_weights_ok(weight, s, p)) return;
  float c[8], gr[3];
  ray_corners(tsdf, s, p, c);
  const float sv = ray_trilinear(c, s);
  if (!(fabsf(sv) < 1.f)) return;                  // saturated free space has no gradient (false for NaN)
  ray_gradient(c, s, gr);
  const float e = p.trunc * sv;
  const float m0 = p.tv * gr[0], m1 = p.tv * gr[1], m2 = p.tv * gr[2];
  // the gradient of e in the camera's frame
  const float n0 = (R[0] * m0 + R[1] * m1) + R[2] * m2;
  const float n1 = (R[3] * m0 + R[4] * m1) + R[5] * m2;
  const float n2 = (R[6] * m0 + R[7] * m1) + R[8] * m2;
  const float J[6] = {n1 * P[2] - n2 * P[1], n2 * P[0] - n0 * P[2], n0 * P[1] - n1 * P[0], -n0, -n1, -n2};
  const int I[6] = {0, 1, 2, 3, 4, 5};
  const float e2 = e * e;
  const float g = 1.f / (1.f + e2 / p.s2);
  const float wgt = g * g;
  pose_add_row(acc, wgt, J, I, e);
  acc[27] += (double)wgt;
  acc[28] += (double)(wgt * e2);
  acc[29] += 1.0;
}

__global__ __launch_bounds__(POSE_BLOCK) void tsdf_align_accum_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                                      const float* __restrict__ disp, const float* __restrict__ R_init,
                                                                      const float* __restrict__ t_init, const double* __restrict__ state,
                                                                      double* __restrict__ partial, const AlignParams p, const int first) {
  const int f = blockIdx.x / p.bpp;                // the view: uniform over the workgroup
  const int blk = blockIdx.x % p.bpp;
  float R[9], t[3];
  if (first) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R_init[f * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t_init[f * 3 + k];
  } else {
    const double* s = state + (size_t)f * POSE_STATE;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (float)s[9 + k];
  }
  const float* df = disp + (size_t)f * p.hw;       // nv h w can pass 2^31
  const int wave = threadIdx.x / DIS_WAVE, lane = threadIdx.x & (DIS_WAVE - 1);
  const int du = (wave & 1) * 8 + (lane & 7), dv = (wave >> 1) * 8 + (lane >> 3);
  double acc[ALIGN_SUMS];
#pragma unroll
  for (int k = 0; k < ALIGN_SUMS; ++k) acc[k] = 0.0;
  for (int tile = blk; tile < p.tiles; tile += p.bpp) {
    const int u = (tile % p.tiles_x) * ALIGN_TILE + du, v = (tile / p.tiles_x) * ALIGN_TILE + dv;
    if (u < p.w && v < p.h) align_pixel(acc, tsdf, weight, df[v * p.w + u], u, v, p, R, t);
  }
  pose_block_record<ALIGN_SUMS>(acc, partial + ((size_t)f * p.bpp + blk) * POSE_REC);
}

struct AlignSolveParams {
  int bpp, min_corr;
  double damping;
};

// {pixels used, mean weight, weighted rms residual} of the sums S
__device__ __forceinline__ void align_stats(const double* S, float* __restrict__ o) {
  const double nc = S[29], sw = S[27], sc = S[28];
  o[0] = (float)nc;
  o[1] = nc > 0.0 ? (float)(sw / nc) : 0.f;
  o[2] = (nc > 0.0 && sw > 0.0) ? (float)sqrt(sc / sw) : 0.f;
}

__global__ __launch_bounds__(DIS_WAVE) void tsdf_align_solve_kernel(const double* __restrict__ partial, const float* __restrict__ R_init,
                                                                    const float* __restrict__ t_init, double* __restrict__ state,
                                                                    float* __restrict__ R_out, float* __restrict__ t_out,
                                                                    float* __restrict__ stats, const AlignSolveParams p, const int first,
                                                                    const int last) {
  __shared__ double S[POSE_REC];
  const int f = blockIdx.x;
  if (threadIdx.x < ALIGN_SUMS) S[threadIdx.x] = pose_sum_records(partial + (size_t)f * p.bpp * POSE_REC + threadIdx.x, p.bpp);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* st = state + (size_t)f * POSE_STATE;
  double R[9], t[3];
  bool failed = false;
  if (first) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)R_init[f * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (double)t_init[f * 3 + k];
    align_stats(S, stats + (size_t)f * 8 + 4);     // the opening pass, at R_init
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = st[9 + k];
    failed = st[12] != 0.0;
  }
  if (last) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R_out[f * 9 + k] = (float)R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t_out[f * 3 + k] = (float)t[k];
    align_stats(S, stats + (size_t)f * 8);
    stats[(size_t)f * 8 + 3] = failed ? 0.f : 1.f;
    stats[(size_t)f * 8 + 7] = (float)S[30];
    return;
  }
  if (!failed) failed = !pose_gn_step(S, p.min_corr, p.damping, R, t);
#pragma unroll
  for (int k = 0; k < 9; ++k) st[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = failed ? 1.0 : 0.0;
}

struct AlignPlan {
  int bpp;
  long off_state, off_partial, bytes;
};

// false: unsupported extents
static bool align_plan(int nv, int h, int w, AlignPlan* pl) {
  if (nv < 1 || nv > ALIGN_MAX_VIEWS || !track_image_ok(h, w, 2)) return false;
  pl->bpp = pose_bpp(h, w);
  TrackCarver ws = {16, 0};
  pl->off_state = ws.take((long)nv * POSE_STATE * 8);
  pl->off_partial = ws.take((long)nv * pl->bpp * POSE_REC * 8);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_tsdf_align_workspace(int nv, int h, int w) {
  AlignPlan pl;
  if (!align_plan(nv, h, w, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_tsdf_align_poses(const float* tsdf, const unsigned char* weight, const float* origin3_host, float voxel, float trunc,
                                    int min_weight, const float* disp, const float* K4_host, float baseline, const float* R_init,
                                    const float* t_init, int iters, float scale, float damping, int min_corr, float* R, float* t,
                                    float* stats, int nv, int h, int w, int nx, int ny, int nz, void* workspace, long workspace_bytes,
                                    void* stream) {
  if (!tsdf || !weight || !origin3_host || !disp || !K4_host || !R_init || !t_init || !R || !t || !stats || !workspace) return DIS_ERR_NULL;
  AlignPlan pl;
  if (!align_plan(nv, h, w, &pl) || !tsdf_grid_ok(nx, ny, nz)) return DIS_ERR_BAD_SHAPE;
  AlignParams p;
  p.s2 = scale * scale;
  p.tv = trunc / voxel;
  if (iters < 1 || iters > 64 || !track_pos_finite(scale) || !track_pos_finite(voxel) || !track_pos_finite(trunc) ||
      !(damping >= 0.f && track_finite(damping)) || min_corr < 6 || min_weight < 1 || min_weight > TRACK_MAX_TL ||
      !track_camera(K4_host, baseline, &p.cam) || !tsdf_origin(origin3_host, &p.ox, &p.oy, &p.oz) || !track_pos_finite(p.s2) ||
      !track_pos_finite(p.tv) || workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15))
    return DIS_ERR_UNSUPPORTED;
  p.nv = nv, p.h = h, p.w = w, p.hw = h * w, p.nx = nx, p.ny = ny, p.nz = nz, p.min_weight = min_weight, p.bpp = pl.bpp;
  p.tiles_x = dis_cdiv(w, ALIGN_TILE), p.tiles = p.tiles_x * dis_cdiv(h, ALIGN_TILE);
  p.voxel = voxel, p.trunc = trunc;
  AlignSolveParams sp;
  sp.bpp = pl.bpp, sp.min_corr = min_corr, sp.damping = (double)damping;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* state = (double*)(ws + pl.off_state);
  double* partial = (double*)(ws + pl.off_partial);
  const unsigned grid = (unsigned)(nv * pl.bpp);   // <= 64 * 128
  for (int k = 0; k <= iters; ++k) {
    hipLaunchKernelGGL(tsdf_align_accum_kernel, dim3(grid), dim3(POSE_BLOCK), 0, st, tsdf, weight, disp, R_init, t_init, (const double*)state,
                       partial, p, k == 0 ? 1 : 0);
    DIS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_align_solve_kernel, dim3((unsigned)nv), dim3(DIS_WAVE), 0, st, (const double*)partial, R_init, t_init, state, R, t,
                       stats, sp, k == 0 ? 1 : 0, k == iters ? 1 : 0);
    DIS_CHECK_LAUNCH();
  }
  return 0;
}
