// A truncated signed distance volume cast back into cameras: per pixel of every view the first zero crossing of the trilinear tsdf along
// the pixel's ray -> disparity, the normal and the carried value there (include/dis_hip.h, section "volumetric fusion",
// dis_tsdf_raycast): fp32, every operation a fixed expression in the operand order of tests/raycast_ref.py.  No atomics, no flags
// polled between workgroups: the launch boundaries alone order the passes, so two calls give the same bits.
//
//   raycast_state_kernel   one byte per cell: 0 a corner weight below min_weight, 1 all corners observed and none negative, 2 all
//                          observed and one negative.  The eight-corner stencil of a 256-point block is staged in LDS as the flags pass
//                          of tsdf.hip stages it (four linear rows of 257).  With a, b >= 0 and 0 <= f < 1 the form a + f (b - a) is
//                          never negative in fp32 (|f (b - a)| <= |b - a| <= a where b < a), so a trilinear value can be negative only in
//                          a state-2 cell.
//   raycast_brick_kernel   one workgroup per brick of 8 x 8 x 8 cells: its number of state-2 cells, by ballots.  0: the brick is dead.
//   raycast_march_kernel   a wave per 8 x 8 tile of pixels (its rays cross the same bricks, its gathers fall into few lines), four waves
//                          per workgroup, the loop runs until the wave's ballot of unfinished rays is empty.
//       variant 1 (plain)  every sample reads its eight weights and, where they suffice, its eight tsdf corners.
//       variant 0          every sample reads its cell's state byte and gathers the corners only in a state-2 cell.  In a dead brick the
//                          ray first jumps to the last sample index that an estimate of the brick's exit depth (less a guard of one
//                          sample) names - after that sample's own cell, formed by the expressions every sample uses, has been found to
//                          lie in the same brick.  The lattice coordinates of a ray are monotonic in n in fp32 (every operation on the
//                          way from n is a rounding of a monotonic function), so all samples between two samples of a brick lie in it:
//                          a jump skips samples of the dead brick only, none of which can be n*, and the state of the sample it lands
//                          on says whether n* - 1 is valid.
//     Both variants end in the same code - s(n* - 1) and s(n*) gathered again, the crossing, the gradient, the value - so they give the
//     same bits.
// The cell rule and the sampler (ray_cell, ray_corners, ray_trilinear, ray_gradient, ray_weights_ok) live in track_common.h:
// tsdf_align.hip samples the volume through them too.
#include "track_common.h"

#define RAY_BLOCK TRACK_BLOCK
#define RAY_TILE 16          // pixels of a workgroup per side: 2 x 2 waves of 8 x 8
#define RAY_BRICK 8
#define RAY_MAX_VIEWS 64
#define RAY_MAX_N 16777215   // 2^24 - 1: float(n) is exact

struct RayParams {
  int nv, h, w, hw, nx, ny, nz, total, min_weight;
  int cx, cy, cz;   // cells per axis
  int bx, by, bz;   // bricks per axis
  TrackCamera cam;
  float ox, oy, oz, voxel, step;
};

__global__ __launch_bounds__(RAY_BLOCK) void raycast_state_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                                  unsigned char* __restrict__ state, const RayParams p) {
  __shared__ float sf[4][RAY_BLOCK + 4];
  __shared__ unsigned char sw[4][RAY_BLOCK + 4];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * RAY_BLOCK;
  const int nxy = p.nx * p.ny;
  // rows dy + 2 dz of the stencil: 257 points each; a point past the end of the volume belongs to no cell's stencil
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int off = (s & 1) * p.nx + (s >> 1) * nxy;
    const long g = (long)b0 + off + tid;
    const bool ok = g < p.total;
    sf[s][tid] = ok ? tsdf[g] : 1.f;
    sw[s][tid] = ok ? weight[g] : 0;
  }
  if (tid < 4) {
    const int off = (tid & 1) * p.nx + (tid >> 1) * nxy;
    const long g = (long)b0 + off + RAY_BLOCK;
    const bool ok = g < p.total;
    sf[tid][RAY_BLOCK] = ok ? tsdf[g] : 1.f;
    sw[tid][RAY_BLOCK] = ok ? weight[g] : 0;
  }
  __syncthreads();
  const int l = b0 + tid;
  if (l >= p.total) return;
  const int i = l % p.nx, r = l / p.nx;
  const int j = r % p.ny, k = r / p.ny;
  if (i > p.nx - 2 || j > p.ny - 2 || k > p.nz - 2) return;   // no cell
  bool allok = true, anyneg = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int s = ((c >> 1) & 1) + 2 * (c >> 2), e = tid + (c & 1);
    anyneg = anyneg || sf[s][e] < 0.f;
    allok = allok && (int)sw[s][e] >= p.min_weight;
  }
  state[((size_t)k * p.cy + j) * p.cx + i] = (unsigned char)(allok ? (anyneg ? 2 : 1) : 0);
}

__global__ __launch_bounds__(RAY_BLOCK) void raycast_brick_kernel(const unsigned char* __restrict__ state, int* __restrict__ brick,
                                                                  const RayParams p) {
  const int b = blockIdx.x;
  const int bi = b % p.bx, r = b / p.bx;
  const int bj = r % p.by, bk = r / p.by;
  int cnt = 0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int c = threadIdx.x + half * RAY_BLOCK;   // 512 cells, x fastest
    const int i = bi * RAY_BRICK + (c & 7), j = bj * RAY_BRICK + ((c >> 3) & 7), k = bk * RAY_BRICK + (c >> 6);
    const bool in = i < p.cx && j < p.cy && k < p.cz;
    const bool live = in && state[((size_t)k * p.cy + j) * p.cx + i] == 2;
    cnt += __popcll(__ballot(live));
  }
  track_block_count(cnt, brick);
}

struct Ray {
  float o0, o1, o2, d0, d1, d2;
};

// sample n of the ray: z_n = float(n) step, g_a = ((o_a + z_n d_a) - origin_a) / voxel; inside: 0 <= g_a < float(n_a - 1), as floats
__device__ __forceinline__ RaySample ray_sample(int n, const Ray& q, const RayParams& p) {
  const float z = (float)n * p.step;
  const float gx = ((q.o0 + z * q.d0) - p.ox) / p.voxel;
  const float gy = ((q.o1 + z * q.d1) - p.oy) / p.voxel;
  const float gz = ((q.o2 + z * q.d2) - p.oz) / p.voxel;
  return ray_cell(gx, gy, gz, p);
}

// [0, 2^24] as an int, whatever q is (NaN: 0)
__device__ __forceinline__ int ray_index(float q) { return (int)fminf(fmaxf(q, 0.f), 16777216.f); }

// one axis of the slab test in lattice units against [-e, float(n - 1) + e]; false: the ray never comes near the lattice
__device__ __forceinline__ bool ray_slab(float go, float gd, float e, int n, float* tmin, float* tmax) {
  const float lo = -e, hi = (float)(n - 1) + e;
  if (gd != 0.f) {
    const float ta = (lo - go) / gd, tb = (hi - go) / gd;
    *tmin = fmaxf(*tmin, fminf(ta, tb));
    *tmax = fminf(*tmax, fmaxf(ta, tb));
    return true;
  }
  return go >= lo && go <= hi;
}

// the depth at which the ray leaves [lo, hi) along one axis (an estimate: the caller verifies the sample it leads to)
__device__ __forceinline__ float ray_exit(float go, float gd, float rgd, float lo, float hi) {
  return gd > 0.f ? (hi - go) * rgd : (gd < 0.f ? (lo - go) * rgd : TRACK_FLT_MAX);
}

template <int VARIANT>
__global__ __launch_bounds__(RAY_BLOCK) void raycast_march_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                                  const float* __restrict__ vvalue, const unsigned char* __restrict__ state,
                                                                  const int* __restrict__ brick, const float* __restrict__ R,
                                                                  const float* __restrict__ t, float* __restrict__ disp_o,
                                                                  float* __restrict__ normal_o, float* __restrict__ value_o,
                                                                  const RayParams p) {
  const int f = blockIdx.z;
  const int wave = threadIdx.x / DIS_WAVE, lane = threadIdx.x & (DIS_WAVE - 1);
  const int u = blockIdx.x * RAY_TILE + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * RAY_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool pixel = u < p.w && v < p.h;
  const float* Rf = R + f * 9;
  const float* tf = t + f * 3;
  const float dc0 = ((float)u - p.cam.cx) / p.cam.fx, dc1 = ((float)v - p.cam.cy) / p.cam.fy;   // dc2 = 1
  Ray q;
  q.o0 = -((Rf[0] * tf[0] + Rf[3] * tf[1]) + Rf[6] * tf[2]);
  q.o1 = -((Rf[1] * tf[0] + Rf[4] * tf[1]) + Rf[7] * tf[2]);
  q.o2 = -((Rf[2] * tf[0] + Rf[5] * tf[1]) + Rf[8] * tf[2]);
  q.d0 = (Rf[0] * dc0 + Rf[3] * dc1) + Rf[6];
  q.d1 = (Rf[1] * dc0 + Rf[4] * dc1) + Rf[7];
  q.d2 = (Rf[2] * dc0 + Rf[5] * dc1) + Rf[8];
  // the ray in lattice units, for the range of n and the jumps only: no result is formed from these
  const float go0 = (q.o0 - p.ox) / p.voxel, go1 = (q.o1 - p.oy) / p.voxel, go2 = (q.o2 - p.oz) / p.voxel;
  const float gd0 = q.d0 / p.voxel, gd1 = q.d1 / p.voxel, gd2 = q.d2 / p.voxel;
  // a conservative range of n: the slabs of the lattice box, each widened by a cell and by 2^-17 of the magnitudes a lattice
  // coordinate is formed from (its rounding error is below 2^-20 of them), the range by 2^-16 of itself and three samples
  const float k17 = 1.f / 131072.f;
  float tmin = 0.f, tmax = TRACK_FLT_MAX;
  bool near = ray_slab(go0, gd0, 1.f + k17 * ((fabsf(q.o0) + fabsf(p.ox)) / p.voxel + (float)p.nx), p.nx, &tmin, &tmax);
  near = ray_slab(go1, gd1, 1.f + k17 * ((fabsf(q.o1) + fabsf(p.oy)) / p.voxel + (float)p.ny), p.ny, &tmin, &tmax) && near;
  near = ray_slab(go2, gd2, 1.f + k17 * ((fabsf(q.o2) + fabsf(p.oz)) / p.voxel + (float)p.nz), p.nz, &tmin, &tmax) && near;
  // a ray that is not finite has no sample inside, and one without a direction has the same sample for every n: neither can hit
  near = near && tmin <= tmax && track_finite(q.o0) && track_finite(q.o1) && track_finite(q.o2) && track_finite(q.d0) &&
         track_finite(q.d1) && track_finite(q.d2) && (q.d0 != 0.f || q.d1 != 0.f || q.d2 != 0.f);
  const int n_hi = min(RAY_MAX_N, ray_index((tmax / p.step) * (1.f + 1.f / 65536.f)) + 3);
  int n = max(1, ray_index((tmin / p.step) * (1.f - 1.f / 65536.f)) - 3);
  bool done = !(pixel && near) || n > n_hi;
  bool prev = false;   // sample n - 1 is valid
  int nstar = 0;       // 0: none
  float rgd0 = 0.f, rgd1 = 0.f, rgd2 = 0.f;
  int cur_brick = -1;
  bool cur_dead = false;
  if (VARIANT == 0) rgd0 = gd0 != 0.f ? 1.f / gd0 : 0.f, rgd1 = gd1 != 0.f ? 1.f / gd1 : 0.f, rgd2 = gd2 != 0.f ? 1.f / gd2 : 0.f;
  while (__ballot(!done)) {
    if (done) continue;
    RaySample s = ray_sample(n, q, p);
    if (!s.inside) {
      prev = false;
    } else if (VARIANT == 0) {
      const int b0 = s.ix >> 3, b1 = s.iy >> 3, b2 = s.iz >> 3;
      const int bid = (b2 * p.by + b1) * p.bx + b0;
      if (bid != cur_brick) {
        cur_brick = bid;
        cur_dead = brick[bid] == 0;
      }
      if (cur_dead) {
        const float zx = fminf(fminf(ray_exit(go0, gd0, rgd0, (float)(b0 * 8), (float)min(b0 * 8 + 8, p.cx)),
                                     ray_exit(go1, gd1, rgd1, (float)(b1 * 8), (float)min(b1 * 8 + 8, p.cy))),
                               ray_exit(go2, gd2, rgd2, (float)(b2 * 8), (float)min(b2 * 8 + 8, p.cz)));
        const int m = min(ray_index(zx / p.step) - 1, n_hi);   // rounded down, less a guard of a sample
        if (m > n) {
          const RaySample sm = ray_sample(m, q, p);
          if (sm.inside && (sm.ix >> 3) == b0 && (sm.iy >> 3) == b1 && (sm.iz >> 3) == b2) {
            n = m;
            s = sm;
          }
        }
      }
      const unsigned st = state[((size_t)s.iz * p.cy + s.iy) * p.cx + s.ix];
      if (st == 2) {
        float c[8];
        ray_corners(tsdf, s, p, c);
        if (ray_trilinear(c, s) < 0.f) {
          nstar = n;
          done = true;
        } else {
          prev = true;
        }
      } else {
        prev = st != 0;
      }
    } else {
      if (ray_weights_ok(weight, s, p)) {
        float c[8];
        ray_corners(tsdf, s, p, c);
        if (ray_trilinear(c, s) < 0.f) {
          nstar = n;
          done = true;
        } else {
          prev = true;
        }
      } else {
        prev = false;
      }
    }
    if (!done) {
      ++n;
      done = n > n_hi;
    }
  }
  if (!pixel) return;
  float od = 0.f, on0 = 0.f, on1 = 0.f, on2 = 0.f, ov = 0.f;
  if (nstar >= 2 && prev) {   // both samples lie inside: they were found valid above
    const RaySample sa = ray_sample(nstar - 1, q, p), sb = ray_sample(nstar, q, p);
    float c[8];
    ray_corners(tsdf, sa, p, c);
    const float s0 = ray_trilinear(c, sa);
    ray_corners(tsdf, sb, p, c);
    const float s1 = ray_trilinear(c, sb);
    if (s0 >= 0.f) {
      const float zs = (float)(nstar - 1) * p.step + p.step * (s0 / (s0 - s1));
      od = p.cam.fb / zs;
      // the gradient of the trilinear interpolant at sample n*, in lattice units (the voxel cancels in the normalisation)
      float g[3];
      ray_gradient(c, sb, g);
      const float g0 = g[0], g1 = g[1], g2 = g[2];
      const float len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
      if (track_pos_finite(len)) on0 = g0 / len, on1 = g1 / len, on2 = g2 / len;
      ray_corners(vvalue, sb, p, c);
      ov = ray_trilinear(c, sb);
    }
  }
  const size_t px = (size_t)v * p.w + u;
  disp_o[(size_t)f * p.hw + px] = od;
  normal_o[((size_t)f * 3 + 0) * p.hw + px] = on0;
  normal_o[((size_t)f * 3 + 1) * p.hw + px] = on1;
  normal_o[((size_t)f * 3 + 2) * p.hw + px] = on2;
  value_o[(size_t)f * p.hw + px] = ov;
}

struct RayPlan {
  long cells, nblocks;
  int bx, by, bz;
  long off_state, off_brick, bytes;   // byte offsets inside the workspace
};

// false: unsupported extents
static bool ray_plan(int nx, int ny, int nz, RayPlan* pl) {
  if (!tsdf_grid_ok(nx, ny, nz)) return false;
  pl->cells = (long)(nx - 1) * (ny - 1) * (nz - 1);
  pl->nblocks = ((long)nx * ny * nz + RAY_BLOCK - 1) / RAY_BLOCK;
  pl->bx = (nx - 1 + RAY_BRICK - 1) / RAY_BRICK, pl->by = (ny - 1 + RAY_BRICK - 1) / RAY_BRICK, pl->bz = (nz - 1 + RAY_BRICK - 1) / RAY_BRICK;
  TrackCarver ws = {16, 0};
  pl->off_state = ws.take(pl->cells);
  pl->off_brick = ws.take((long)pl->bx * pl->by * pl->bz * 4);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_tsdf_raycast_workspace(int nx, int ny, int nz) {
  RayPlan pl;
  if (!ray_plan(nx, ny, nz, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_tsdf_raycast(const float* tsdf, const unsigned char* weight, const float* vvalue, const float* origin3_host, float voxel,
                                int min_weight, const float* R, const float* t, const float* K4_host, float baseline, float step, int variant,
                                float* disp, float* normal, float* value, int nv, int h, int w, int nx, int ny, int nz, void* workspace,
                                long workspace_bytes, void* stream) {
  if (!tsdf || !weight || !vvalue || !origin3_host || !R || !t || !K4_host || !disp || !normal || !value || !workspace) return DIS_ERR_NULL;
  RayPlan pl;
  if (nv < 1 || nv > RAY_MAX_VIEWS || !track_image_ok(h, w, 2) || !ray_plan(nx, ny, nz, &pl)) return DIS_ERR_BAD_SHAPE;
  RayParams p;
  if (!track_camera(K4_host, baseline, &p.cam) || !track_pos_finite(voxel) || !tsdf_origin(origin3_host, &p.ox, &p.oy, &p.oz) ||
      min_weight < 1 || min_weight > TRACK_MAX_TL)
    return DIS_ERR_UNSUPPORTED;
  if (!(step >= voxel / 8.f && step <= 8.f * voxel)) return DIS_ERR_UNSUPPORTED;
  // float(n) must stay exact: the samples a ray can have inside the lattice, from its diagonal, stay below 2^24 (the kernel takes no
  // sample beyond 2^24 - 1 either, however far away the camera is)
  const float diag = sqrtf(((float)nx * (float)nx + (float)ny * (float)ny) + (float)nz * (float)nz);
  if (!((diag * voxel) / step < 16777216.f)) return DIS_ERR_UNSUPPORTED;
  if (workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15) || (variant != 0 && variant != 1)) return DIS_ERR_UNSUPPORTED;
  p.nv = nv, p.h = h, p.w = w, p.hw = h * w, p.nx = nx, p.ny = ny, p.nz = nz, p.total = nx * ny * nz, p.min_weight = min_weight;
  p.cx = nx - 1, p.cy = ny - 1, p.cz = nz - 1, p.bx = pl.bx, p.by = pl.by, p.bz = pl.bz;
  p.voxel = voxel, p.step = step;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* state = (unsigned char*)workspace + pl.off_state;
  int* brick = (int*)((char*)workspace + pl.off_brick);
  const dim3 grid((unsigned)dis_cdiv(w, RAY_TILE), (unsigned)dis_cdiv(h, RAY_TILE), (unsigned)nv), block(RAY_BLOCK);
  if (variant == 0) {
    hipLaunchKernelGGL(raycast_state_kernel, dim3((unsigned)pl.nblocks), block, 0, st, tsdf, weight, state, p);
    DIS_CHECK_LAUNCH();
    hipLaunchKernelGGL(raycast_brick_kernel, dim3((unsigned)(pl.bx * pl.by * pl.bz)), block, 0, st, (const unsigned char*)state, brick, p);
    DIS_CHECK_LAUNCH();
    hipLaunchKernelGGL(raycast_march_kernel<0>, grid, block, 0, st, tsdf, weight, vvalue, (const unsigned char*)state, (const int*)brick, R, t,
                       disp, normal, value, p);
  } else {
    hipLaunchKernelGGL(raycast_march_kernel<1>, grid, block, 0, st, tsdf, weight, vvalue, (const unsigned char*)state, (const int*)brick, R, t,
                       disp, normal, value, p);
  }
  DIS_CHECK_LAUNCH();
  return 0;
}
