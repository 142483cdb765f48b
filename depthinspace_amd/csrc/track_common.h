// Parts the track tools share (render.hip, sgm.hip, flow.hip, fuse.hip, pose.hip, tsdf.hip, raycast.hip, tsdf_align.hip): the finite tests,
// the workspace carver, the pinhole camera, the rigid transforms, the scan / count / rank steps of a stream compaction, the trilinear
// sampler of a volume (raycast.hip, tsdf_align.hip) and the 30-sum reduction and 6 x 6 Gauss-Newton step of the pose tools (pose.hip,
// tsdf_align.hip).  Every helper is inlined, and a
// device helper holds an expression only where the tools spell it token for token alike: the build uses -ffp-contract=off and the
// restatements tests/*_ref.py fix the operand order.  The three projections into a frame are NOT shared, they differ:
//   fuse  (fx * X0) / X2 + cx        pose  fx * (X0 * (1 / X2)) + cx        tsdf  fx * (x / zs) + cx, rounded
// nor is the bilinear sample (fuse interpolates depths, pose disparities).
#pragma once
#include "common.h"

#define TRACK_FLT_MAX 3.4028234663852886e38f
#define TRACK_MAX_TL 4
#define TRACK_MAX_HW 8192
#define TRACK_BLOCK 256    // lanes of a workgroup that counts or ranks: four waves
#define TRACK_SCAN 1024    // lanes of the workgroup that scans

// (NaN: false)
__host__ __device__ __forceinline__ bool track_pos_finite(float v) { return v > 0.f && v <= TRACK_FLT_MAX; }
__host__ __device__ __forceinline__ bool track_finite(float v) { return v >= -TRACK_FLT_MAX && v <= TRACK_FLT_MAX; }
__host__ __device__ __forceinline__ bool track_valid(float d) { return track_pos_finite(d); }   // a disparity: finite and > 0

static inline bool track_image_ok(int h, int w, int lo) { return h >= lo && w >= lo && h <= TRACK_MAX_HW && w <= TRACK_MAX_HW; }

static inline long track_align_up(long v, long a) { return (v + a - 1) & ~(a - 1); }   // a: a power of two

// hands out the pieces of a workspace one after the other, each at a multiple of `align`; `off` ends as the size of the whole
struct TrackCarver {
  long align, off;
  long take(long size) {
    const long at = off;
    off = track_align_up(off + size, align);
    return at;
  }
};

struct TrackCamera {
  float fx, fy, cx, cy, fb;   // fb = fx * baseline
};

// false: not a camera (the entry points answer DIS_ERR_UNSUPPORTED)
static inline bool track_camera(const float* K4_host, float baseline, TrackCamera* c) {
  c->fx = K4_host[0], c->fy = K4_host[1], c->cx = K4_host[2], c->cy = K4_host[3];
  c->fb = c->fx * baseline;
  return track_pos_finite(c->fx) && track_pos_finite(c->fy) && track_pos_finite(baseline) && track_finite(c->cx) && track_finite(c->cy) &&
         track_pos_finite(c->fb);
}

// the lattice of a volume (tsdf.hip, raycast.hip): every extent in 2 .. 1024
static inline bool tsdf_grid_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && nx <= 1024 && ny <= 1024 && nz <= 1024;
}
// false: not a lattice origin
static inline bool tsdf_origin(const float* origin3_host, float* ox, float* oy, float* oz) {
  *ox = origin3_host[0], *oy = origin3_host[1], *oz = origin3_host[2];
  return track_finite(*ox) && track_finite(*oy) && track_finite(*oz);
}

// pixel (u, v) with disparity d -> its point in the camera's frame
__device__ __forceinline__ void track_backproject(float d, int u, int v, const TrackCamera& c, float* P) {
  const float z = c.fb / d;
  P[0] = z * (((float)u - c.cx) / c.fx);
  P[1] = z * (((float)v - c.cy) / c.fy);
  P[2] = z;
}

// R X + t, each component ((R[k][0] X0 + R[k][1] X1) + R[k][2] X2) + t[k]
__device__ __forceinline__ void track_to_camera(const float* __restrict__ R, const float* __restrict__ t, const float* X, float* Y) {
#pragma unroll
  for (int k = 0; k < 3; ++k) Y[k] = ((R[3 * k] * X[0] + R[3 * k + 1] * X[1]) + R[3 * k + 2] * X[2]) + t[k];
}

// R^T (a - t), each component (R[0][k] q0 + R[1][k] q1) + R[2][k] q2
__device__ __forceinline__ void track_to_world(const float* __restrict__ R, const float* __restrict__ t, const float* a, float* X) {
  const float q0 = a[0] - t[0], q1 = a[1] - t[1], q2 = a[2] - t[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = (R[k] * q0 + R[3 + k] * q1) + R[6 + k] * q2;
}

// One workgroup of TRACK_SCAN lanes: the exclusive scan of counts[0 .. nblocks) -> offs[0 .. nblocks], offs[nblocks] the total, which
// is also returned (in every lane).  A wave __shfl_up scan, the wave sums through LDS, a carry from one round of 1024 to the next.
__device__ __forceinline__ int track_scan(const int* __restrict__ counts, int* offs, int nblocks) {
  __shared__ int wave_sum_s[TRACK_SCAN / DIS_WAVE];
  const int lane = threadIdx.x & (DIS_WAVE - 1), wid = threadIdx.x / DIS_WAVE;
  int carry = 0;
  for (int base = 0; base < nblocks; base += TRACK_SCAN) {
    const int k = base + threadIdx.x;
    const int c = k < nblocks ? counts[k] : 0;
    int x = c;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < DIS_WAVE; o <<= 1) {
      const int y = __shfl_up(x, o, DIS_WAVE);
      if (lane >= o) x += y;
    }
    if (lane == DIS_WAVE - 1) wave_sum_s[wid] = x;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < TRACK_SCAN / DIS_WAVE; ++q) {
      const int s = wave_sum_s[q];
      if (q < wid) before += s;
      total += s;
    }
    if (k < nblocks) offs[k] = carry + before + (x - c);
    carry += total;
    __syncthreads();   // wave_sum_s is rewritten by the next round
  }
  if (threadIdx.x == 0) offs[nblocks] = carry;
  return carry;
}

// The two halves of a compaction over workgroups of TRACK_BLOCK lanes.  wave_cnt: the flagged items of the lane's wave (__popcll of a
// __ballot, or a sum of them); wave_count: TRACK_BLOCK / DIS_WAVE ints of LDS.

// every lane of the workgroup calls (a barrier is passed): wave_count[] holds the counts of the four waves afterwards
__device__ __forceinline__ void track_wave_counts(int wave_cnt, int* wave_count) {
  if ((threadIdx.x & (DIS_WAVE - 1)) == 0) wave_count[threadIdx.x / DIS_WAVE] = wave_cnt;
  __syncthreads();
}

// -> block_count[blockIdx.x]: the flagged items of the workgroup; every lane calls
__device__ __forceinline__ void track_block_count(int wave_cnt, int* __restrict__ block_count) {
  __shared__ int wave_count[TRACK_BLOCK / DIS_WAVE];
  track_wave_counts(wave_cnt, wave_count);
  if (threadIdx.x == 0) block_count[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

__device__ __forceinline__ unsigned long long track_lanes_below() { return (1ull << (threadIdx.x & (DIS_WAVE - 1))) - 1ull; }

// after track_wave_counts (the lanes without an item may have left) -> the rank of the lane's first item in the whole compaction: the
// workgroup's offset (the scan of the counts above) + `below`, the flagged items of the lower lanes of its wave, + the waves before it
__device__ __forceinline__ int track_rank(const int* __restrict__ block_off, const int* wave_count, int below) {
  int rank = block_off[blockIdx.x] + below;
  for (int q = 0; q < (int)(threadIdx.x / DIS_WAVE); ++q) rank += wave_count[q];
  return rank;
}

// ------------------------------------------------------------------------------------------------ the trilinear sampler of a volume
// (raycast.hip, tsdf_align.hip).  L: any struct with the lattice's nx, ny, nz and min_weight.
struct RaySample {
  bool inside;
  int ix, iy, iz;
  float fx, fy, fz;
};

// the cell of the lattice coordinates (gx, gy, gz); inside: 0 <= g_a < float(n_a - 1), as floats (false for NaN)
template <typename L>
__device__ __forceinline__ RaySample ray_cell(const float gx, const float gy, const float gz, const L& p) {
  RaySample s;
  s.inside = gx >= 0.f && gx < (float)(p.nx - 1) && gy >= 0.f && gy < (float)(p.ny - 1) && gz >= 0.f && gz < (float)(p.nz - 1);
  s.ix = s.inside ? (int)floorf(gx) : 0;
  s.iy = s.inside ? (int)floorf(gy) : 0;
  s.iz = s.inside ? (int)floorf(gz) : 0;
  s.fx = gx - (float)s.ix, s.fy = gy - (float)s.iy, s.fz = gz - (float)s.iz;
  return s;
}

// the eight corners of the sample's cell, corner c at the offsets (c & 1, c >> 1 & 1, c >> 2)
template <typename L>
__device__ __forceinline__ void ray_corners(const float* __restrict__ A, const RaySample& s, const L& p, float* c) {
  const size_t l = ((size_t)s.iz * p.ny + s.iy) * p.nx + s.ix;
  const int nxy = p.nx * p.ny;
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = A[l + (k & 1) + ((k >> 1) & 1) * p.nx + (k >> 2) * nxy];
}

// along x, then y, then z, each a + f (b - a)
__device__ __forceinline__ float ray_trilinear(const float* c, const RaySample& s) {
  const float c00 = c[0] + s.fx * (c[1] - c[0]), c10 = c[2] + s.fx * (c[3] - c[2]);
  const float c01 = c[4] + s.fx * (c[5] - c[4]), c11 = c[6] + s.fx * (c[7] - c[6]);
  const float c0 = c00 + s.fy * (c10 - c00), c1 = c01 + s.fy * (c11 - c01);
  return c0 + s.fz * (c1 - c0);
}

// the gradient of that interpolant in lattice units: d/dx from the four x-differences blended in y then z, and likewise for y and z
__device__ __forceinline__ void ray_gradient(const float* c, const RaySample& s, float* g) {
  const float dx00 = c[1] - c[0], dx10 = c[3] - c[2], dx01 = c[5] - c[4], dx11 = c[7] - c[6];
  const float c00 = c[0] + s.fx * dx00, c10 = c[2] + s.fx * dx10, c01 = c[4] + s.fx * dx01, c11 = c[6] + s.fx * dx11;
  const float gx0 = dx00 + s.fy * (dx10 - dx00), gx1 = dx01 + s.fy * (dx11 - dx01);
  const float dy0 = c10 - c00, dy1 = c11 - c01;
  const float c0 = c00 + s.fy * dy0, c1 = c01 + s.fy * dy1;
  g[0] = gx0 + s.fz * (gx1 - gx0), g[1] = dy0 + s.fz * (dy1 - dy0), g[2] = c1 - c0;
}

template <typename L>
__device__ __forceinline__ bool ray_weights_ok(const unsigned char* __restrict__ weight, const RaySample& s, const L& p) {
  const size_t l = ((size_t)s.iz * p.ny + s.iy) * p.nx + s.ix;
  const int nxy = p.nx * p.ny;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) ok = ok && (int)weight[l + (k & 1) + ((k >> 1) & 1) * p.nx + (k >> 2) * nxy] >= p.min_weight;
  return ok;
}

// ------------------------------------------------------------------------------------------------ the reduction and the step of the pose tools
// (pose.hip, tsdf_align.hip): per-pixel terms -> 30 fp64 sums per workgroup -> a record -> the sums of a pair or view -> a 6 x 6
// Cholesky step applied on the left: R <- dR R, t <- dR t + delta.
#define POSE_BLOCK 256
#define POSE_WAVES (POSE_BLOCK / DIS_WAVE)
#define POSE_SUMS 30     // H_pq (p <= q, row by row) 0 .. 20, g_p 21 .. 26, S_w 27, S_c 28, n 29
#define POSE_REC 32      // doubles per record of partial sums
#define POSE_STATE 16    // doubles per pair or view: R (9, row-major), t (3), failed (1), 3 unused
#define POSE_MAX_BPP 128
#define POSE_BATCH 32    // records in flight per lane of the solve launch

// workgroups per image: about four pixels per lane, until the cap
static inline int pose_bpp(int h, int w) {
  const int bpp = dis_cdiv((long)h * w, 4 * POSE_BLOCK);
  return bpp > POSE_MAX_BPP ? POSE_MAX_BPP : bpp;
}

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

// every lane of the workgroup calls (a barrier is passed): the sum of acc[0 .. N) over the wave, over the four waves through LDS ->
// rec[0 .. 32), zeros from N on
template <int N>
__device__ __forceinline__ void pose_block_record(const double* acc, double* __restrict__ rec) {
  static_assert(N <= POSE_REC, "a record holds 32 doubles");
  __shared__ double wave_part[POSE_WAVES][POSE_REC];
  const int lane = threadIdx.x & (DIS_WAVE - 1), wid = threadIdx.x / DIS_WAVE;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double s = wave_sum_d(acc[k]);           // valid in every lane
    if (lane == 0) wave_part[wid][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < POSE_REC) {
    double s = 0.0;
    if (threadIdx.x < N) s = (wave_part[0][threadIdx.x] + wave_part[1][threadIdx.x]) + (wave_part[2][threadIdx.x] + wave_part[3][threadIdx.x]);
    rec[threadIdx.x] = s;
  }
}

// one lane, one sum: the element rec[0] of bpp records in ascending workgroup order; the records are asked for POSE_BATCH at a time, so
// that the additions do not wait for one load each
__device__ __forceinline__ double pose_sum_records(const double* __restrict__ rec, const int bpp) {
  double s = 0.0;
  for (int k = 0; k < bpp; k += POSE_BATCH) {
    double v[POSE_BATCH];
#pragma unroll
    for (int m = 0; m < POSE_BATCH; ++m) v[m] = rec[(size_t)min(k + m, bpp - 1) * POSE_REC];
#pragma unroll
    for (int m = 0; m < POSE_BATCH; ++m)
      if (k + m < bpp) s += v[m];
  }
  return s;
}

// the twist d (rotation 0 .. 2, translation 3 .. 5) applied on the left: R <- dR R, t <- dR t + d[3 .. 6), dR = exp([d[0 .. 3)]x)
__device__ __forceinline__ void pose_apply_twist(const double* d, double* R, double* t) {
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

// one Gauss-Newton step from the 30 sums S on the state (R, t).  false: fewer than min_corr used pixels, or a pivot that is not > 0
// and finite - the state is left as it is
__device__ __forceinline__ bool pose_gn_step(const double* S, const int min_corr, const double damping, double* R, double* t) {
  bool failed = S[29] < (double)min_corr;
  double L[6][6], d[6];
  if (!failed) {
    // Cholesky of H + damping diag(H), column by column; a pivot that is not > 0 or not finite ends the pair
    // (a bad pivot lets the remaining columns run on: their values are not used)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double hcc = S[pose_hidx(c, c)];
      double s = hcc + damping * hcc;
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
    pose_apply_twist(d, R, t);
  }
  return !failed;
}
