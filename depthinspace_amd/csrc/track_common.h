// Parts the track tools share (render.hip, sgm.hip, flow.hip, fuse.hip, pose.hip, tsdf.hip, raycast.hip): the finite tests, the workspace carver,
// the pinhole camera, the rigid transforms and the scan / count / rank steps of a stream compaction.  Every helper is inlined, and a
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
