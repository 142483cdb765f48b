// A track's per-frame disparity maps fused into one point cloud (include/dis_hip.h, section "track fusion"): fp32, every operation a
// fixed per-pixel expression in the operand order of tests/fuse_ref.py.  Three launches; order and hand-off between them are held by
// the launch boundaries alone - no atomics, no flags polled between workgroups - so nothing depends on where workgroups are placed
// and two calls give the same bits.
//
//   fuse_check_kernel    one lane per pixel, 256-pixel blocks that never straddle a frame (ceil(h w / 256) blocks per frame), so the
//                        track and the frame are uniform over a block and R, t come through the scalar cache.  Loads its own disparity
//                        (coalesced) and the four neighbours of the normal, does tl - 1 four-tap gathers from the other frames
//                        (all taps are asked for before any is used), writes the dense maps views, seen, keep (uint8), resid, point
//                        and normal (planar) and the block's kept count: a 64-bit ballot per wave, __popcll, four partial counts
//                        through LDS.
//   fuse_scan_kernel     one workgroup of 1024 lanes loops over the block counts, 1024 at a time: exclusive offsets, the total, and
//                        the per-track counts (a track's tl ceil(h w / 256) blocks are contiguous).
//   fuse_scatter_kernel  the same grid as the check: a kept pixel writes its record at block offset + rank inside the block (ballot of
//                        `keep`, popcount of the lower lanes, the waves before it through LDS); records at or beyond `cap` are dropped.
#include "track_common.h"

#define FUSE_BLOCK TRACK_BLOCK
#define FUSE_MAX_TL TRACK_MAX_TL

struct FuseParams {
  int n, tl, h, w, hw, bpf;              // bpf = blocks per frame
  TrackCamera cam;
  float tol;
  int min_views, cap;
};

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_check_kernel(const float* __restrict__ disp, const float* __restrict__ R,
                                                                const float* __restrict__ t, unsigned char* __restrict__ views_o,
                                                                unsigned char* __restrict__ seen_o, unsigned char* __restrict__ keep_o,
                                                                float* __restrict__ resid_o, float* __restrict__ point_o,
                                                                float* __restrict__ normal_o, int* __restrict__ block_count,
                                                                const FuseParams p) {
  const int frame = blockIdx.x / p.bpf;                                // b tl + i: uniform over the block
  const int pix = (blockIdx.x % p.bpf) * FUSE_BLOCK + threadIdx.x;     // inside the frame: (v, u)
  const int i = frame % p.tl;
  const int frame0 = frame - i;                                        // the track's first frame
  bool keep = false;
  if (pix < p.hw) {
    const int v = pix / p.w, u = pix % p.w;
    const int idx = frame * p.hw + pix;             // < 2^31: checked on the host
    const float* di = disp + frame * p.hw;
    const float d = di[pix];
    // the four neighbours of the normal, asked for up front (the pixel's own address where there is none) so that their latency
    // and that of the gathers below overlap (profiles/fuse_rate.md)
    const bool interior = u > 0 && u < p.w - 1 && v > 0 && v < p.h - 1;
    const float dl = di[interior ? pix - 1 : pix], dr = di[interior ? pix + 1 : pix];
    const float du = di[interior ? pix - p.w : pix], dd = di[interior ? pix + p.w : pix];
    const bool valid = track_valid(d);
    int views = 0, seen = 0;
    float resid = 0.f, pt[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
    if (valid) {
      const float* Ri = R + frame * 9;
      const float* ti = t + frame * 3;
      float P[3], Xw[3];
      track_backproject(d, u, v, p.cam, P);
      track_to_world(Ri, ti, P, Xw);
      // first every projection and its four taps (slot s is frame j = s + (s >= i): ascending j), then the arithmetic
      float Xj[FUSE_MAX_TL - 1][3], uj[FUSE_MAX_TL - 1], vj[FUSE_MAX_TL - 1], tap[FUSE_MAX_TL - 1][4];
      int x0[FUSE_MAX_TL - 1], y0[FUSE_MAX_TL - 1];
      bool ok[FUSE_MAX_TL - 1];
#pragma unroll
      for (int s = 0; s < FUSE_MAX_TL - 1; ++s) {
        ok[s] = false;
        if (s < p.tl - 1) {
          const int j = s + (s >= i ? 1 : 0);
          float Y[3];   // (handing the helper the row Xj[s] itself costs four registers and reorders the blocks)
          track_to_camera(R + (frame0 + j) * 9, t + (frame0 + j) * 3, Xw, Y);
#pragma unroll
          for (int k = 0; k < 3; ++k) Xj[s][k] = Y[k];
          // this projection is fuse's own: pose has fx * (X0 * (1 / X2)) + cx, tsdf fx * (x / zs) + cx, rounded
          uj[s] = (p.cam.fx * Xj[s][0]) / Xj[s][2] + p.cam.cx;
          vj[s] = (p.cam.fy * Xj[s][1]) / Xj[s][2] + p.cam.cy;
          // (every comparison is false for NaN)
          ok[s] = Xj[s][2] > 0.f && uj[s] >= 0.f && uj[s] <= (float)(p.w - 1) && vj[s] >= 0.f && vj[s] <= (float)(p.h - 1);
          // 0 <= x0 <= w - 2, 0 <= y0 <= h - 2; a pixel that frame j does not see reads the cell at the origin and drops it
          x0[s] = ok[s] ? min((int)floorf(uj[s]), p.w - 2) : 0;
          y0[s] = ok[s] ? min((int)floorf(vj[s]), p.h - 2) : 0;
          const float* dj = disp + (frame0 + j) * p.hw + y0[s] * p.w + x0[s];
          tap[s][0] = dj[0], tap[s][1] = dj[1], tap[s][2] = dj[p.w], tap[s][3] = dj[p.w + 1];
        }
      }
      float acc[3] = {Xw[0], Xw[1], Xw[2]};
      float rsum = 0.f;
      bool lower = false;
      views = 1;
#pragma unroll
      for (int s = 0; s < FUSE_MAX_TL - 1; ++s) {
        if (!ok[s]) continue;
        const int j = s + (s >= i ? 1 : 0);
        const float d00 = tap[s][0], d01 = tap[s][1], d10 = tap[s][2], d11 = tap[s][3];
        if (!(track_valid(d00) && track_valid(d01) && track_valid(d10) && track_valid(d11))) continue;
        const float ax = uj[s] - (float)x0[s], ay = vj[s] - (float)y0[s];
        const float gx = 1.f - ax, gy = 1.f - ay;
        const float z00 = p.cam.fb / d00, z01 = p.cam.fb / d01, z10 = p.cam.fb / d10, z11 = p.cam.fb / d11;
        const float zs = (z00 * gx + z01 * ax) * gy + (z10 * gx + z11 * ax) * ay;
        const float rel = fabsf(zs - Xj[s][2]) / Xj[s][2];
        ++seen;
        rsum = rsum + rel;
        if (rel <= p.tol) {
          ++views;
          lower = lower || j < i;
          const float sc = zs / Xj[s][2];
          const float S[3] = {Xj[s][0] * sc, Xj[s][1] * sc, Xj[s][2] * sc};
          float Sw[3];
          track_to_world(R + (frame0 + j) * 9, t + (frame0 + j) * 3, S, Sw);
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] = acc[k] + Sw[k];
        }
      }
      if (seen > 0) resid = rsum / (float)seen;
#pragma unroll
      for (int k = 0; k < 3; ++k) pt[k] = acc[k] / (float)views;
      keep = views >= p.min_views && !lower;
      if (interior) {
        if (track_valid(dl) && track_valid(dr) && track_valid(du) && track_valid(dd)) {
          float Pl[3], Pr[3], Pu[3], Pd[3];
          track_backproject(dl, u - 1, v, p.cam, Pl);
          track_backproject(dr, u + 1, v, p.cam, Pr);
          track_backproject(du, u, v - 1, p.cam, Pu);
          track_backproject(dd, u, v + 1, p.cam, Pd);
          const float a[3] = {Pr[0] - Pl[0], Pr[1] - Pl[1], Pr[2] - Pl[2]};
          const float c[3] = {Pd[0] - Pu[0], Pd[1] - Pu[1], Pd[2] - Pu[2]};
          float m[3] = {a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]};
          const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
          if (track_pos_finite(len)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = m[k] / len;
            const float dot = (m[0] * P[0] + m[1] * P[1]) + m[2] * P[2];
            if (dot > 0.f) {
#pragma unroll
              for (int k = 0; k < 3; ++k) m[k] = -m[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) nrm[k] = (Ri[k] * m[0] + Ri[3 + k] * m[1]) + Ri[6 + k] * m[2];
          }
        }
      }
    }
    views_o[idx] = (unsigned char)views;
    seen_o[idx] = (unsigned char)seen;
    keep_o[idx] = keep ? 1 : 0;
    resid_o[idx] = resid;
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // planar (n, tl, 3, h, w); 3 n tl h w may pass 2^31
      const size_t o = ((size_t)frame * 3 + k) * p.hw + pix;
      point_o[o] = pt[k];
      normal_o[o] = nrm[k];
    }
  }
  track_block_count(__popcll(__ballot(keep)), block_count);
}

// exclusive scan of block_count[0 .. nblocks) -> block_off[0 .. nblocks], block_off[nblocks] the total; count[b] of every track
__global__ __launch_bounds__(TRACK_SCAN) void fuse_scan_kernel(const int* __restrict__ block_count, int* block_off, int* __restrict__ count,
                                                              int nblocks, int n, int bpt) {
  track_scan(block_count, block_off, nblocks);
  __threadfence();
  __syncthreads();     // the offsets written above by other lanes of this workgroup are read below
  for (int b = threadIdx.x; b < n; b += TRACK_SCAN) count[b] = block_off[(b + 1) * bpt] - block_off[b * bpt];
}

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_scatter_kernel(const unsigned char* __restrict__ keep_i, const float* __restrict__ point_i,
                                                                  const float* __restrict__ normal_i, const float* __restrict__ value_i,
                                                                  const int* __restrict__ block_off, float* __restrict__ xyz,
                                                                  float* __restrict__ normal, float* __restrict__ value,
                                                                  int* __restrict__ src, const FuseParams p) {
  __shared__ int wave_count[FUSE_BLOCK / DIS_WAVE];
  const int frame = blockIdx.x / p.bpf;
  const int pix = (blockIdx.x % p.bpf) * FUSE_BLOCK + threadIdx.x;
  const int idx = frame * p.hw + pix;
  const bool keep = pix < p.hw && keep_i[idx] != 0;
  const unsigned long long mask = __ballot(keep);
  track_wave_counts(__popcll(mask), wave_count);
  if (!keep) return;
  const int rank = track_rank(block_off, wave_count, __popcll(mask & track_lanes_below()));
  if (rank >= p.cap) return;
  const size_t o = (size_t)frame * 3 * p.hw + pix;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xyz[(size_t)rank * 3 + k] = point_i[o + (size_t)k * p.hw];
    normal[(size_t)rank * 3 + k] = normal_i[o + (size_t)k * p.hw];
  }
  value[rank] = value_i ? value_i[idx] : 0.f;
  src[rank] = idx;
}

struct FusePlan {
  long pixels, nblocks;
  int bpf, bpt;   // blocks per frame, per track
  long off_count, off_off, off_point, off_normal, bytes;   // byte offsets inside the workspace
};

// false: unsupported extents
static bool fuse_plan(int n, int tl, int h, int w, FusePlan* pl) {
  if (n < 1 || tl < 2 || tl > TRACK_MAX_TL || !track_image_ok(h, w, 2)) return false;
  pl->pixels = (long)n * tl * h * w;
  if (pl->pixels > 0x7fffffffL) return false;
  pl->bpf = dis_cdiv((long)h * w, FUSE_BLOCK);
  pl->bpt = tl * pl->bpf;
  pl->nblocks = (long)n * pl->bpt;
  TrackCarver ws = {16, 0};
  pl->off_count = ws.take(pl->nblocks * 4);
  pl->off_off = ws.take((pl->nblocks + 1) * 4);
  pl->off_point = ws.take(pl->pixels * 12);
  pl->off_normal = ws.take(pl->pixels * 12);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_fuse_workspace(int n, int tl, int h, int w) {
  FusePlan pl;
  if (!fuse_plan(n, tl, h, w, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_fuse_track(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, const float* value,
                              float tol, int min_views, int cap, const DisFuseOut* out, int n, int tl, int h, int w, void* workspace,
                              long workspace_bytes, void* stream) {
  if (!disp || !R || !t || !K4_host || !out || !workspace) return DIS_ERR_NULL;
  if (!out->count || !out->views || !out->seen || !out->keep || !out->resid) return DIS_ERR_NULL;
  if (cap > 0 && (!out->xyz || !out->normal || !out->value || !out->src)) return DIS_ERR_NULL;
  FusePlan pl;
  if (!fuse_plan(n, tl, h, w, &pl)) return DIS_ERR_BAD_SHAPE;
  FuseParams p;
  if (!(tol > 0.f && tol < 1.f) || min_views < 1 || min_views > tl || !track_camera(K4_host, baseline, &p.cam) || cap < 0 ||
      workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15))
    return DIS_ERR_UNSUPPORTED;
  p.n = n, p.tl = tl, p.h = h, p.w = w, p.hw = h * w, p.bpf = pl.bpf;
  p.tol = tol, p.min_views = min_views, p.cap = cap;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* block_count = (int*)(ws + pl.off_count);
  int* block_off = (int*)(ws + pl.off_off);
  float* point = out->point ? out->point : (float*)(ws + pl.off_point);
  float* dnormal = out->dnormal ? out->dnormal : (float*)(ws + pl.off_normal);
  const unsigned grid = (unsigned)pl.nblocks;
  hipLaunchKernelGGL(fuse_check_kernel, dim3(grid), dim3(FUSE_BLOCK), 0, st, disp, R, t, out->views, out->seen, out->keep, out->resid, point,
                     dnormal, block_count, p);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(TRACK_SCAN), 0, st, (const int*)block_count, block_off, out->count, (int)pl.nblocks, n,
                     pl.bpt);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(fuse_scatter_kernel, dim3(grid), dim3(FUSE_BLOCK), 0, st, (const unsigned char*)out->keep, (const float*)point,
                     (const float*)dnormal, value, (const int*)block_off, out->xyz, out->normal, out->value, out->src, p);
  DIS_CHECK_LAUNCH();
  return 0;
}
