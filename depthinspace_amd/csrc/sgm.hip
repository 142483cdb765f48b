// Semi-global matching of IR frames against the projector pattern (include/dis_hip.h, section "semi-global matching"):
// 9 x 7 census -> Hamming cost -> 8 path aggregations -> winner with uniqueness / left-right checks and a parabola fit.
// Integer arithmetic from the image comparison to the winning candidate: no float atomics, no host synchronisation, the result does
// not depend on any order.
//
//   sgm_census_kernel   one lane per pixel, 64 x 4 tile with its (4, 3) halo through LDS, 8-byte stores.
//   sgm_path_kernel     one wave per image line of a direction, lane l holds the D / 64 candidates d = l * VPL + j.  The chain over
//                       the line's pixels is sequential; per step: the cost from the two census words (never stored), the minimum of
//                       the previous L over d (DPP row operations, as f2_wave_max), the d +- 1 neighbours across lanes, S += L.
//                       One launch per direction: within a direction every pixel belongs to exactly one line, so S is read and
//                       written without atomics; the first direction stores instead of adding, so S needs no clearing.
//   sgm_winner_kernel   one wave per pixel (16 consecutive pixels per wave): argmin, second minimum, the right-view argmin read along
//                       the diagonal of S, validity, parabola; writes every element of disp.
#include "track_common.h"

typedef unsigned long long sgm_u64;
typedef unsigned short sgm_u16;

#define SGM_TILE_W 64
#define SGM_TILE_H 4
#define SGM_HALO_X 4
#define SGM_HALO_Y 3
#define SGM_LDS_W (SGM_TILE_W + 2 * SGM_HALO_X)
#define SGM_LDS_H (SGM_TILE_H + 2 * SGM_HALO_Y)

// frames 0 .. n - 1 come from im, frame n is the pattern
__global__ __launch_bounds__(256) void sgm_census_kernel(const float* __restrict__ im, const float* __restrict__ pattern,
                                                         sgm_u64* __restrict__ census, int n, int h, int w, int tiles_x, int tiles_y) {
  __shared__ float t[SGM_LDS_H][SGM_LDS_W];
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const int f = blockIdx.x / (tiles_x * tiles_y);
  const size_t hw = (size_t)h * w;
  const float* src = f < n ? im + (size_t)f * hw : pattern;
  for (int i = threadIdx.x; i < SGM_LDS_H * SGM_LDS_W; i += 256) {
    const int r = i / SGM_LDS_W, c = i % SGM_LDS_W;
    const int yy = min(max(ty * SGM_TILE_H + r - SGM_HALO_Y, 0), h - 1);
    const int xx = min(max(tx * SGM_TILE_W + c - SGM_HALO_X, 0), w - 1);
    t[r][c] = src[(size_t)yy * w + xx];
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = tx * SGM_TILE_W + lx, y = ty * SGM_TILE_H + ly;
  const float ctr = t[ly + SGM_HALO_Y][lx + SGM_HALO_X];
  sgm_u64 bits = 0;
  int k = 0;
#pragma unroll
  for (int dy = -SGM_HALO_Y; dy <= SGM_HALO_Y; ++dy)
#pragma unroll
    for (int dx = -SGM_HALO_X; dx <= SGM_HALO_X; ++dx) {
      if (dy == 0 && dx == 0) continue;
      bits |= (sgm_u64)(t[ly + SGM_HALO_Y + dy][lx + SGM_HALO_X + dx] < ctr ? 1 : 0) << k;   // NaN compares false
      ++k;
    }
  if (x < w && y < h) census[(size_t)f * hw + (size_t)y * w + x] = bits;
}

// maximum of a non-negative int over the wave, valid in every lane (the DPP sequence of f2_wave_max, conv_args.h)
__device__ __forceinline__ int sgm_wave_max(int v) {
#define SGM_DPP(ctrl, rmask) v = max(v, __builtin_amdgcn_update_dpp(0, v, ctrl, rmask, 0xf, true))
  SGM_DPP(0xB1, 0xf);   // quad_perm [1,0,3,2]
  SGM_DPP(0x4E, 0xf);   // quad_perm [2,3,0,1]
  SGM_DPP(0x124, 0xf);  // row_ror:4
  SGM_DPP(0x128, 0xf);  // row_ror:8   -> every lane holds its row's maximum
  SGM_DPP(0x142, 0xa);  // row_bcast:15 into rows 1, 3
  SGM_DPP(0x143, 0xc);  // row_bcast:31 into rows 2, 3 -> lane 63 holds the wave's maximum
#undef SGM_DPP
  return __builtin_amdgcn_readlane(v, 63);
}
// minimum over the wave of a value in [0, top]
__device__ __forceinline__ int sgm_wave_min(int v, int top) { return top - sgm_wave_max(top - v); }

template <int VPL>
struct SgmVec;
template <>
struct SgmVec<1> { typedef sgm_u16 T; };
template <>
struct SgmVec<2> { typedef unsigned int T; };
template <>
struct SgmVec<4> { typedef uint2 T; };

template <int VPL>
__device__ __forceinline__ void sgm_load(const sgm_u16* p, int (&v)[VPL]) {
  typename SgmVec<VPL>::T raw = *reinterpret_cast<const typename SgmVec<VPL>::T*>(p);
  sgm_u16 e[VPL];
  __builtin_memcpy(e, &raw, sizeof raw);
#pragma unroll
  for (int j = 0; j < VPL; ++j) v[j] = e[j];
}
template <int VPL>
__device__ __forceinline__ void sgm_store(sgm_u16* p, const int (&v)[VPL]) {
  sgm_u16 e[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) e[j] = (sgm_u16)v[j];
  typename SgmVec<VPL>::T raw;
  __builtin_memcpy(&raw, e, sizeof raw);
  *reinterpret_cast<typename SgmVec<VPL>::T*>(p) = raw;
}

#define SGM_BIG 0x3fff   // an absent d +- 1 neighbour: never the minimum (L <= 191, P1 <= 126)
#define SGM_CHUNK 4      // steps whose loads are issued together, one chunk ahead of the chain

// One wave per line of direction (dx, dy); lines_per_frame = h, w or h + w - 1.  FIRST: S = L, else S += L.
template <int VPL, bool FIRST>
__global__ __launch_bounds__(256) void sgm_path_kernel(const sgm_u64* __restrict__ census, sgm_u16* __restrict__ S, int n, int h, int w,
                                                       int dx, int dy, int p1, int p2, int lines_per_frame) {
  constexpr int D = 64 * VPL;
  const int lane = threadIdx.x & 63;
  const long line = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform, in a scalar register
  if (line >= (long)n * lines_per_frame) return;                 // (no block-level barrier in this kernel)
  const int f = (int)(line / lines_per_frame), k = (int)(line % lines_per_frame);
  int x, y;
  if (dy == 0) {
    y = k;
    x = dx > 0 ? 0 : w - 1;
  } else if (dx == 0 || k < w) {
    x = k;
    y = dy > 0 ? 0 : h - 1;
  } else {
    const int j = k - w + 1;   // 1 .. h - 1: the side column below / above the corner
    y = dy > 0 ? j : h - 1 - j;
    x = dx > 0 ? 0 : w - 1;
  }
  // pixels on the line before it leaves the image
  int len = dy == 0 ? w : (dx == 0 ? h : 0x7fffffff);
  if (dx > 0) len = min(len, w - x);
  if (dx < 0) len = min(len, x + 1);
  if (dy > 0) len = min(len, h - y);
  if (dy < 0) len = min(len, y + 1);
  const size_t hw = (size_t)h * w;
  const sgm_u64* cI = census + (size_t)f * hw;
  const sgm_u64* cP = census + (size_t)n * hw;
  sgm_u16* Sf = S + (size_t)f * hw * D;
  const int d0 = lane * VPL;

  // the loads of chunk k + 1 are issued in front of the chain of chunk k: a step waits for the d-minimum and the two neighbours, not
  // for memory
  struct Chunk {
    sgm_u64 ci[SGM_CHUNK], cp[SGM_CHUNK][VPL];
    int sv[SGM_CHUNK][VPL];
  };
  auto fetch = [&](int s0, Chunk& c) {
#pragma unroll
    for (int u = 0; u < SGM_CHUNK; ++u) {
      const int s = min(s0 + u, len - 1);   // a step past the end re-reads the last pixel and is not used
      const int xs = x + s * dx, ys = y + s * dy;
      const size_t pix = (size_t)ys * w + xs;
      c.ci[u] = cI[pix];
#pragma unroll
      for (int j = 0; j < VPL; ++j) c.cp[u][j] = cP[(size_t)ys * w + max(xs - d0 - j, 0)];
      if (!FIRST) sgm_load<VPL>(Sf + pix * D + d0, c.sv[u]);
    }
  };
  int Lp[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) Lp[j] = 0;
  Chunk cur, nxt;
  fetch(0, cur);
  for (int s0 = 0; s0 < len; s0 += SGM_CHUNK) {
    fetch(s0 + SGM_CHUNK, nxt);
#pragma unroll
    for (int u = 0; u < SGM_CHUNK; ++u) {
      const int s = s0 + u;
      if (s >= len) break;   // wave-uniform
      const int xs = x + s * dx, ys = y + s * dy;
      int L[VPL];
      if (s == 0) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) L[j] = xs - d0 - j >= 0 ? __popcll(cur.ci[u] ^ cur.cp[u][j]) : 64;
      } else {
        int lm = Lp[0];
#pragma unroll
        for (int j = 1; j < VPL; ++j) lm = min(lm, Lp[j]);
        const int m = sgm_wave_min(lm, 255);
        const int up = __shfl_up(Lp[VPL - 1], 1, 64);   // L(d - 1) of this lane's first candidate
        const int dn = __shfl_down(Lp[0], 1, 64);       // L(d + 1) of its last one
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const int c = xs - d0 - j >= 0 ? __popcll(cur.ci[u] ^ cur.cp[u][j]) : 64;
          const int lo = j > 0 ? Lp[j - 1] : (lane > 0 ? up : SGM_BIG);
          const int hi = j < VPL - 1 ? Lp[j + 1] : (lane < 63 ? dn : SGM_BIG);
          L[j] = c + min(min(Lp[j], m + p2), min(lo, hi) + p1) - m;
        }
      }
      int out[VPL];
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        out[j] = FIRST ? L[j] : cur.sv[u][j] + L[j];
        Lp[j] = L[j];
      }
      sgm_store<VPL>(Sf + ((size_t)ys * w + xs) * D + d0, out);
    }
    cur = nxt;
  }
}

#define SGM_PIX_PER_WAVE 16
#define SGM_KEY_TOP 0x7fffff   // keys are S * 256 + d <= 1528 * 256 + 255

template <int VPL>
__global__ __launch_bounds__(256) void sgm_winner_kernel(const sgm_u16* __restrict__ S, float* __restrict__ disp, int* __restrict__ d_int,
                                                         long total, int h, int w, int uniq, int lr) {
  constexpr int D = 64 * VPL;
  const int lane = threadIdx.x & 63;
  const long first = ((long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * SGM_PIX_PER_WAVE;   // wave-uniform
  if (first >= total) return;
  const int cnt = (int)min((long)SGM_PIX_PER_WAVE, total - first);
  const int dl = lane * VPL;
  float my_disp = 0.f;
  int my_d = 0;
  for (int i = 0; i < cnt; ++i) {
    const long pix = first + i;
    const int x = (int)(pix % w);
    const sgm_u16* sp = S + (size_t)pix * D;
    int v[VPL];
    sgm_load<VPL>(sp + dl, v);
    int key = SGM_KEY_TOP;
#pragma unroll
    for (int j = 0; j < VPL; ++j) key = min(key, (v[j] << 8) | (dl + j));
    key = sgm_wave_min(key, SGM_KEY_TOP);   // lowest S, then lowest d
    const int dw = key & 255, sw = key >> 8;
    int s2 = 0xffff;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      if (abs(dl + j - dw) > 1) s2 = min(s2, v[j]);
    s2 = sgm_wave_min(s2, 0xffff);
    bool valid = dw >= 1 && dw <= D - 2 && (long long)s2 * (100 - uniq) > (long long)sw * 100 && x - dw >= 0;
    if (valid) {   // wave-uniform: the right view's argmin at (x - dw, v), along the diagonal of S
      const int xr = x - dw;
      int rkey = SGM_KEY_TOP;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int d = dl + j;
        if (xr + d < w) rkey = min(rkey, ((int)S[((size_t)pix - dw + d) * D + d] << 8) | d);
      }
      rkey = sgm_wave_min(rkey, SGM_KEY_TOP);
      valid = abs((rkey & 255) - dw) <= lr;
    }
    float out = 0.f;
    if (valid) {
      const float a = (float)sp[dw - 1], b = (float)sw, c = (float)sp[dw + 1];
      const float den = a + c - 2.f * b;
      out = den > 0.f ? (float)dw + (a - c) / (2.f * den) : (float)dw;
    }
    if (lane == i) {
      my_disp = out;
      my_d = dw;
    }
  }
  if (lane < cnt) {
    disp[first + lane] = my_disp;
    if (d_int) d_int[first + lane] = my_d;
  }
}

static inline bool sgm_extents_ok(int n, int h, int w) {
  return n > 0 && track_image_ok(h, w, 1) && ((long)n + 1) * h * w <= 0x7fffffffL;
}
static inline long sgm_census_bytes(int n, int h, int w) { return ((long)n + 1) * h * w * 8; }

extern "C" long dis_sgm_workspace(int n, int h, int w, int ndisp) {
  if (!sgm_extents_ok(n, h, w) || (ndisp != 64 && ndisp != 128 && ndisp != 256)) return -1;
  return sgm_census_bytes(n, h, w) + (long)n * h * w * ndisp * 2;
}

template <int VPL>
static int sgm_run(const sgm_u64* cen, sgm_u16* S, float* disp, int* d_int, int n, int h, int w, int p1, int p2, int uniq, int lr,
                   hipStream_t st) {
  static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
  for (int r = 0; r < 8; ++r) {
    const int dx = dirs[r][0], dy = dirs[r][1];
    const int lpf = dy == 0 ? h : (dx == 0 ? w : h + w - 1);
    const int grid = dis_cdiv((long)n * lpf, 4);
    if (r == 0)
      hipLaunchKernelGGL((sgm_path_kernel<VPL, true>), dim3(grid), dim3(256), 0, st, cen, S, n, h, w, dx, dy, p1, p2, lpf);
    else
      hipLaunchKernelGGL((sgm_path_kernel<VPL, false>), dim3(grid), dim3(256), 0, st, cen, S, n, h, w, dx, dy, p1, p2, lpf);
    DIS_CHECK_LAUNCH();
  }
  const long total = (long)n * h * w;
  hipLaunchKernelGGL((sgm_winner_kernel<VPL>), dim3(dis_cdiv(total, 4 * SGM_PIX_PER_WAVE)), dim3(256), 0, st, S, disp, d_int, total, h, w,
                     uniq, lr);
  DIS_CHECK_LAUNCH();
  return 0;
}

extern "C" int dis_sgm_disparity(const float* im, const float* pattern, float* disp, int* d_int, short* vol, long long* census, int n,
                                 int h, int w, int ndisp, int p1, int p2, int uniq, int lr, void* workspace, void* stream) {
  if (!im || !pattern || !disp || !workspace) return DIS_ERR_NULL;
  if (!sgm_extents_ok(n, h, w)) return DIS_ERR_BAD_SHAPE;
  if ((ndisp != 64 && ndisp != 128 && ndisp != 256) || !(0 < p1 && p1 < p2 && p2 <= 127) || uniq < 0 || uniq >= 100 || lr < 0 ||
      ((uintptr_t)workspace & 15) || ((uintptr_t)vol & 7) || ((uintptr_t)census & 7))   // (S is accessed 8 bytes per lane at D = 256)
    return DIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  // the outputs asked for serve as the working buffers themselves
  sgm_u64* cen = census ? (sgm_u64*)census : (sgm_u64*)workspace;
  sgm_u16* S = vol ? (sgm_u16*)vol : (sgm_u16*)((char*)workspace + sgm_census_bytes(n, h, w));
  const int tiles_x = dis_cdiv(w, SGM_TILE_W), tiles_y = dis_cdiv(h, SGM_TILE_H);
  hipLaunchKernelGGL(sgm_census_kernel, dim3((unsigned)((long)(n + 1) * tiles_x * tiles_y)), dim3(256), 0, st, im, pattern, cen, n, h, w,
                     tiles_x, tiles_y);
  DIS_CHECK_LAUNCH();
  if (ndisp == 64) return sgm_run<1>(cen, S, disp, d_int, n, h, w, p1, p2, uniq, lr, st);
  if (ndisp == 128) return sgm_run<2>(cen, S, disp, d_int, n, h, w, p1, p2, uniq, lr, st);
  return sgm_run<4>(cen, S, disp, d_int, n, h, w, p1, p2, uniq, lr, st);
}
