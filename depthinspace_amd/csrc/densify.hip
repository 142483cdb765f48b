// Densification of disparity maps (include/dis_hip.h, section "disparity densification"): a gated hole fill from the first valid pixel
// in each of 8 directions, then the lower median over the valid pixels of a (2 r + 1)^2 window.  Everything is selection and
// comparison (the gate is one fp32 subtraction), so the result equals the restatement tests/densify_ref.py bit for bit.  No atomics.
// At most two launches, both over the 64 x 16 tiles of speckle.hip, four waves per tile, each wave rows wid, wid + 4, ...:
//
//   densify_fill_kernel     stages the tile with a halo of max_gap cells in LDS - invalid and out-of-image cells as 0, so "valid" is
//                           "> 0" and a walk needs no bounds test.  A tile without a hole skips the halo.  A lane whose pixel is invalid
//                           walks the 8 directions together, one step of each per round, and keeps the first hit of each; the lanes
//                           of a wave sit in one row and take the same step, so every read is 64 consecutive words: no bank
//                           conflict in any direction, whatever the pitch.  The hits are sorted by a network on 8 registers.
//   densify_median_kernel   <R>: the tile with a halo of R cells in LDS, a sorting network on 9 or 25 registers with +inf for the missing
//                           entries, the element (k - 1) / 2 taken as the largest of the first (k - 1) / 2 + 1.  Reads the fill's map (the workspace) when both
//                           stages run, the input otherwise.
//
// With max_gap = 0 the fill kernel walks nothing and is the copy that writes invalid elements as +0.0.
#include <utility>

#include "track_common.h"

#define DNS_TW 64
#define DNS_TH 16
#define DNS_ROWS_PER_WAVE (DNS_TH / 4)
#define DNS_MAX_GAP 32
#define DNS_INF __builtin_huge_valf()

__device__ __forceinline__ float dns_clean(float d) { return track_valid(d) ? d : 0.f; }

// Batcher's merge exchange on N registers, ascending.  (Correct for every N, not only the
// powers of two: the comparators of the next power of two that would touch an index >= N are the ones left out, and those never move
// a +inf that pads the top.)
// The comparators are listed at compile time and expanded one call each with constant indices: the values stay in registers.
template <int N>
struct DnsNetwork {
  int lo[N * 8], hi[N * 8], count;
  constexpr DnsNetwork() : lo{}, hi{}, count(0) {
    for (int p = 1; p < N; p *= 2)
      for (int k = p; k >= 1; k /= 2)
        for (int j = k % p; j <= N - 1 - k; j += 2 * k)
          for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) lo[count] = i + j, hi[count] = i + j + k, ++count;
  }
};

template <int N, int C>
__host__ __device__ __forceinline__ void dns_exchange(float (&v)[N]) {
  constexpr DnsNetwork<N> net;
  constexpr int lo = net.lo[C], hi = net.hi[C];
  const float a = v[lo], b = v[hi];
  v[lo] = fminf(a, b);
  v[hi] = fmaxf(a, b);
}

template <int N, int... C>
__host__ __device__ __forceinline__ void dns_sort_seq(float (&v)[N], std::integer_sequence<int, C...>) {
  (dns_exchange<N, C>(v), ...);
}

template <int N>
__host__ __device__ __forceinline__ void dns_sort(float (&v)[N]) {
  dns_sort_seq<N>(v, std::make_integer_sequence<int, DnsNetwork<N>().count>{});
}

// v[pos] of the ascending v (every entry > 0), pos in 0 .. LAST, without indexing the registers by a variable: the largest of
// v[0 .. pos].  (A chain of pos == i ? v[i] : r is turned back into an indexed load of a copy in scratch memory by the compiler.)
template <int LAST, int N>
__host__ __device__ __forceinline__ float dns_pick(const float (&v)[N], int pos) {
  static_assert(LAST < N, "inside the array");
  float r = v[0];
#pragma unroll
  for (int i = 1; i <= LAST; ++i) r = fmaxf(r, i <= pos ? v[i] : 0.f);
  return r;
}

// the lower median of the valid (> 0) entries of w[0 .. N): +inf when there is none
template <int N>
__host__ __device__ __forceinline__ float dns_lower_median(float (&w)[N]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool ok = w[i] > 0.f;
    k += ok ? 1 : 0;
    w[i] = ok ? w[i] : DNS_INF;
  }
  dns_sort<N>(w);
  return dns_pick<(N - 1) / 2, N>(w, (k > 0 ? k - 1 : 0) / 2);
}

// tile (16 + 2 g) x pitch floats, pitch = 64 + 2 g; the pixel (ry, lane) of the tile is the cell (g + ry, g + lane)
__global__ __launch_bounds__(256) void densify_fill_kernel(const float* __restrict__ disp, float* __restrict__ out,
                                                           unsigned char* __restrict__ state, int h, int w, int tiles_x, int tiles_y,
                                                           int g, int min_dirs, float max_spread) {
  extern __shared__ float dns_tile[];
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const int f = blockIdx.x / (tiles_x * tiles_y);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int x = tx * DNS_TW + lane;
  const size_t base = (size_t)f * h * w;
  const int pitch = DNS_TW + 2 * g, rows = DNS_TH + 2 * g;

  float d[DNS_ROWS_PER_WAVE];
  bool hole = false;
#pragma unroll
  for (int k = 0; k < DNS_ROWS_PER_WAVE; ++k) {
    const int y = ty * DNS_TH + wid + 4 * k;
    const bool in = x < w && y < h;
    d[k] = in ? dns_clean(disp[base + (size_t)y * w + x]) : 0.f;
    hole = hole || (in && !(d[k] > 0.f));
  }
  if (g > 0 && __syncthreads_or(hole)) {   // (the same answer in every lane of the workgroup)
    // four rows of the wave per round, both halves of a row (pitch <= 128): 8 loads in flight, then the 8 stores.  (One row per
    // round left one load's latency after the other: 43 instead of 40 us per call of 4 frames of 512 x 432.)
    for (int ly0 = wid; ly0 < rows; ly0 += 16) {
      float v[4][2];
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int ly = ly0 + 4 * b, lx = lane + 64 * c;
          const int y = ty * DNS_TH - g + ly, xx = tx * DNS_TW - g + lx;
          const bool in = ly < rows && lx < pitch && y >= 0 && y < h && xx >= 0 && xx < w;
          v[b][c] = in ? disp[base + (size_t)y * w + xx] : 0.f;
        }
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int ly = ly0 + 4 * b, lx = lane + 64 * c;
          if (ly < rows && lx < pitch) dns_tile[ly * pitch + lx] = dns_clean(v[b][c]);
        }
    }
    __syncthreads();
    // E, W, S, N, SE, SW, NE, NW as steps through the tile
    const int step[8] = {1, -1, pitch, -pitch, pitch + 1, pitch - 1, -pitch + 1, -pitch - 1};
#pragma unroll
    for (int k = 0; k < DNS_ROWS_PER_WAVE; ++k) {
      const int y = ty * DNS_TH + wid + 4 * k;
      if (!(x < w && y < h) || d[k] > 0.f) continue;
      const int at = (g + wid + 4 * k) * pitch + g + lane;
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = 0.f;
      for (int s = 1; s <= g; ++s) {
        bool all = true;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float t = dns_tile[at + s * step[q]];   // the first hit stays
          v[q] = v[q] > 0.f ? v[q] : t;
          all = all && v[q] > 0.f;
        }
        if (all) break;
      }
      int m = 0;
      float hi = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        m += v[q] > 0.f ? 1 : 0;
        hi = fmaxf(hi, v[q]);
      }
      const float med = dns_lower_median<8>(v);   // v is ascending afterwards, +inf for the directions without a hit
      if (m >= min_dirs && hi - v[0] <= max_spread) d[k] = -med;   // (negative: filled - told apart from the input's pixels below)
    }
  }
#pragma unroll
  for (int k = 0; k < DNS_ROWS_PER_WAVE; ++k) {
    const int y = ty * DNS_TH + wid + 4 * k;
    if (x < w && y < h) {
      const size_t i = base + (size_t)y * w + x;
      out[i] = fabsf(d[k]);
      if (state) state[i] = d[k] > 0.f ? 1 : (d[k] < 0.f ? 2 : 0);
    }
  }
}

// src: the input (state wanted or not) or the fill's map (state: NULL, the fill wrote it)
template <int R>
__global__ __launch_bounds__(256) void densify_median_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                             unsigned char* __restrict__ state, int h, int w, int tiles_x, int tiles_y) {
  constexpr int PITCH = DNS_TW + 2 * R, ROWS = DNS_TH + 2 * R;
  __shared__ float tile[ROWS * PITCH];
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const int f = blockIdx.x / (tiles_x * tiles_y);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int x = tx * DNS_TW + lane;
  const size_t base = (size_t)f * h * w;
  for (int ly = wid; ly < ROWS; ly += 4) {
    const int y = ty * DNS_TH - R + ly;
    for (int lx = lane; lx < PITCH; lx += 64) {
      const int xx = tx * DNS_TW - R + lx;
      const bool in = y >= 0 && y < h && xx >= 0 && xx < w;
      tile[ly * PITCH + lx] = in ? dns_clean(src[base + (size_t)y * w + xx]) : 0.f;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < DNS_ROWS_PER_WAVE; ++k) {
    const int ry = wid + 4 * k, y = ty * DNS_TH + ry;
    if (!(x < w && y < h)) continue;
    const float c = tile[(R + ry) * PITCH + R + lane];
    float r = 0.f;
    if (c > 0.f) {
      float win[(2 * R + 1) * (2 * R + 1)];
#pragma unroll
      for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) win[dy * (2 * R + 1) + dx] = tile[(ry + dy) * PITCH + lane + dx];
      r = dns_lower_median<(2 * R + 1) * (2 * R + 1)>(win);   // k >= 1: the pixel itself
    }
    const size_t i = base + (size_t)y * w + x;
    out[i] = r;
    if (state) state[i] = c > 0.f ? 1 : 0;
  }
}

static inline bool densify_extents_ok(int n, int h, int w) { return n > 0 && track_image_ok(h, w, 1) && (long)n * h * w <= 0x7fffffffL; }

static inline bool densify_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}

extern "C" long dis_disp_densify_workspace(int n, int h, int w) {
  if (!densify_extents_ok(n, h, w)) return -1;
  TrackCarver c{16, 0};
  c.take((long)n * h * w * 4);   // the fill's map, read by the median
  return c.off;
}

extern "C" int dis_disp_densify(const float* disp, float* out, unsigned char* state, int n, int h, int w, int max_gap, int min_dirs,
                                float max_spread, int median_r, void* workspace, void* stream) {
  if (!disp || !out || !workspace) return DIS_ERR_NULL;
  if (!densify_extents_ok(n, h, w)) return DIS_ERR_BAD_SHAPE;
  if (max_gap < 0 || max_gap > DNS_MAX_GAP || min_dirs < 1 || min_dirs > 8 || median_r < 0 || median_r > 2 ||
      !(max_spread >= 0.f && max_spread <= TRACK_FLT_MAX) || ((uintptr_t)workspace & 15))
    return DIS_ERR_UNSUPPORTED;
  const long total = (long)n * h * w;
  if (densify_overlap(out, total * 4, disp, total * 4) || (state && densify_overlap(state, total, disp, total * 4)) ||
      (state && densify_overlap(state, total, out, total * 4)))
    return DIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = dis_cdiv(w, DNS_TW), tiles_y = dis_cdiv(h, DNS_TH);
  const dim3 grid((unsigned)((long)n * tiles_x * tiles_y));
  const bool fill = max_gap > 0 || median_r == 0;   // (neither stage: the fill kernel with no walk is the copy)
  const float* src = disp;
  if (fill) {
    float* mid = median_r > 0 ? (float*)workspace : out;
    const size_t lds = max_gap > 0 ? (size_t)(DNS_TH + 2 * max_gap) * (DNS_TW + 2 * max_gap) * sizeof(float) : 0;
    hipLaunchKernelGGL(densify_fill_kernel, grid, dim3(256), lds, st, disp, mid, state, h, w, tiles_x, tiles_y, max_gap, min_dirs,
                       max_spread);
    DIS_CHECK_LAUNCH();
    src = mid;
    state = nullptr;
  }
  if (median_r == 1) {
    hipLaunchKernelGGL(densify_median_kernel<1>, grid, dim3(256), 0, st, src, out, state, h, w, tiles_x, tiles_y);
    DIS_CHECK_LAUNCH();
  } else if (median_r == 2) {
    hipLaunchKernelGGL(densify_median_kernel<2>, grid, dim3(256), 0, st, src, out, state, h, w, tiles_x, tiles_y);
    DIS_CHECK_LAUNCH();
  }
  return 0;
}
