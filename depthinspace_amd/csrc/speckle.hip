// Speckle filter of disparity maps (include/dis_hip.h, section "speckle filter"): the 4-connected components of pixels whose
// disparities differ by at most max_diff, and the components of at most max_size pixels set to 0.  Labels and counts are integers; the
// only atomics are integer minima and integer adds whose final values do not depend on the order, so the result is the same on every
// run and equals the restatement tests/speckle_ref.py bit for bit.  Four launches, g = the linear index f h w + y w + x of a pixel:
//
//   speckle_tile_kernel     one workgroup per 64 x 16 tile, one wave per row at a time.  The horizontal runs of a row come from one
//                           __ballot (a run's first lane is its label), the vertical links are unions in LDS (atomicMin, the root is
//                           the lowest index).  Writes, for every pixel of the tile, parent[g] = g of the root of its piece inside the
//                           tile (-1: invalid) and count[g] = the pixels of the piece at its root, 0 elsewhere: nothing is cleared.
//   speckle_merge_kernel    one lane per pixel pair across a tile border: union by atomicMin on parent[].  Roots only ever get a lower
//                           parent, so the root of a component ends as its lowest g whatever the order.  Every access to parent[] in
//                           this launch is an agent-scope atomic (a CU's L1 and another XCD's L2 are not refreshed by other workgroups'
//                           stores); a stale read would still be an ancestor, the atomics decide.
//   speckle_flatten_kernel  one lane per pixel, plain loads: root[g] = the end of the parent chain; the root of a tile piece adds the
//                           piece's count to its component's root (one integer add per piece, not per pixel).
//   speckle_apply_kernel    out = disp where count[root] > max_size, else 0; the optional label and size planes.
#include "track_common.h"

#define SPK_TW 64
#define SPK_TH 16
#define SPK_ROWS_PER_WAVE (SPK_TH / 4)

__device__ __forceinline__ bool spk_linked(float a, float b, float max_diff) {
  return track_valid(a) && track_valid(b) && fabsf(a - b) <= max_diff;   // (NaN: false)
}

// the unions run on a word another lane may lower at any time: every read of it is an atomic load
template <int SCOPE>
__device__ __forceinline__ int spk_find(int* L, int x) {
  int p;
  while ((p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE)) != x) x = p;
  return x;
}

// joins the trees of a and b; the higher root gets the lower one as its parent.  When another lane lowered that root first, the
// value it wrote still has to be joined with ours: go on from it.
template <int SCOPE>
__device__ __forceinline__ void spk_union(int* L, int a, int b) {
  for (;;) {
    a = spk_find<SCOPE>(L, a);
    b = spk_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);   // a > b
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(256) void speckle_tile_kernel(const float* __restrict__ disp, int* __restrict__ parent, int* __restrict__ count,
                                                           int h, int w, int tiles_x, int tiles_y, float max_diff) {
  __shared__ float d_s[SPK_TH][SPK_TW];
  __shared__ int lab_s[SPK_TH * SPK_TW];
  __shared__ int cnt_s[SPK_TH * SPK_TW];
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const int f = blockIdx.x / (tiles_x * tiles_y);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int x = tx * SPK_TW + lane;
  const size_t base = (size_t)f * h * w;
  const unsigned long long below_incl = lane == 63 ? ~0ull : (2ull << lane) - 1ull;

  // rows wid, wid + 4, ...: the disparity into LDS (0 outside the image: invalid), the run's first lane as the label
  unsigned long long left_mask[SPK_ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
    const int ry = wid + 4 * k, y = ty * SPK_TH + ry;
    const float d = (x < w && y < h) ? disp[base + (size_t)y * w + x] : 0.f;
    d_s[ry][lane] = d;
    const float dl = __shfl_up(d, 1, 64);
    left_mask[k] = __ballot(lane > 0 && spk_linked(d, dl, max_diff));
    // the highest lane <= this one that is not linked to its left neighbour (lane 0 never is)
    const int start = 63 - __clzll(~left_mask[k] & below_incl);
    lab_s[ry * SPK_TW + lane] = track_valid(d) ? ry * SPK_TW + start : -1;
    cnt_s[ry * SPK_TW + lane] = 0;
  }
  __syncthreads();
  // vertical links.  A link whose left neighbour has the same link, with both rows' runs continuing, joins what that one joins: skipped.
#pragma unroll
  for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
    const int ry = wid + 4 * k;
    if (ry == 0) continue;
    const float d = d_s[ry][lane], du = d_s[ry - 1][lane];
    const bool up = spk_linked(d, du, max_diff);
    const unsigned long long up_mask = __ballot(up);
    bool need = up;
    if (up && lane > 0) {
      const bool left_same = (left_mask[k] >> lane & 1) && (up_mask >> (lane - 1) & 1) &&
                             spk_linked(du, d_s[ry - 1][lane - 1], max_diff);
      need = !left_same;
    }
    if (need) spk_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab_s, ry * SPK_TW + lane, (ry - 1) * SPK_TW + lane);
  }
  __syncthreads();
  // the root of every pixel; a run's first lane adds the run's length to the root's count
  int root[SPK_ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
    const int i = (wid + 4 * k) * SPK_TW + lane;
    root[k] = -1;
    if (lab_s[i] >= 0) {
      root[k] = spk_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab_s, i);
      if (!(left_mask[k] >> lane & 1)) {
        const unsigned long long above = lane == 63 ? 0ull : (~left_mask[k] >> (lane + 1)) << (lane + 1);   // the run starts after this one
        const int end = above ? __ffsll((long long)above) - 1 : 64;
        atomicAdd(&cnt_s[root[k]], end - lane);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
    const int ry = wid + 4 * k, y = ty * SPK_TH + ry;
    if (x < w && y < h) {
      const size_t g = base + (size_t)y * w + x;
      const int r = root[k];
      parent[g] = r < 0 ? -1 : (int)(base + (size_t)(ty * SPK_TH + r / SPK_TW) * w + tx * SPK_TW + r % SPK_TW);
      count[g] = cnt_s[ry * SPK_TW + lane];   // 0 except at a root
    }
  }
}

// The pixel pairs across tile borders of one image: first the (tiles_y - 1) w pairs across horizontal borders (x fastest), then the
// (tiles_x - 1) h pairs across vertical ones (y fastest).
__global__ __launch_bounds__(256) void speckle_merge_kernel(const float* __restrict__ disp, int* parent, int n, int h, int w, int tiles_x,
                                                            int tiles_y, float max_diff) {
  const long per_image = (long)(tiles_y - 1) * w + (long)(tiles_x - 1) * h;
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= per_image * n) return;
  const int f = (int)(item / per_image);
  long k = item % per_image;
  const size_t base = (size_t)f * h * w;
  const float* d = disp + base;
  int x, y, xo, yo;   // the pixel and its neighbour in the tile before
  if (k < (long)(tiles_y - 1) * w) {
    y = ((int)(k / w) + 1) * SPK_TH, x = (int)(k % w);
    yo = y - 1, xo = x;
    const float dp = d[(size_t)y * w + x], dq = d[(size_t)yo * w + x];
    if (!spk_linked(dp, dq, max_diff)) return;
    if (x > 0) {   // the pair to the left joins the same two components (through links inside the tiles or across a vertical border)
      const float dpl = d[(size_t)y * w + x - 1], dql = d[(size_t)yo * w + x - 1];
      if (spk_linked(dp, dpl, max_diff) && spk_linked(dq, dql, max_diff) && spk_linked(dpl, dql, max_diff)) return;
    }
  } else {
    k -= (long)(tiles_y - 1) * w;
    x = ((int)(k / h) + 1) * SPK_TW, y = (int)(k % h);
    xo = x - 1, yo = y;
    if (!spk_linked(d[(size_t)y * w + x], d[(size_t)y * w + xo], max_diff)) return;
  }
  spk_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)(base + (size_t)y * w + x), (int)(base + (size_t)yo * w + xo));
}

__global__ __launch_bounds__(256) void speckle_flatten_kernel(const int* __restrict__ parent, int* __restrict__ root, int* count, long total) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  int r = parent[g];
  if (r >= 0) {
    int p;
    while ((p = parent[r]) != r) r = p;
    const int c = count[g];   // > 0: the root of a tile piece; no other lane adds to it unless it is the component's root
    if (c > 0 && r != (int)g) atomicAdd(count + r, c);
  }
  root[g] = r;
}

__global__ __launch_bounds__(256) void speckle_apply_kernel(const float* __restrict__ disp, const int* __restrict__ root,
                                                            const int* __restrict__ count, float* __restrict__ out, int* __restrict__ label,
                                                            int* __restrict__ size, long total, int hw, int max_size) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int r = root[g];
  const int c = r >= 0 ? count[r] : 0;
  out[g] = c > max_size ? disp[g] : 0.f;
  if (label) label[g] = r >= 0 ? r - (int)(g / hw) * hw : -1;
  if (size) size[g] = c;
}

static inline bool speckle_extents_ok(int n, int h, int w) { return n > 0 && track_image_ok(h, w, 1) && (long)n * h * w <= 0x7fffffffL; }

extern "C" long dis_speckle_workspace(int n, int h, int w) {
  if (!speckle_extents_ok(n, h, w)) return -1;
  TrackCarver c{16, 0};
  for (int k = 0; k < 3; ++k) c.take((long)n * h * w * 4);   // parent, count, root
  return c.off;
}

extern "C" int dis_speckle_filter(const float* disp, float* out, int* label, int* size, int n, int h, int w, int max_size, float max_diff,
                                  void* workspace, void* stream) {
  if (!disp || !out || !workspace) return DIS_ERR_NULL;
  if (!speckle_extents_ok(n, h, w)) return DIS_ERR_BAD_SHAPE;
  if (max_size < 0 || !(max_diff >= 0.f && max_diff <= TRACK_FLT_MAX) || ((uintptr_t)workspace & 15)) return DIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)n * h * w;
  TrackCarver c{16, 0};
  int* parent = (int*)((char*)workspace + c.take(total * 4));
  int* count = (int*)((char*)workspace + c.take(total * 4));
  int* root = (int*)((char*)workspace + c.take(total * 4));
  const int tiles_x = dis_cdiv(w, SPK_TW), tiles_y = dis_cdiv(h, SPK_TH);
  hipLaunchKernelGGL(speckle_tile_kernel, dim3((unsigned)((long)n * tiles_x * tiles_y)), dim3(256), 0, st, disp, parent, count, h, w,
                     tiles_x, tiles_y, max_diff);
  DIS_CHECK_LAUNCH();
  const long pairs = ((long)(tiles_y - 1) * w + (long)(tiles_x - 1) * h) * n;
  if (pairs > 0) {
    hipLaunchKernelGGL(speckle_merge_kernel, dim3(dis_cdiv(pairs, 256)), dim3(256), 0, st, disp, parent, n, h, w, tiles_x, tiles_y,
                       max_diff);
    DIS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(speckle_flatten_kernel, dim3(dis_cdiv(total, 256)), dim3(256), 0, st, parent, root, count, total);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(speckle_apply_kernel, dim3(dis_cdiv(total, 256)), dim3(256), 0, st, disp, root, count, out, label, size, total, h * w,
                     max_size);
  DIS_CHECK_LAUNCH();
  return 0;
}
