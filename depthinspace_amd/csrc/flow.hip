// Dense optical flow between the frames of a track (include/dis_hip.h, section "dense optical flow"): coarse-to-fine Horn-Schunck with
// warping, fp32, every operation a fixed per-pixel stencil in the operand order of tests/flow_ref.py.  No atomics and no sum whose
// order depends on the launch: two calls give the same bits.  All ordered pairs of all tracks ride in the grid of every launch.
//
//   flow_stats_kernel      one workgroup per frame: population mean and standard deviation, fp64, fixed order.
//   flow_normalise_kernel  level 0 of the pyramid.
//   flow_down_kernel       [1 4 6 4 1] / 16 over x, then over y, at the even positions; one lane per output pixel.
//   flow_upsample_kernel   u = 2 bilinear(u_coarse, x / 2, y / 2) when a finer level is entered (zeros at the coarsest).
//   flow_warp_kernel       32 x 8 tile: m = (a + bw) / 2 with a 1-pixel halo through LDS -> Ix, Iy, It.
//   flow_jacobi_kernel     the hot path.  A workgroup holds a 64 x 48 region of (u, v) in LDS, twice (Jacobi reads the old field while
//                          it writes the new one), and the coefficients Ix, Iy, It, den, u0, v0 of its 12 pixels per lane in registers.
//                          It runs up to FLOW_T = 8 steps and writes the 48 x 32 interior: a pixel FLOW_T away from the region's edge
//                          has seen nothing but exact values after FLOW_T steps, so the result equals the global iteration.  The image
//                          border replicates by clamping the neighbour's GLOBAL coordinate; where the region's edge lies on or beyond
//                          the image's, that side stays exact.  Rows that can no longer reach the interior are skipped.
//   flow_jacobi_step_kernel  one step per launch from global memory: the variant scripts/flow_rate.py measures the above against.
//   flow_store_kernel      (pairs, 2, h, w) -> flow (n, tl tl, 2, h, w) with the zero diagonal.
#include "track_common.h"

#define FLOW_T 8
#define FLOW_RW 64
#define FLOW_RH 48
#define FLOW_IW (FLOW_RW - 2 * FLOW_T)
#define FLOW_IH (FLOW_RH - 2 * FLOW_T)
#define FLOW_PPT (FLOW_RH / 4)
#define FLOW_MAX_LEVELS 12   // 8192 / 2^11 = 4 = the smallest min_size
#define FLOW_WT_W 32
#define FLOW_WT_H 8

__global__ __launch_bounds__(1024) void flow_stats_kernel(const float* __restrict__ frames, float* __restrict__ stats, int hw) {
  __shared__ double sm[16];
  __shared__ double bc;
  const float* p = frames + (size_t)blockIdx.x * hw;
  double s = 0.0;
  for (int i = threadIdx.x; i < hw; i += 1024) s += (double)p[i];
  const double tot = block_sum_d(s, sm);
  if (threadIdx.x == 0) bc = tot / (double)hw;
  __syncthreads();
  const double mean = bc;
  double q = 0.0;
  for (int i = threadIdx.x; i < hw; i += 1024) {
    const double d = (double)p[i] - mean;
    q += d * d;
  }
  const double tq = block_sum_d(q, sm);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = (float)mean;
    stats[2 * blockIdx.x + 1] = fmaxf((float)sqrt(tq / (double)hw), 1e-6f);
  }
}

__global__ __launch_bounds__(256) void flow_normalise_kernel(const float* __restrict__ frames, const float* __restrict__ stats,
                                                             float* __restrict__ out, int hw, int blocks_per_frame) {
  const int f = blockIdx.x / blocks_per_frame;
  const int i = (blockIdx.x % blocks_per_frame) * 256 + threadIdx.x;
  if (i >= hw) return;
  const size_t o = (size_t)f * hw + i;
  out[o] = (frames[o] - stats[2 * f]) / stats[2 * f + 1];
}

__device__ __forceinline__ float flow_binomial(float a, float b, float c, float d, float e) {
  const float s = (a + e) + 4.f * (b + d);
  return (s + 6.f * c) * 0.0625f;
}

__global__ __launch_bounds__(256) void flow_down_kernel(const float* __restrict__ in, float* __restrict__ out, long total, int h, int w,
                                                        int hc, int wc) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % wc), y = (int)((idx / wc) % hc);
  const long f = idx / ((long)wc * hc);
  const float* p = in + (size_t)f * h * w;
  int xs[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) xs[d] = min(max(2 * x + d - 2, 0), w - 1);
  float r[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    const float* row = p + (size_t)min(max(2 * y + d - 2, 0), h - 1) * w;
    r[d] = flow_binomial(row[xs[0]], row[xs[1]], row[xs[2]], row[xs[3]], row[xs[4]]);
  }
  out[idx] = flow_binomial(r[0], r[1], r[2], r[3], r[4]);
}

// img at (x, y) clamped into the image: (I00 (1 - fx) + I01 fx) (1 - fy) + (I10 (1 - fx) + I11 fx) fy.  fmaxf / fminf drop a NaN
// operand, so every index lies inside the image whatever the flow holds.
struct FlowTap {
  int i00, i01, i10, i11;
  float fx, fy, gx, gy;
};
__device__ __forceinline__ FlowTap flow_tap(float x, float y, int h, int w) {
  x = fminf(fmaxf(x, 0.f), (float)(w - 1));
  y = fminf(fmaxf(y, 0.f), (float)(h - 1));
  const float xf = floorf(x), yf = floorf(y);
  const int x0 = (int)xf, y0 = (int)yf;
  const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  FlowTap t;
  t.i00 = y0 * w + x0;
  t.i01 = y0 * w + x1;
  t.i10 = y1 * w + x0;
  t.i11 = y1 * w + x1;
  t.fx = x - xf;
  t.fy = y - yf;
  t.gx = 1.f - t.fx;
  t.gy = 1.f - t.fy;
  return t;
}
__device__ __forceinline__ float flow_sample(const float* __restrict__ img, const FlowTap& t) {
  const float top = img[t.i00] * t.gx + img[t.i01] * t.fx;
  const float bot = img[t.i10] * t.gx + img[t.i11] * t.fx;
  return top * t.gy + bot * t.fy;
}

// uv (pairs, 2, h, w) from the coarser (pairs, 2, hc, wc); coarse == NULL: zeros
__global__ __launch_bounds__(256) void flow_upsample_kernel(const float* __restrict__ coarse, float* __restrict__ uv, long total, int h, int w,
                                                            int hc, int wc) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // over pairs * h * w
  if (idx >= total) return;
  const int hw = h * w;
  const long p = idx / hw;
  const int pix = (int)(idx % hw);
  float u = 0.f, v = 0.f;
  if (coarse) {
    const FlowTap t = flow_tap((float)(pix % w) * 0.5f, (float)(pix / w) * 0.5f, hc, wc);
    const float* c = coarse + (size_t)p * 2 * hc * wc;
    u = 2.f * flow_sample(c, t);
    v = 2.f * flow_sample(c + (size_t)hc * wc, t);
  }
  uv[(size_t)p * 2 * hw + pix] = u;
  uv[(size_t)p * 2 * hw + hw + pix] = v;
}

// pair p of a track -> its frames: q = i (tl - 1) + (j - (j > i))
__device__ __forceinline__ void flow_pair(long p, int tl, long* fa, long* fb) {
  const int pt = tl * (tl - 1);
  const long track = p / pt;
  const int q = (int)(p % pt);
  const int i = q / (tl - 1), jj = q % (tl - 1);
  const int j = jj + (jj >= i ? 1 : 0);
  *fa = track * tl + i;
  *fb = track * tl + j;
}

// pyr: this level of the pyramid (frames, h, w); uv (pairs, 2, h, w); coef (pairs, 3, h, w) = Ix, Iy, It; dbg (4, pairs, h, w) or NULL
__global__ __launch_bounds__(256) void flow_warp_kernel(const float* __restrict__ pyr, const float* __restrict__ uv, float* __restrict__ coef,
                                                        float* __restrict__ dbg, long pairs, int tl, int h, int w, int tiles_x, int tiles_y) {
  __shared__ float m[FLOW_WT_H + 2][FLOW_WT_W + 2];
  __shared__ float bws[FLOW_WT_H + 2][FLOW_WT_W + 2];
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const long p = blockIdx.x / (tiles_x * tiles_y);
  const int hw = h * w;
  long fa, fb;
  flow_pair(p, tl, &fa, &fb);
  const float* a = pyr + (size_t)fa * hw;
  const float* b = pyr + (size_t)fb * hw;
  const float* u = uv + (size_t)p * 2 * hw;
  const float* v = u + hw;
  for (int i = threadIdx.x; i < (FLOW_WT_H + 2) * (FLOW_WT_W + 2); i += 256) {
    const int r = i / (FLOW_WT_W + 2), c = i % (FLOW_WT_W + 2);
    const int y = min(max(ty * FLOW_WT_H + r - 1, 0), h - 1), x = min(max(tx * FLOW_WT_W + c - 1, 0), w - 1);
    const int pix = y * w + x;
    const FlowTap t = flow_tap((float)x + u[pix], (float)y + v[pix], h, w);
    const float bw = flow_sample(b, t);
    bws[r][c] = bw;
    m[r][c] = (a[pix] + bw) * 0.5f;
  }
  __syncthreads();
  const int lx = threadIdx.x % FLOW_WT_W, ly = threadIdx.x / FLOW_WT_W;
  const int x = tx * FLOW_WT_W + lx, y = ty * FLOW_WT_H + ly;
  if (x >= w || y >= h) return;
  const int pix = y * w + x;
  const float ix = (m[ly + 1][lx + 2] - m[ly + 1][lx]) * 0.5f;
  const float iy = (m[ly + 2][lx + 1] - m[ly][lx + 1]) * 0.5f;
  const float bw = bws[ly + 1][lx + 1];
  const float it = bw - a[pix];
  float* c = coef + (size_t)p * 3 * hw + pix;
  c[0] = ix;
  c[hw] = iy;
  c[2 * (size_t)hw] = it;
  if (dbg) {
    const size_t plane = (size_t)pairs * hw;
    float* d = dbg + (size_t)p * hw + pix;
    d[0] = bw;
    d[plane] = ix;
    d[2 * plane] = iy;
    d[3 * plane] = it;
  }
}

#define FLOW_C6 ((float)(1.0 / 6.0))
#define FLOW_C12 ((float)(1.0 / 12.0))

// one Jacobi step at a pixel from its 8 neighbours:  ub = ((l + r) + (t + b)) / 6 + ((tl + tr) + (bl + br)) / 12 (v alike),
// r = ((Ix (ub - u0) + Iy (vb - v0)) + It) / den,  u = ub - Ix r,  v = vb - Iy r
__device__ __forceinline__ float2 flow_step(float2 l, float2 r, float2 t, float2 b, float2 tl, float2 tr, float2 bl, float2 br, float ix,
                                            float iy, float it, float den, float u0, float v0) {
  const float ub = ((l.x + r.x) + (t.x + b.x)) * FLOW_C6 + ((tl.x + tr.x) + (bl.x + br.x)) * FLOW_C12;
  const float vb = ((l.y + r.y) + (t.y + b.y)) * FLOW_C6 + ((tl.y + tr.y) + (bl.y + br.y)) * FLOW_C12;
  const float q = ((ix * (ub - u0) + iy * (vb - v0)) + it) / den;
  return make_float2(ub - ix * q, vb - iy * q);
}

// uv0: the flow at the warp (u0, v0); uv_in -> uv_out: `steps` (1 .. FLOW_T) Jacobi steps.  All (pairs, 2, h, w); uv_out is neither input.
__global__ __launch_bounds__(256) void flow_jacobi_kernel(const float* __restrict__ uv0, const float* __restrict__ uv_in,
                                                          float* __restrict__ uv_out, const float* __restrict__ coef, int h, int w,
                                                          int tiles_x, int tiles_y, float alpha2, int steps) {
  __shared__ float2 s[2][FLOW_RH][FLOW_RW];
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const size_t p = blockIdx.x / (tiles_x * tiles_y);
  const int hw = h * w;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gx0 = tx * FLOW_IW - FLOW_T, gy0 = ty * FLOW_IH - FLOW_T;
  const int gx = gx0 + lane;
  const bool in_x = gx >= 0 && gx < w;
  const int cx = min(max(gx, 0), w - 1);
  // LDS columns of the x neighbours: the global coordinate clamped into the image, then into the region (a column lost to the
  // region's edge only feeds pixels that are not written)
  const int xm = min(max(min(max(gx - 1, 0), w - 1) - gx0, 0), FLOW_RW - 1);
  const int xp = min(max(min(max(gx + 1, 0), w - 1) - gx0, 0), FLOW_RW - 1);
  const float* u_in = uv_in + p * 2 * hw;
  const float* u_0 = uv0 + p * 2 * hw;
  const float* cf = coef + p * 3 * hw;
  float ix[FLOW_PPT], iy[FLOW_PPT], it[FLOW_PPT], den[FLOW_PPT], u0[FLOW_PPT], v0[FLOW_PPT];
#pragma unroll
  for (int k = 0; k < FLOW_PPT; ++k) {
    const int ly = k * 4 + wv;
    const int pix = min(max(gy0 + ly, 0), h - 1) * w + cx;
    s[0][ly][lane] = make_float2(u_in[pix], u_in[hw + pix]);
    ix[k] = cf[pix];
    iy[k] = cf[hw + pix];
    it[k] = cf[2 * (size_t)hw + pix];
    den[k] = (alpha2 + ix[k] * ix[k]) + iy[k] * iy[k];
    u0[k] = u_0[pix];
    v0[k] = u_0[hw + pix];
  }
  __syncthreads();
  const int ry0 = max(0, -gy0), ry1 = min(FLOW_RH, h - gy0);
  const bool top_open = gy0 > 0, bot_open = gy0 + FLOW_RH < h;
  for (int st = 1; st <= steps; ++st) {
    const float2(*cur)[FLOW_RW] = s[(st - 1) & 1];
    float2(*nxt)[FLOW_RW] = s[st & 1];
    // rows that are still exact after this step (and inside the image)
    const int lo = top_open ? st : ry0, hi = bot_open ? FLOW_RH - st : ry1;
#pragma unroll
    for (int k = 0; k < FLOW_PPT; ++k) {
      const int ly = k * 4 + wv;   // wave-uniform
      if (ly >= lo && ly < hi && in_x) {
        const int gy = gy0 + ly;
        const int ym = min(max(max(gy - 1, 0) - gy0, 0), FLOW_RH - 1);
        const int yp = min(max(min(gy + 1, h - 1) - gy0, 0), FLOW_RH - 1);
        nxt[ly][lane] = flow_step(cur[ly][xm], cur[ly][xp], cur[ym][lane], cur[yp][lane], cur[ym][xm], cur[ym][xp], cur[yp][xm],
                                  cur[yp][xp], ix[k], iy[k], it[k], den[k], u0[k], v0[k]);
      }
    }
    __syncthreads();
  }
  if (lane < FLOW_T || lane >= FLOW_RW - FLOW_T || !in_x) return;
  const float2(*fin)[FLOW_RW] = s[steps & 1];
  float* u_out = uv_out + p * 2 * hw;
#pragma unroll
  for (int k = 0; k < FLOW_PPT; ++k) {
    const int ly = k * 4 + wv, gy = gy0 + ly;
    if (ly >= FLOW_T && ly < FLOW_RH - FLOW_T && gy < h) {
      const float2 r = fin[ly][lane];
      u_out[gy * w + gx] = r.x;
      u_out[hw + gy * w + gx] = r.y;
    }
  }
}

// the same step, one per launch, every operand from global memory
__global__ __launch_bounds__(256) void flow_jacobi_step_kernel(const float* __restrict__ uv0, const float* __restrict__ uv_in,
                                                               float* __restrict__ uv_out, const float* __restrict__ coef, long total, int h,
                                                               int w, float alpha2) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // over pairs * h * w
  if (idx >= total) return;
  const int hw = h * w;
  const size_t p = idx / hw;
  const int pix = (int)(idx % hw);
  const int x = pix % w, y = pix / w;
  const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0) * w, yp = min(y + 1, h - 1) * w, yc = y * w;
  const float* u = uv_in + p * 2 * hw;
  const float* v = u + hw;
  const float* cf = coef + p * 3 * hw;
#define FLOW_AT(o) make_float2(u[o], v[o])
  const float ix = cf[pix], iy = cf[hw + pix], it = cf[2 * (size_t)hw + pix];
  const float den = (alpha2 + ix * ix) + iy * iy;
  const float2 r = flow_step(FLOW_AT(yc + xm), FLOW_AT(yc + xp), FLOW_AT(ym + x), FLOW_AT(yp + x), FLOW_AT(ym + xm), FLOW_AT(ym + xp),
                             FLOW_AT(yp + xm), FLOW_AT(yp + xp), ix, iy, it, den, uv0[p * 2 * hw + pix], uv0[p * 2 * hw + hw + pix]);
#undef FLOW_AT
  uv_out[p * 2 * hw + pix] = r.x;
  uv_out[p * 2 * hw + hw + pix] = r.y;
}

__global__ __launch_bounds__(256) void flow_store_kernel(const float* __restrict__ uv, float* __restrict__ flow, long total, int tl, int hw) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // over n * tl * tl * 2 * h * w
  if (idx >= total) return;
  const int pix = (int)(idx % hw);
  const long plane = idx / hw;
  const int c = (int)(plane & 1);
  const int e = (int)((plane >> 1) % (tl * tl));
  const long track = (plane >> 1) / (tl * tl);
  const int i = e / tl, j = e % tl;
  float r = 0.f;
  if (i != j) {
    const long p = track * tl * (tl - 1) + i * (tl - 1) + j - (j > i ? 1 : 0);
    r = uv[((size_t)p * 2 + c) * hw + pix];
  }
  flow[idx] = r;
}

__global__ __launch_bounds__(256) void flow_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < total) dst[idx] = src[idx];
}

struct FlowPlan {
  int levels;
  int h[FLOW_MAX_LEVELS], w[FLOW_MAX_LEVELS];
  long pyr_off[FLOW_MAX_LEVELS + 1];   // floats, level k of the pyramid; [levels]: its size
  long lev_off[FLOW_MAX_LEVELS + 1];   // floats, level k of the per-level flows
  long frames, pairs;
  long stats, pyr, uv[3], coef, total;   // float offsets inside the workspace
};

static bool flow_extents_ok(int n, int tl, int h, int w) {
  return n > 0 && tl >= 2 && tl <= TRACK_MAX_TL && track_image_ok(h, w, 8) && (long)n * tl * tl * 2 * h * w <= 0x7fffffffL;
}

// false: unsupported extents
static bool flow_plan(int n, int tl, int h, int w, int min_size, FlowPlan* pl) {
  if (!flow_extents_ok(n, tl, h, w) || min_size < 4) return false;
  pl->frames = (long)n * tl;
  pl->pairs = (long)n * tl * (tl - 1);
  int k = 0;
  pl->h[0] = h;
  pl->w[0] = w;
  pl->pyr_off[0] = pl->lev_off[0] = 0;
  for (;;) {
    const long hw = (long)pl->h[k] * pl->w[k];
    pl->pyr_off[k + 1] = pl->pyr_off[k] + pl->frames * hw;
    pl->lev_off[k + 1] = pl->lev_off[k] + pl->pairs * 2 * hw;
    if ((pl->h[k] < pl->w[k] ? pl->h[k] : pl->w[k]) < 2 * min_size || k + 1 >= FLOW_MAX_LEVELS) break;
    pl->h[k + 1] = (pl->h[k] + 1) / 2;
    pl->w[k + 1] = (pl->w[k] + 1) / 2;
    ++k;
  }
  pl->levels = k + 1;
  const long hw = (long)h * w;
  TrackCarver ws = {4, 0};   // in floats: 16 bytes
  pl->stats = ws.take(2 * pl->frames);
  pl->pyr = ws.take(pl->pyr_off[pl->levels]);
  for (int b = 0; b < 3; ++b) pl->uv[b] = ws.take(pl->pairs * 2 * hw);
  pl->coef = ws.take(pl->pairs * 3 * hw);
  pl->total = ws.off;
  return true;
}

extern "C" long dis_flow_workspace(int n, int tl, int h, int w, int min_size) {
  FlowPlan pl;
  if (!flow_plan(n, tl, h, w, min_size, &pl)) return -1;
  return pl.total * 4;
}

extern "C" int dis_dense_flow(const float* frames, float* flow, const DisFlowDebug* dbg, int n, int tl, int h, int w, float alpha, int warps,
                              int iters, int min_size, void* workspace, void* stream) {
  if (!frames || !flow || !workspace) return DIS_ERR_NULL;
  if (!flow_extents_ok(n, tl, h, w)) return DIS_ERR_BAD_SHAPE;
  FlowPlan pl;
  if (!(alpha > 0.f) || !(alpha <= 3.0e38f) || warps < 1 || warps > 16 || iters < 1 || iters > 1024 || min_size < 4 ||
      ((uintptr_t)workspace & 15) || !flow_plan(n, tl, h, w, min_size, &pl))
    return DIS_ERR_UNSUPPORTED;
  float* dbg_pyr = dbg ? dbg->pyr : nullptr;
  float* dbg_warp = dbg ? dbg->warp : nullptr;
  float* dbg_levels = dbg ? dbg->levels : nullptr;
  const int variant = dbg ? dbg->variant : 0;
  if (variant < 0 || variant > 1 || (dbg_warp && (dbg->level < 0 || dbg->level >= pl.levels))) return DIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* stats = ws + pl.stats;
  float* pyr = dbg_pyr ? dbg_pyr : ws + pl.pyr;   // the output asked for serves as the working buffer itself
  float* uv[3] = {ws + pl.uv[0], ws + pl.uv[1], ws + pl.uv[2]};
  float* coef = ws + pl.coef;
  const float alpha2 = alpha * alpha;
  const int hw0 = h * w;

  hipLaunchKernelGGL(flow_stats_kernel, dim3((unsigned)pl.frames), dim3(1024), 0, st, frames, stats, hw0);
  DIS_CHECK_LAUNCH();
  const int bpf = dis_cdiv(hw0, 256);
  hipLaunchKernelGGL(flow_normalise_kernel, dim3((unsigned)(pl.frames * bpf)), dim3(256), 0, st, frames, stats, pyr, hw0, bpf);
  DIS_CHECK_LAUNCH();
  for (int k = 1; k < pl.levels; ++k) {
    const long total = pl.frames * pl.h[k] * pl.w[k];
    hipLaunchKernelGGL(flow_down_kernel, dim3(dis_cdiv(total, 256)), dim3(256), 0, st, pyr + pl.pyr_off[k - 1], pyr + pl.pyr_off[k], total,
                       pl.h[k - 1], pl.w[k - 1], pl.h[k], pl.w[k]);
    DIS_CHECK_LAUNCH();
  }
  int cur = 0;
  for (int k = pl.levels - 1; k >= 0; --k) {
    const int hk = pl.h[k], wk = pl.w[k];
    const long px = pl.pairs * hk * wk;
    {
      const bool first = k == pl.levels - 1;
      const int dst = first ? 0 : (cur + 1) % 3;
      hipLaunchKernelGGL(flow_upsample_kernel, dim3(dis_cdiv(px, 256)), dim3(256), 0, st, first ? (const float*)nullptr : uv[cur], uv[dst], px,
                         hk, wk, first ? 1 : pl.h[k + 1], first ? 1 : pl.w[k + 1]);
      DIS_CHECK_LAUNCH();
      cur = dst;
    }
    const int wtx = dis_cdiv(wk, FLOW_WT_W), wty = dis_cdiv(hk, FLOW_WT_H);
    const int jtx = dis_cdiv(wk, FLOW_IW), jty = dis_cdiv(hk, FLOW_IH);
    for (int s = 0; s < warps; ++s) {
      float* d = (dbg_warp && k == dbg->level && s == warps - 1) ? dbg_warp : nullptr;
      hipLaunchKernelGGL(flow_warp_kernel, dim3((unsigned)(pl.pairs * wtx * wty)), dim3(256), 0, st, pyr + pl.pyr_off[k], uv[cur], coef, d,
                         pl.pairs, tl, hk, wk, wtx, wty);
      DIS_CHECK_LAUNCH();
      // uv[cur] stays (u0, v0); the steps alternate between the other two buffers
      const int o[2] = {(cur + 1) % 3, (cur + 2) % 3};
      int in = cur, turn = 0;
      for (int done = 0; done < iters;) {
        const int steps = variant == 1 ? 1 : (iters - done < FLOW_T ? iters - done : FLOW_T);
        if (variant == 1)
          hipLaunchKernelGGL(flow_jacobi_step_kernel, dim3(dis_cdiv(px, 256)), dim3(256), 0, st, uv[cur], uv[in], uv[o[turn]], coef, px, hk, wk,
                             alpha2);
        else
          hipLaunchKernelGGL(flow_jacobi_kernel, dim3((unsigned)(pl.pairs * jtx * jty)), dim3(256), 0, st, uv[cur], uv[in], uv[o[turn]], coef,
                             hk, wk, jtx, jty, alpha2, steps);
        DIS_CHECK_LAUNCH();
        in = o[turn];
        turn ^= 1;
        done += steps;
      }
      cur = in;
    }
    if (dbg_levels) {
      hipLaunchKernelGGL(flow_copy_kernel, dim3(dis_cdiv(px * 2, 256)), dim3(256), 0, st, uv[cur], dbg_levels + pl.lev_off[k], px * 2);
      DIS_CHECK_LAUNCH();
    }
  }
  const long total = (long)n * tl * tl * 2 * hw0;
  hipLaunchKernelGGL(flow_store_kernel, dim3(dis_cdiv(total, 256)), dim3(256), 0, st, uv[cur], flow, total, tl, hw0);
  DIS_CHECK_LAUNCH();
  return 0;
}
