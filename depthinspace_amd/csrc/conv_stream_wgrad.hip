// Weight gradient of the streaming convolutions (DispNetS), ONE family for both activation storages: fp32 (conv_gen.hip,
// dis_convg_wgrad) and bf16 (conv_bf16.hip, dis_convb_wgrad).  dW[tap][xc][gc] = sum_pixels X[pixel + tap][xc] * G[pixel][gc]; X and
// G are each fp32 or bf16 (template flags XB / GB), everything behind the load is fp32: exact products of the stored values, fp32
// accumulation, fp64 sums over the slabs in a fixed order (deterministic).
//
//   stream_wgrad_kernel<MTW, NTW, XB, GB>   one tap x TX x-channels x TG g-channels per workgroup, 32 pixels per step on
//       v_mfma_f32_16x16x4_f32, split-K over pixel ranges into slabs that stream_wgrad_reduce_kernel sums.
//   stream_head_wgrad_kernel<C8, XB, GB>    a disparity head (one gradient channel, 3x3): one pass over x, no matrix core.
//
// Dispatch, the same for every storage: slice pairs (conv2d.hip, dis_wgrad_pairs_*), then the head form, then the generic kernel.
// The head form needs cG <= 4 and the pairs cG >= 16, so their order decides nothing.  Routing follows the operand flags, not the
// entry point; three kinds of call, none of which ops.py issues (_head_stream_bwd always passes cG = 4 and pad = k / 2, disp_head_g
// picks the entry point by x.dtype, and the bf16 storage never holds two fp32 operands), are served differently than before the
// two families were merged:
//   - a bf16 call with cG_w == 1 but cG > 4 runs the generic kernel (the head form's slabs are only sized for cG <= 4);
//   - a dis_convb_wgrad call with an fp32 x of head shape takes the head form;
//   - a dis_convb_wgrad call with two fp32 operands takes the fp32 slice pairs where dis_convg_wgrad would.
#include "conv_args.h"
#include "conv_plan.h"
#include <stdlib.h>

struct StreamWgArgs {
  const void* X;
  const void* G;
  float* part;  // [ksplit][tap][cXp][cGp]
  int n, hX, wX, ldX, xoff, cX;
  int hG, wG, ldG, goff, cG;
  int S, pad, k;
  int nxb, ngb;
  int mper;  // G pixels per split (multiple of 32)
  int cXp, cGp;
};
template <bool BF>
__device__ __forceinline__ float4 cb_load4(const void* p, long e) {
  if (BF) {
    const uint2 v = *(const uint2*)((const bf16_t*)p + e);
    return make_float4(cb_lo(v.x), cb_hi(v.x), cb_lo(v.y), cb_hi(v.y));
  }
  return *(const float4*)((const float*)p + e);
}
template <int MTW, int NTW, bool XB, bool GB>
__global__ __launch_bounds__(256) void stream_wgrad_kernel(StreamWgArgs a) {
  constexpr int TX = 32 * MTW, TG = 32 * NTW, XS = TX + 16, GS = TG + 16;
  constexpr int X_FL = 32 * XS, G_FL = 32 * GS;
  constexpr int NLX = TX / 32, NLG = TG / 32;  // 4-channel loads per thread per step
  __shared__ __attribute__((aligned(16))) float smem[2 * (X_FL + G_FL)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int ntaps = a.k * a.k;
  const int tap = blockIdx.x % ntaps;
  const int rest = blockIdx.x / ntaps;
  const int xb = rest % a.nxb, gb = rest / a.nxb;
  const int ky = tap / a.k, kx = tap % a.k;
  const int M = a.n * a.hG * a.wG;
  const int m_lo = blockIdx.y * a.mper;
  const int m_hi = min(M, m_lo + a.mper);
  float4 rx[NLX], rg[NLG];
  auto prefetch = [&](int mbase) {
#pragma unroll
    for (int j = 0; j < NLX; ++j) {
      const int item = tid + j * 256;
      const int px = item / (TX / 4), q = item % (TX / 4);
      const int m = mbase + px;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int c = xb * TX + q * 4;
      if (m < m_hi && c < a.cX) {
        const int gx = m % a.wG, t = m / a.wG, gy = t % a.hG, nn = t / a.hG;
        const int iy = gy * a.S - a.pad + ky, ix = gx * a.S - a.pad + kx;
        if (iy >= 0 && iy < a.hX && ix >= 0 && ix < a.wX)
          v = cb_load4<XB>(a.X, (((long)nn * a.hX + iy) * a.wX + ix) * a.ldX + a.xoff + c);
      }
      rx[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int item = tid + j * 256;
      const int px = item / (TG / 4), q = item % (TG / 4);
      const int m = mbase + px;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int c = gb * TG + q * 4;
      if (m < m_hi && c < a.cG) v = cb_load4<GB>(a.G, (long)m * a.ldG + a.goff + c);
      rg[j] = v;
    }
  };
  auto stage = [&](int buf) {
    float* Xt = smem + buf * (X_FL + G_FL);
    float* Gt = Xt + X_FL;
#pragma unroll
    for (int j = 0; j < NLX; ++j) {
      const int item = tid + j * 256;
      *(float4*)(Xt + (item / (TX / 4)) * XS + (item % (TX / 4)) * 4) = rx[j];
    }
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int item = tid + j * 256;
      *(float4*)(Gt + (item / (TG / 4)) * GS + (item % (TG / 4)) * 4) = rg[j];
    }
  };
  f32x4 acc[MTW][NTW];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int wx = wave & 1, wg = wave >> 1;
  if (m_lo < m_hi) {
    prefetch(m_lo);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int mb = m_lo; mb < m_hi; mb += 32) {
      const bool more = mb + 32 < m_hi;
      if (more) prefetch(mb + 32);
      const float* Xt = smem + buf * (X_FL + G_FL);
      const float* Gt = Xt + X_FL;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        float av[MTW], bv[NTW];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) av[mt] = Xt[(kk * 4 + lg) * XS + wx * 16 * MTW + mt * 16 + li];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bv[nt] = Gt[(kk * 4 + lg) * GS + wg * 16 * NTW + nt * 16 + li];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
      }
      if (more) stage(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }
  float* out = a.part + ((long)blockIdx.y * ntaps + tap) * a.cXp * a.cGp;
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xc = xb * TX + wx * 16 * MTW + mt * 16 + lg * 4 + r;
        const int gc = gb * TG + wg * 16 * NTW + nt * 16 + li;
        out[(long)xc * a.cGp + gc] = acc[mt][nt][r];
      }
}
// grad_w[(g*cXw + x)*k*k + tap] = sum_split part[split][tap][x][g]
__global__ void stream_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, int nsplit, int ntaps,
                                           int cXp, int cGp, int cXw, int cGw) {
  const long total = (long)ntaps * cXw * cGw;
  const long slab = (long)ntaps * cXp * cGp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int g = (int)(i % cGw);
    long r = i / cGw;
    const int x = (int)(r % cXw);
    const int tap = (int)(r / cXw);
    const float* p = part + ((long)tap * cXp + x) * cGp + g;
    double s = 0.0;  // fp64 over the split-K slabs (sums of ~1e5 signed per-pixel terms at full resolution)
    for (int k = 0; k < nsplit; ++k) s += (double)p[k * slab];
    gw[((long)g * cXw + x) * ntaps + tap] = (float)s;
  }
}

// ---- weight gradient of a disparity head: ONE gradient channel (cG_w = 1), 3x3, stride 1 ----
// dW[tap][c] = sum_o x[o + tap - pad][c] * g[o] is a reduction with 9 cX outputs: no matrix core needed, HBM-bound on the ONE read
// of x (the generic kernel above takes one pass over x per tap: 1.0 GB for a 113 MB fp32 tensor, 0.34 ms for the 64-channel head at
// 128 x 108).  Thread = (8-channel chunk, pixel slot): per x pixel one 16-byte load (bf16) or two (fp32) and 9 gradient scalars
// (neighbouring output pixels: served by L1 / L2), 72 register accumulators; lanes of a chunk are folded with xor-shuffles, waves
// through LDS, workgroups through [block][tap][cX] slabs finished by stream_head_reduce_kernel (fp64, fixed order: deterministic).
#define SWH_BLOCKS 512
template <int C8, bool XB, bool GB>
__global__ __launch_bounds__(256) void stream_head_wgrad_kernel(const void* __restrict__ X, int ldX, int xoff,
                                                                const void* __restrict__ G, int ldG, int goff,
                                                                float* __restrict__ part, int n, int h, int w, int pad) {
  constexpr int PPB = 256 / C8, CX = 8 * C8;
  __shared__ float red[4][9 * CX];
  const int chunk = threadIdx.x % C8, slot = threadIdx.x / C8;
  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
  const long npix = (long)n * h * w;
  for (long p = (long)blockIdx.x * PPB + slot; p < npix; p += (long)gridDim.x * PPB) {
    const int xx = (int)(p % w);
    const long r = p / w;
    const int yy = (int)(r % h);
    float xv[8];
    if (XB) {
      const uint4 v = *(const uint4*)((const bf16_t*)X + p * ldX + xoff + chunk * 8);
      xv[0] = cb_lo(v.x), xv[1] = cb_hi(v.x), xv[2] = cb_lo(v.y), xv[3] = cb_hi(v.y);
      xv[4] = cb_lo(v.z), xv[5] = cb_hi(v.z), xv[6] = cb_lo(v.w), xv[7] = cb_hi(v.w);
    } else {
      const float4 v0 = *(const float4*)((const float*)X + p * ldX + xoff + chunk * 8);
      const float4 v1 = *(const float4*)((const float*)X + p * ldX + xoff + chunk * 8 + 4);
      xv[0] = v0.x, xv[1] = v0.y, xv[2] = v0.z, xv[3] = v0.w, xv[4] = v1.x, xv[5] = v1.y, xv[6] = v1.z, xv[7] = v1.w;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int oy = yy - ky + pad, ox = xx - kx + pad;
        float g = 0.f;
        if ((unsigned)oy < (unsigned)h && (unsigned)ox < (unsigned)w) {
          const long o = p + (long)(pad - ky) * w + (pad - kx);
          g = GB ? __uint_as_float((unsigned)((const bf16_t*)G)[o * ldG + goff] << 16) : ((const float*)G)[o * ldG + goff];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ky * 3 + kx][j] = fmaf(g, xv[j], acc[ky * 3 + kx][j]);
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[t][j];
#pragma unroll
      for (int m = C8; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
      if (lane < C8) red[wave][t * CX + chunk * 8 + j] = a;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 9 * CX; i += 256)
    part[(long)blockIdx.x * (9 * CX) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}
// gw[0][x][tap] = sum over the workgroup slabs, one wave per output (lanes stride over the slabs in fp64, fixed fold order)
__global__ __launch_bounds__(256) void stream_head_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw,
                                                                 int nslab, int cX, int cXw) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= 9 * cXw) return;
  const int tap = o / cXw, x = o % cXw;
  double s = 0.0;
  for (int k = lane; k < nslab; k += 64) s += (double)part[(long)k * (9 * cX) + tap * cX + x];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) gw[(long)x * 9 + tap] = (float)s;
}
// The head form's predicate (cG <= 4: the padded gradient tensor of a disparity head; pad == 1: the only padding with hX == hG for a
// 3 x 3 window; a bf16 x is read in 16-byte vectors).  stream_wgrad_workspace sizes the head form's slabs under cG <= 4 && k == 3:
// the run's condition is a subset of the condition the workspace query sizes for, for both storages.
static bool stream_head_eligible(int x_bf16, int ldX, int xoff, int hX, int wX, int cX, int hG, int wG, int cG, int cG_w, int k,
                                 int stride, int pad) {
  static const bool off = getenv("DIS_CONVG_HEAD_WGRAD") && getenv("DIS_CONVG_HEAD_WGRAD")[0] == '0';
  return !off && cG <= 4 && cG_w == 1 && k == 3 && stride == 1 && pad == 1 && hX == hG && wX == wG &&
         (cX == 16 || cX == 32 || cX == 64 || cX == 128) && !(x_bf16 && ((ldX | xoff) & 7));
}
template <bool XB, bool GB>
static void stream_head_launch(int c8, int blocks, const void* X, int ldX, int xoff, const void* G, int ldG, int goff,
                               float* part, int n, int h, int w, int pad, hipStream_t s) {
#define SWH_CASE(C8_) \
  if (c8 == C8_)      \
    hipLaunchKernelGGL((stream_head_wgrad_kernel<C8_, XB, GB>), dim3(blocks), dim3(256), 0, s, X, ldX, xoff, G, ldG, goff, part, n, \
                       h, w, pad);
  SWH_CASE(2) SWH_CASE(4) SWH_CASE(8) SWH_CASE(16)
#undef SWH_CASE
}
template <bool XB, bool GB>
static void stream_wgrad_launch(const StreamWgArgs& a, int mtw, int ntw, dim3 grid, hipStream_t s) {
  if (mtw == 2 && ntw == 2) hipLaunchKernelGGL((stream_wgrad_kernel<2, 2, XB, GB>), grid, dim3(256), 0, s, a);
  else if (mtw == 2) hipLaunchKernelGGL((stream_wgrad_kernel<2, 1, XB, GB>), grid, dim3(256), 0, s, a);
  else if (ntw == 2) hipLaunchKernelGGL((stream_wgrad_kernel<1, 2, XB, GB>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((stream_wgrad_kernel<1, 1, XB, GB>), grid, dim3(256), 0, s, a);
}
// launch F<XB, GB> for the storage flags of the two operands
#define STREAM_BY_STORAGE(F, ...)                          \
  do {                                                     \
    if (x_bf16 && g_bf16) F<true, true>(__VA_ARGS__);      \
    else if (x_bf16) F<true, false>(__VA_ARGS__);          \
    else if (g_bf16) F<false, true>(__VA_ARGS__);          \
    else F<false, false>(__VA_ARGS__);                     \
  } while (0)

// workspace floats of stream_wgrad_run for every form it may take (x_bf16 / g_bf16: storage of the operands, as in dis_convb_run)
static long stream_wgrad_workspace(int x_bf16, int g_bf16, int n, int hG, int wG, int cX, int cG, int k) {
  if (n <= 0 || hG <= 0 || wG <= 0 || cX <= 0 || cG <= 0 || k <= 0 || k * k > CONV_PLAN_MAXTAPS) return -1;
  const WgradSplitPlan p = wgrad_split_plan(n, hG, wG, cX, cG, k);
  const long f32 = (long)p.nsplit * k * k * (p.nxb * 32 * p.mtw) * (p.ngb * 32 * p.ntw);
  // (the slice-pair form, if the run takes it for this layer: the stride is not known here, so size for both)
  const int bf = x_bf16 && g_bf16, ld = bf ? 8 : 4;
  const long b1 = dis_wgrad_pairs_workspace(n, 1, 1, hG, wG, cX, cG, ld, ld, k, 1, bf);
  const long b2 = dis_wgrad_pairs_workspace(n, 1, 1, hG, wG, cX, cG, ld, ld, k, 2, bf);
  long b3 = b1 > b2 ? b1 : b2;
  if (cG <= 4 && k == 3 && b3 < (long)SWH_BLOCKS * 9 * cX) b3 = (long)SWH_BLOCKS * 9 * cX;  // head form
  return b3 > f32 ? b3 : f32;
}
// ld / offsets in elements of the operand's own storage
static int stream_wgrad_run(const void* X, int x_bf16, int ldX, int xoff, int hX, int wX, int cX, int cX_w, const void* G,
                            int g_bf16, int ldG, int goff, int hG, int wG, int cG, int cG_w, float* grad_w, float* workspace,
                            int n, int k, int stride, int pad, void* stream) {
  if (!X || !G || !grad_w || !workspace) return DIS_ERR_NULL;
  if (n <= 0 || hX <= 0 || wX <= 0 || hG <= 0 || wG <= 0 || cX <= 0 || cG <= 0 || cX_w <= 0 || cG_w <= 0 || cX_w > cX ||
      cG_w > cG || k <= 0 || pad < 0)
    return DIS_ERR_BAD_SHAPE;
  if ((cX & 3) || (cG & 3) || (xoff & 3) || (goff & 3) || (ldX & 3) || (ldG & 3) || xoff + cX > ldX || goff + cG > ldG)
    return DIS_ERR_BAD_SHAPE;
  if (k * k > CONV_PLAN_MAXTAPS || (stride != 1 && stride != 2)) return DIS_ERR_UNSUPPORTED;
  if ((long)n * hG * wG > 2147483647L - 64) return DIS_ERR_BAD_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  // slice pairs: both operands of one storage; bf16 ones in whole 16-byte items of 8 channels inside their pixels
  const bool pairs_ok = x_bf16 == g_bf16 && (!x_bf16 || (!((xoff | goff) & 7) && xoff + ((cX + 7) & ~7) <= ldX &&
                                                         goff + ((cG + 7) & ~7) <= ldG));
  if (pairs_ok && dis_wgrad_pairs_workspace(n, hX, wX, hG, wG, cX, cG, ldX, ldG, k, stride, x_bf16) >= 0)
    return dis_wgrad_pairs_run((const float*)X, ldX, xoff, hX, wX, cX, cX_w, (const float*)G, ldG, goff, hG, wG, cG, cG_w,
                               grad_w, workspace, n, k, stride, pad, x_bf16, s);
  if (stream_head_eligible(x_bf16, ldX, xoff, hX, wX, cX, hG, wG, cG, cG_w, k, stride, pad)) {
    const long npix = (long)n * hG * wG;
    const int c8 = cX / 8, ppb = 256 / c8;
    long blocks = (npix + ppb - 1) / ppb;
    if (blocks > SWH_BLOCKS) blocks = SWH_BLOCKS;
    DIS_TAG("stream_head_wgrad_kernel (one gradient channel)");
    STREAM_BY_STORAGE(stream_head_launch, c8, (int)blocks, X, ldX, xoff, G, ldG, goff, workspace, n, hG, wG, pad, s);
    hipLaunchKernelGGL(stream_head_reduce_kernel, dim3((unsigned)((9L * cX_w + 3) / 4)), dim3(256), 0, s,
                       (const float*)workspace, grad_w, (int)blocks, cX, cX_w);
    DIS_CHECK_LAUNCH();
    return DIS_OK;
  }
  StreamWgArgs a;
  a.X = X; a.G = G; a.part = workspace;
  a.n = n; a.hX = hX; a.wX = wX; a.ldX = ldX; a.xoff = xoff; a.cX = cX;
  a.hG = hG; a.wG = wG; a.ldG = ldG; a.goff = goff; a.cG = cG;
  a.S = stride; a.pad = pad; a.k = k;
  const WgradSplitPlan p = wgrad_split_plan(n, hG, wG, cX, cG, k);
  a.nxb = p.nxb; a.ngb = p.ngb; a.mper = p.mper;
  a.cXp = a.nxb * 32 * p.mtw;
  a.cGp = a.ngb * 32 * p.ntw;
  const dim3 grid((unsigned)(k * k * a.nxb * a.ngb), (unsigned)p.nsplit);
  DIS_TAG("stream_wgrad_kernel (fp32 MFMA, split-K slabs)");
  STREAM_BY_STORAGE(stream_wgrad_launch, a, p.mtw, p.ntw, grid, s);
  const long total = (long)k * k * cX_w * cG_w;
  hipLaunchKernelGGL(stream_wgrad_reduce_kernel, dim3(dis_ew_grid(total, 256)), dim3(256), 0, s, (const float*)workspace,
                     grad_w, p.nsplit, k * k, a.cXp, a.cGp, cX_w, cG_w);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}

extern "C" long dis_convg_wgrad_workspace(int n, int hG, int wG, int cX, int cG, int k) {
  return stream_wgrad_workspace(0, 0, n, hG, wG, cX, cG, k);
}
extern "C" int dis_convg_wgrad(const float* X, int ldX, int xoff, int hX, int wX, int cX, int cX_w, const float* G,
                               int ldG, int goff, int hG, int wG, int cG, int cG_w, float* grad_w, float* workspace,
                               int n, int k, int stride, int pad, void* stream) {
  return stream_wgrad_run(X, 0, ldX, xoff, hX, wX, cX, cX_w, G, 0, ldG, goff, hG, wG, cG, cG_w, grad_w, workspace, n, k, stride,
                          pad, stream);
}
// (the storage of the operands is not known to the query: the sizes do not depend on it, and bf16 pairs exist wherever fp32 ones do)
extern "C" long dis_convb_wgrad_workspace(int n, int hG, int wG, int cX, int cG, int k) {
  return stream_wgrad_workspace(1, 1, n, hG, wG, cX, cG, k);
}
extern "C" int dis_convb_wgrad(const void* X, int x_bf16, int ldX, int xoff, int hX, int wX, int cX, int cX_w, const void* G,
                               int g_bf16, int ldG, int goff, int hG, int wG, int cG, int cG_w, float* grad_w,
                               float* workspace, int n, int k, int stride, int pad, void* stream) {
  return stream_wgrad_run(X, x_bf16 != 0, ldX, xoff, hX, wX, cX, cX_w, G, g_bf16 != 0, ldG, goff, hG, wG, cG, cG_w, grad_w,
                          workspace, n, k, stride, pad, stream);
}
