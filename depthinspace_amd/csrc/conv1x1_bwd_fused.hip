// One-launch backward of the 1 x 1 multi-frame convolution of Block2D3D (conv_mf: y = conv(x * xscale), 128 -> 32 channels, followed
// by GroupNorm(1 group)): input gradient and weight / bias gradient from ONE staging of the operand.
//
// The two launches it replaces: conv_fwd_kernel<32, 128, 1, 1, 1, GNB> forms gpre = act'(q) (g k1_c + q kx + k0) - the elementwise
// pass of the GroupNorm backward - while it stages g, multiplies it with W^T and STORES gpre (113 MB at core resolution) only so that
// conv_wgrad_kernel<128, 32, 1, 1, 1> can read it back.  Here a workgroup (4 waves, persistent over 4 x 16 pixel tiles) stages gpre
// (64 pixels x 32) and x * xscale (64 pixels x 128) in LDS once per tile and runs both products on v_mfma_f32_16x16x4_f32:
//   * input gradient: the GNB kernel's staging arithmetic, fragment order (q 0..1, e 0..3, one accumulator chain per 16-channel output
//     tile, wave w = tile row w) and yscale / accumulate epilogue: gx is the same bits;
//   * weight gradient: dW[ci][co] = sum over pixels (x xscale)[pixel][ci] gpre[pixel][co]; the 8 x 2 accumulator tiles are split over
//     the waves (wave w: input channels 32 w .. 32 w + 31), each wave contracts all 64 pixels of a tile, the accumulators stay in
//     registers over all tiles of the workgroup: no cross-wave add.  One slab [128][32] per workgroup in conv_wgrad_kernel's layout,
//     summed by wgrad_reduce_kernel (fixed order, fp64): no float atomics, repeated runs give the same bits;
//   * bias gradient: as conv_wgrad_kernel - wave w sums tile row w (k-steps 4 w .. 4 w + 3: that kernel's grouping and order), per-workgroup partials.
// gpre never reaches HBM.  LDS: 16 KB weights + 9 KB gpre + 36 KB x = 61.5 KB, two workgroups per CU.
#include "conv_args.h"

#define MFB_GS 36    // gpre pixel stride in LDS (floats): ConvCfg<32, 128, 1, 1, 1>::CS
#define MFB_XS 144   // x pixel stride: WgCfg<128, 32, 1, 1, 1>::CS (== 16 mod 32: the b32 fragment reads of 4 pixels hit disjoint banks)
#define MFB_W_FLOATS (32 * 128)
#define MFB_LDS_BYTES ((MFB_W_FLOATS + 64 * MFB_GS + 64 * MFB_XS + 128) * 4)

__global__ __launch_bounds__(256, 2) void conv1x1_bwd_fused_kernel(MfbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mfb_smem[];
  float* wl = mfb_smem;
  float* gl = wl + MFB_W_FLOATS;
  float* xl = gl + 64 * MFB_GS;
  float* red = xl + 64 * MFB_XS;
  for (int i = threadIdx.x; i < MFB_W_FLOATS / 4; i += 256) ((float4*)wl)[i] = ((const float4*)a.w)[i];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int tiles_x = (a.wd + 15) / 16, tiles_y = (a.h + 3) / 4;
  const int ntiles = a.n * tiles_y * tiles_x;

  // staging items: g / q 64 pixels x 8 float4 (2 per thread, channel group threadIdx % 8); x 64 pixels x 32 float4 (8 per thread,
  // channel group threadIdx % 32).  Loads are unconditional at clamped addresses and zeroed when they are written to LDS.
  float4 pg[2], pq[2], px[8];
  float psc[8];
  unsigned okg = 0, okx = 0;
  int st_n = 0, cf_n = -1;
  float4 cf_k1 = make_float4(0.f, 0.f, 0.f, 0.f);
  float cf_kx = 0.f, cf_k0 = 0.f;
  const int gvv = threadIdx.x & 7, xvv = threadIdx.x & 31;
  auto prefetch = [&](int tile) {
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
    st_n = n;
    okg = 0, okx = 0;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int pix = ((int)threadIdx.x >> 3) + it * 32;
      const int y = ty * 4 + (pix >> 4), x = tx * 16 + (pix & 15);
      const long off = ((long)n * a.h + min(y, a.h - 1)) * a.wd + min(x, a.wd - 1);
      pg[it] = *(const float4*)(a.g + off * 32 + gvv * 4);
      pq[it] = *(const float4*)(a.q + off * 32 + gvv * 4);
      okg |= ((y < a.h && x < a.wd) ? 1u : 0u) << it;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int pix = ((int)threadIdx.x >> 5) + it * 8;
      const int y = ty * 4 + (pix >> 4), x = tx * 16 + (pix & 15);
      const long off = ((long)n * a.h + min(y, a.h - 1)) * a.wd + min(x, a.wd - 1);
      px[it] = *(const float4*)(a.x + off * 128 + xvv * 4);
      psc[it] = a.xscale ? a.xscale[off * 4 + (xvv >> 3)] : 1.f;
      okx |= ((y < a.h && x < a.wd) ? 1u : 0u) << it;
    }
  };
  auto stage = [&]() {
    if (st_n != cf_n) {
      cf_n = st_n;
      const float* cf = a.coef + (long)st_n * (32 + 2);
      cf_k1 = *(const float4*)(cf + gvv * 4);
      cf_kx = cf[32];
      cf_k0 = cf[33];
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int pix = ((int)threadIdx.x >> 3) + it * 32;
      const float4 q = pq[it];
      float4 v = pg[it];
      v.x = __builtin_fmaf(v.x, cf_k1.x, __builtin_fmaf(q.x, cf_kx, cf_k0));
      v.y = __builtin_fmaf(v.y, cf_k1.y, __builtin_fmaf(q.y, cf_kx, cf_k0));
      v.z = __builtin_fmaf(v.z, cf_k1.z, __builtin_fmaf(q.z, cf_kx, cf_k0));
      v.w = __builtin_fmaf(v.w, cf_k1.w, __builtin_fmaf(q.w, cf_kx, cf_k0));
      if (a.in_act != DIS_ACT_NONE) {
        v.x *= act_grad_from_out(q.x, a.in_act), v.y *= act_grad_from_out(q.y, a.in_act);
        v.z *= act_grad_from_out(q.z, a.in_act), v.w *= act_grad_from_out(q.w, a.in_act);
      }
      *(float4*)(gl + pix * MFB_GS + gvv * 4) = ((okg >> it) & 1u) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int pix = ((int)threadIdx.x >> 5) + it * 8;
      const float sc = psc[it];
      *(float4*)(xl + pix * MFB_XS + xvv * 4) =
          ((okx >> it) & 1u) ? make_float4(px[it].x * sc, px[it].y * sc, px[it].z * sc, px[it].w * sc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  f32x4 wacc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) wacc[m][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum0 = 0.f, bsum1 = 0.f;

  int tile = blockIdx.x;
  if (tile < ntiles) prefetch(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();   // every wave finished reading the previous tile (and the weights are in)
    stage();
    __syncthreads();
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
    const int vy = ty * 4 + wave, vx0 = tx * 16 + lg * 4;
    // this tile's output multipliers first, then the next tile's operands: they land while the MFMAs below run
    float4 ysc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      ysc[r] = a.yscale ? *(const float4*)(a.yscale + (((long)n * a.h + min(vy, a.h - 1)) * a.wd + min(vx0 + r, a.wd - 1)) * 4)
                        : make_float4(1.f, 1.f, 1.f, 1.f);
    if (tile + (int)gridDim.x < ntiles) prefetch(tile + gridDim.x);

    // ---- input gradient: gx[pixel][128] = gpre[pixel][32] W^T (conv_fwd_kernel<32, 128, 1, 1, 1, GNB>'s sequence)
    f32x4 acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const f32x4 av = *(const f32x4*)(gl + (wave * 16 + li) * MFB_GS + lg * 8 + q2 * 4);
      f32x4 bv[8];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) bv[nt] = *(const f32x4*)(wl + ((lg * 2 + q2) * 128 + nt * 16 + li) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[nt][e], acc[nt], 0, 0, 0);
    }
    if (a.yscale) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv[4] = {ysc[r].x, ysc[r].y, ysc[r].z, ysc[r].w};
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) acc[nt][r] *= sv[(nt >> 1) & 3];
      }
    }
    if (vy < a.h) {
      float* ybase = a.gx + (((long)n * a.h + vy) * a.wd + vx0) * 128 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (vx0 + r < a.wd) {
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) {
            float* yp = ybase + r * 128 + nt * 16;
            float v = acc[nt][r] + 0.f;   // (the GNB launch adds its absent bias as 0.f)
            if (a.accum) v += *yp;
            *yp = v;
          }
        }
    }

    // ---- weight gradient: 16 k-steps of 4 pixels; this wave's rows are input channels 32 wave .. 32 wave + 31
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int pk = st * 4 + lg;
      const float b0 = gl[pk * MFB_GS + li], b1 = gl[pk * MFB_GS + 16 + li];
      if ((st >> 2) == wave) bsum0 += b0, bsum1 += b1;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float av = xl[pk * MFB_XS + (wave * 2 + m) * 16 + li];
        wacc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, wacc[m][0], 0, 0, 0);
        wacc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, wacc[m][1], 0, 0, 0);
      }
    }
  }

  // the slab [ci][co]: accumulator register r of lane (li, lg) is row lg * 4 + r, column li of its 16 x 16 tile
  float* out = a.part + (long)blockIdx.x * (128 * 32);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[((wave * 2 + m) * 16 + lg * 4 + r) * 32 + nb * 16 + li] = wacc[m][nb][r];
  if (a.bpart) {
    float v0 = bsum0, v1 = bsum1;
    v0 += __shfl_xor(v0, 16, 64);
    v0 += __shfl_xor(v0, 32, 64);
    v1 += __shfl_xor(v1, 16, 64);
    v1 += __shfl_xor(v1, 32, 64);
    if (lg == 0) red[(wave * 2 + 0) * 16 + li] = v0, red[(wave * 2 + 1) * 16 + li] = v1;
    __syncthreads();
    if (threadIdx.x < 32) {
      const int nb = threadIdx.x >> 4, l2 = threadIdx.x & 15;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) sum += red[(w * 2 + nb) * 16 + l2];
      a.bpart[(long)blockIdx.x * 32 + threadIdx.x] = sum;
    }
  }
}

hipError_t dis_mfb_launch(const MfbArgs& a, long grid, hipStream_t stream) {
  static_assert(MFB_LDS_BYTES <= 64 * 1024, "two workgroups per CU");
  hipLaunchKernelGGL(conv1x1_bwd_fused_kernel, dim3((unsigned)grid), dim3(256), MFB_LDS_BYTES, stream, a);
  return hipGetLastError();
}
