// Input gradient AND weight gradient of a 3x3 stride-1 pad-1 convolution C -> C (C = 32) in ONE launch, three-term bf16 operands.
//
// The strict split's form of conv_bwd_fused.hip: every fp32 operand is split into three bf16 terms (split3_pair, no scale: bf16 has
// fp32's exponent range) and a product is the six terms a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1 on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation, as conv_bf16x3_kernel (input gradient) and conv_wgrad_bf16x3_kernel (weight gradient) compute them.  The gy halo a
// tile stages serves both products:
//     gx[q][ci]        = sum_tap sum_co gy[q + 1 - tap][co] W[co][ci][tap]          (contraction over channels, per tile)
//     dW[tap][ci][co]  = sum_q'  x[q'][ci] gy[q' + 1 - tap][co]                     (contraction over the pixels q' a tile OWNS)
// gx: the same weight planes, the same k-step order (kx outer, ky inner) and the same six products per k-step as conv_bf16x3_kernel
// with mode-1 OIHW weights, accumulated from zero: each output element sees the same sequence of matrix instructions on the same
// operands, so gx is BIT-identical to dis_conv2d_fwd_bf16x3_oihw(mode 1) / dis_conv2d_dgrad_bf16x3_act.
//
// Shape of the kernel: 8 waves, two per SIMD, one workgroup per CU (grid = #CUs, persistent over the tiles of its XCD's share).
// The tile is 8 x 16 pixels (three planes make a 16 x 16 tile's halo + x tile + weights 185 KB of LDS; 8 x 16 needs 121 KB).
// Per tile:
//   barrier A  (every wave has left the previous tile)
//   staging  the gy halo (10 x 18 x 32, times act'(y) when INACT) and the x tile (8 x 16 x 32, GroupNorm applied when XGN) go to LDS
//            as three bf16 planes; the bias gradient sums the halo items the tile owns
//   barrier B  (the next tile's halo and x pieces are requested into the registers the staging emptied)
//   D        input gradient: wave w owns tile row w (2 accumulator tiles), 9 taps x 6 products, then its 2 float4 stores per lane
//   W        weight gradient: wave (kh, ah, bh) = (w >> 2, (w >> 1) & 1, w & 1) owns the 9 tap tiles of (ci half ah, co half bh) over
//            tile rows 4 kh .. 4 kh + 3 (2 k-steps of 32 pixels), x^T and the shifted gy fragments read with ds_read_b64_tr_b16
// The two kh halves of a (ci half, co half) are added once at the end of the launch (kh 0 + kh 1, fixed order), and the workgroup's
// slab is summed over workgroups by wgrad_reduce_kernel (fixed order, fp64): no float atomics, bit-reproducible.
// LDS: weights 55.3 KB + halo 40.3 KB + x tile 28.7 KB = 124.3 KB.
#include "conv_bwd_fused_common.h"

struct F3Cfg {
  static constexpr int C = 32, TR = 8, TC = 16, IR = TR + 2, IC = TC + 2, CV = C / 4, NP = 3, NT = 2, KS = 9;
  static constexpr int PS = 112;   // LDS pixel stride (16-bit units): 3 planes + 32 B pad, 2 (mod 4) sixteen-byte units as in BxCfg
  static constexpr int NW = 8, NTHR = 64 * NW;
  static constexpr int W_U16 = KS * NP * 4 * C * 8, X_U16 = IR * IC * PS, XT_U16 = TR * TC * PS;
  static constexpr int NITEMS = IR * IC * CV, NLOAD = (NITEMS + NTHR - 1) / NTHR;
  static constexpr int LDS_BYTES = (W_U16 + X_U16 + XT_U16) * 2;
};
static_assert(F3Cfg::LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(F3Cfg::NW == 8 && F3Cfg::TR == F3Cfg::NW, "one tile row per wave in D, two k-steps per wave in W");
static_assert(32 * (32 * 9 + 1) * 4 <= (F3Cfg::X_U16 + F3Cfg::XT_U16) * 2, "the weight prologue's fp32 scratch aliases halo + x tile");
static_assert(4 * 9 * 4 * 64 * 4 <= F3Cfg::X_U16 * 2, "the kh = 1 accumulators alias the halo");
static_assert((F3Cfg::NTHR / F3Cfg::CV) * F3Cfg::C * 8 <= F3Cfg::XT_U16 * 2, "the bias partials alias the x tile");

// INACT: the operand of both products is gy * act'(y) (y = c.xact, the conv's activated output).  ACCUM: gx += the input gradient.
// XGN: the weight gradient's x is staged as GroupNorm(x) (FbArgs::wx_gn_*).
template <int INACT, bool ACCUM, bool XGN>
__global__ __launch_bounds__(512) void conv_bwd_fused_bf16x3_kernel(FbArgs fa_) {
  using K = F3Cfg;
  const ConvArgs& a = fa_.c;
  constexpr int C = K::C, IC = K::IC, PS = K::PS, NT = K::NT, KS = K::KS, NLOAD = K::NLOAD, CV = K::CV, NP = K::NP;
  constexpr int TR = K::TR, TC = K::TC, NTHR = K::NTHR;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem16[];
  unsigned short* wl = smem16;                          // weights, fragment order, three planes
  unsigned short* xh = smem16 + K::W_U16;               // the gy halo of the current tile [10 x 18 pixels][plane][channel]
  unsigned short* xt = smem16 + K::W_U16 + K::X_U16;    // the x tile of the current tile  [8 x 16 pixels][plane][channel]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4, tq = li >> 2, tp = li & 3;
  const int kh = wave >> 2, ah = (wave >> 1) & 1, bh = wave & 1;   // dW: this wave's (row half, ci half, co half)
  const int tiles_x = (a.wv + TC - 1) / TC, tiles_y = (a.hv + TR - 1) / TR;
  // (fbc_tile_share's and fbc_advance's arithmetic, spelled out: through either helper the compiler allocates this kernel's scalar
  //  registers differently - profiles/r9_bwd_fused_shared.md - and the device code of this family is held to the byte)
  const int ntiles = a.n * tiles_y * tiles_x;
  const int nxcd = (gridDim.x % 8 == 0) ? 8 : 1;
  const int xcd = blockIdx.x % nxcd, rank = blockIdx.x / nxcd, per = gridDim.x / nxcd;
  const int t_lo = (int)((long)ntiles * xcd / nxcd), t_hi = (int)((long)ntiles * (xcd + 1) / nxcd);
  const int d_tx = per % tiles_x, d_ty = (per / tiles_x) % tiles_y, d_n = per / (tiles_x * tiles_y);

  // ---- halo items of this thread (as conv_bf16x3_kernel): (row, col) inside the 10 x 18 halo and the byte offset from its first
  // pixel; items past the end of the halo get a row outside every image.  512 % CV == 0: a thread's 4 channels are the same in all.
  float4 pre[NLOAD], pre2[INACT ? NLOAD : 1];
  int it_rc[NLOAD], it_off[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) {
    const int idx = (int)threadIdx.x + it * NTHR;
    const int vv = idx % CV, pix = idx / CV;
    const int r = pix / IC, c = pix % IC;
    it_rc[it] = idx < K::NITEMS ? (r | (c << 16)) : 0x4000;
    it_off[it] = ((r * a.win + c) * C + vv * 4) * 4;
  }
  const unsigned x_bytes = (unsigned)a.hin * a.win * (C * 4u), y_bytes = (unsigned)a.hf * a.wf * (C * 4u);
  const float* pf_x = a.x;
  unsigned pf_bytes = 0;
  int pf_iy0 = 0, pf_ix0 = 0, pf_off0 = 0;
  auto pf_setup = [&](int n, int ty, int tx, bool live) {
    pf_iy0 = ty * TR - 1;
    pf_ix0 = tx * TC - 1;
    pf_off0 = (pf_iy0 * a.win + pf_ix0) * (C * 4);
    pf_x = a.x + (long)n * a.hin * a.win * C;
    pf_bytes = live ? x_bytes : 0u;   // no next tile: every load is out of range
  };
  auto pf_issue = [&](int it) {
    const int iy = pf_iy0 + (it_rc[it] & 0xffff), ix = pf_ix0 + (it_rc[it] >> 16);
    const bool ok = (unsigned)iy < (unsigned)a.hin && (unsigned)ix < (unsigned)a.win;
    const unsigned off = ok ? (unsigned)(pf_off0 + it_off[it]) : BX_OOB;
    pre[it] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(pf_x, pf_bytes), off, 0, 0));
    if (INACT)
      pre2[it] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(a.xact + (pf_x - a.x), pf_bytes), off, 0, 0));
  };

  // ---- centre pieces of this lane: tile row `wave`, column li, channels 16 nt + 4 lg .. (x for dW, fetched one tile ahead; gx so far)
  const int y_lane = ((wave * a.wf + li) * C + lg * 4) * 4;
  auto centre_off = [&](int ty, int tx) -> unsigned {
    const int vy = ty * TR + wave, vx = tx * TC + li;
    return (vx < a.wv && vy < a.hv) ? (unsigned)((ty * TR * a.wf + tx * TC) * (C * 4) + y_lane) : BX_OOB;
  };
  float4 cxw[NT], cy[ACCUM ? NT : 1];
  auto x_issue = [&](int n, int ty, int tx, bool live) {
    const unsigned off = centre_off(ty, tx);
    const float* xb = fa_.wx + (long)n * a.hf * a.wf * C;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      cxw[nt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(xb, live ? y_bytes : 0u), off + nt * 64, 0, 0));
  };

  int tile = t_lo + rank;
  int cn = 0, cty = 0, ctx = 0;
  if (tile < t_hi) {
    ctx = tile % tiles_x, cty = (tile / tiles_x) % tiles_y, cn = tile / (tiles_x * tiles_y);
    pf_setup(cn, cty, ctx, true);
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) pf_issue(it);   // (in flight while the weights are split)
    x_issue(cn, cty, ctx, true);
  }

  // ---- weights: OIHW fp32 -> three bf16 planes in fragment order (conv_bf16x3_kernel's OIHW prologue, mode 1; the fp32 copy sits
  // in the halo and x tile, which are first written after barrier A of the first tile)
  {
    float* ws = (float*)xh;
    const int row = a.w_i * 9;
    dis_copy_w_rows(a.w, a.w_o, row, a.w_rs, ws);
    __syncthreads();
    for (int u = threadIdx.x; u < KS * 4 * C; u += NTHR) {
      const int co = u % C, g = (u / C) & 3, ks = u / (4 * C);
      unsigned pl[NP][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v0 = fbc_weight<32>(ws, row + 1, a.w_o, a.w_i, ks, g, 2 * j, co);
        const float v1 = fbc_weight<32>(ws, row + 1, a.w_o, a.w_i, ks, g, 2 * j + 1, co);
        split3_pair(v0, v1, pl[0][j], pl[1][j], pl[2][j]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
        *(uint4*)(wl + (((ks * NP + p) * 4 + g) * C + co) * 8) = make_uint4(pl[p][0], pl[p][1], pl[p][2], pl[p][3]);
    }
  }

  f32x4 accw[9];   // dW: tap j of this wave's (ci half, co half), over its row half of every tile
#pragma unroll
  for (int j = 0; j < 9; ++j) accw[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // bias gradient: this thread's 4 channels over the pixels its tiles own (fp64: one fp32 rounding per workgroup partial)
  double bsum[4] = {0.0, 0.0, 0.0, 0.0};
  float4 xg_sc[XGN ? NT : 1], xg_sh[XGN ? NT : 1];   // XGN: GroupNorm's affine map for this lane's 8 channels, per sample
  int xg_n = -1;
#pragma unroll
  for (int nt = 0; nt < (XGN ? NT : 1); ++nt) xg_sc[nt] = xg_sh[nt] = make_float4(0.f, 0.f, 0.f, 0.f);

  using PO = FbcOrder3;   // the six products of a k-step
  const int xa_lane = (wave * IC + li) * PS + lg * 8;
  const int lds_vv = ((int)threadIdx.x % CV) * 4;

  while (tile < t_hi) {
    const unsigned cur_off = centre_off(cty, ctx);
    float* cur_y = a.y + (long)cn * a.hf * a.wf * C;
    if (XGN && cn != xg_n) {
      xg_n = cn;
      fbc_gn_affine<NT>(fa_, cn, (double)a.hf * a.wf * C, lg, xg_sc, xg_sh);
    }
    // barrier A: every wave has finished the previous tile (and, first tile, the weight split has read its fp32 copy)
    __syncthreads();

    // ---- staging: the halo (gy, or gy act'(y)) and the x tile as three bf16 planes
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) {
      const int idx = (int)threadIdx.x + it * NTHR;
      if (idx < K::NITEMS) {
        float4 v = pre[it];
        if (INACT) {
          const float4 q = pre2[it];
          v.x *= act_grad_from_out(q.x, INACT), v.y *= act_grad_from_out(q.y, INACT);
          v.z *= act_grad_from_out(q.z, INACT), v.w *= act_grad_from_out(q.w, INACT);
        }
        const int r = it_rc[it] & 0xffff, c = it_rc[it] >> 16;
        if (r >= 1 && r <= TR && c >= 1 && c <= TC) bsum[0] += v.x, bsum[1] += v.y, bsum[2] += v.z, bsum[3] += v.w;
        unsigned a1, a2, a3, b1, b2, b3;
        split3_pair(v.x, v.y, a1, a2, a3);
        split3_pair(v.z, v.w, b1, b2, b3);
        unsigned short* p = xh + (idx / CV) * PS + lds_vv;
        *(uint2*)(p) = make_uint2(a1, b1);
        *(uint2*)(p + C) = make_uint2(a2, b2);
        *(uint2*)(p + 2 * C) = make_uint2(a3, b3);
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float4 v = cxw[nt];
      if (XGN) {   // (pixels past the map stay zero)
        v.x = v.x * xg_sc[nt].x + xg_sh[nt].x, v.y = v.y * xg_sc[nt].y + xg_sh[nt].y;
        v.z = v.z * xg_sc[nt].z + xg_sh[nt].z, v.w = v.w * xg_sc[nt].w + xg_sh[nt].w;
        v = cur_off != BX_OOB ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      unsigned a1, a2, a3, b1, b2, b3;
      split3_pair(v.x, v.y, a1, a2, a3);
      split3_pair(v.z, v.w, b1, b2, b3);
      unsigned short* p = xt + (wave * TC + li) * PS + nt * 16 + lg * 4;
      *(uint2*)(p) = make_uint2(a1, b1);
      *(uint2*)(p + C) = make_uint2(a2, b2);
      *(uint2*)(p + 2 * C) = make_uint2(a3, b3);
    }
    // barrier B: halo, x tile (and, first tile, the weight planes) are complete
    __syncthreads();

    // the next tile's halo and x pieces, and this tile's old gx (ACCUM), are requested under the products
    int n1 = cn + d_n, ty1 = cty + d_ty, tx1 = ctx + d_tx;
    if (tx1 >= tiles_x) tx1 -= tiles_x, ++ty1;
    if (ty1 >= tiles_y) ty1 -= tiles_y, ++n1;
    const bool live1 = tile + per < t_hi;
    pf_setup(n1, ty1, tx1, live1);
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) pf_issue(it);
    x_issue(n1, ty1, tx1, live1);
    if (ACCUM) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        cy[nt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(cur_y, y_bytes), cur_off + nt * 64, 0, 0));
    }

    // ---------------- input gradient: 9 k-steps (kx outer, ky inner) x 6 products x 2 channel blocks
    {
      f32x4 acc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      s16x8 R[2][3][NP];    // [kx parity][halo row w + j][plane]
      s16x8 fw[2][NP][NT];  // [buffer][plane][nt]
      auto load_rows = [&](int kx) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int p = 0; p < NP; ++p) R[kx & 1][j][p] = *(const s16x8*)(xh + xa_lane + (j * IC + kx) * PS + p * C);
      };
      auto load_w = [&](int ks, s16x8 (&B)[NP][NT]) __attribute__((always_inline)) {
        const int wt = (ks % 3) * 3 + ks / 3;   // the weights are packed tap-major (ky * 3 + kx)
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) B[p][nt] = *(const s16x8*)(wl + (((wt * NP + p) * 4 + lg) * C + nt * 16 + li) * 8);
      };
      load_rows(0);
      load_w(0, fw[0]);
      fbc_static_for<0, KS>([&](auto ksc) __attribute__((always_inline)) {
        constexpr int ks = decltype(ksc)::value;
        constexpr int kx = ks / 3, ky = ks % 3, b = ks & 1;
        if (ks + 1 < KS) {
          load_w(ks + 1, fw[b ^ 1]);
          if (ky == 2) load_rows(kx + 1);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fw[b][PO::PB[q]][nt]),
                                                              __builtin_bit_cast(bf16x8, R[kx & 1][ky][PO::PA[q]]), acc[nt], 0, 0, 0);
      });
      // epilogue (conv_bf16x3_kernel's with no bias and no activation: acc, + the old value when accumulating)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 o = acc[nt];
        if (ACCUM) {
          const float4 q = cy[ACCUM ? nt : 0];
          o += (f32x4){q.x, q.y, q.z, q.w};
        }
        const u32x4 ov = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
        __builtin_amdgcn_raw_buffer_store_b128(ov, bx_rsrc(cur_y, y_bytes), cur_off + nt * 64, 0, 0);
      }
    }

    // ---------------- weight gradient: this wave's 9 tap tiles over tile rows 4 kh .. 4 kh + 3: 2 k-steps of 32 pixels (rows 2 ks,
    // 2 ks + 1), x^T fragments (three planes) against the gy fragments of the 9 tap shifts - centre pixel (r', c') meets the halo pixel
    // (r' + 2 - ky, c' + 2 - kx)
    fbc_static_for<0, 2>([&](auto sc) __attribute__((always_inline)) {
      const int ks = 2 * kh + decltype(sc)::value;
      s16x8 fx[NP];
      const unsigned short* xq = xt + (2 * ks * TC + 4 * lg + tq) * PS + ah * 16 + tp * 4;
#pragma unroll
      for (int p = 0; p < NP; ++p) fx[p] = fbc_tr_read8(xq + p * C, xq + TC * PS + p * C);
      s16x8 G[2][3][NP];   // [ky parity][kx][plane]
      auto load_g = [&](int ky, s16x8 (&Gk)[3][NP]) __attribute__((always_inline)) {
        const int row0 = 2 * ks + 2 - ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const unsigned short* gq = xh + (row0 * IC + (4 * lg + tq) + 2 - kx) * PS + bh * 16 + tp * 4;
#pragma unroll
          for (int p = 0; p < NP; ++p) Gk[kx][p] = fbc_tr_read8(gq + p * C, gq + IC * PS + p * C);
        }
      };
      load_g(0, G[0]);
      fbc_static_for<0, 3>([&](auto kyc) __attribute__((always_inline)) {
        constexpr int ky = decltype(kyc)::value;
        if (ky + 1 < 3) load_g(ky + 1, G[(ky + 1) & 1]);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int q = 0; q < 6; ++q)
            accw[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fx[PO::PA[q]]),
                                                                        __builtin_bit_cast(bf16x8, G[ky & 1][kx][PO::PB[q]]), accw[ky * 3 + kx], 0, 0, 0);
      });
    });

    cn = n1, cty = ty1, ctx = tx1;
    tile += per;
  }

  // ---------------- the workgroup's results leave: the two row halves of dW added (kh 0 + kh 1), its slab, its bias partials
  __syncthreads();   // (every wave is done with the halo and the x tile: the scratch below aliases them)
  float* red = (float*)xh;   // [wave & 3][tap][r][lane]
  double* bred = (double*)xt;  // [NTHR / CV][C]
  if (kh == 1) {
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(((wave & 3) * 9 + j) * 4 + r) * 64 + lane] = accw[j][r];
  }
  if (fa_.bpart) {
    const int vv = threadIdx.x % CV, row = threadIdx.x / CV;
#pragma unroll
    for (int k = 0; k < 4; ++k) bred[row * C + vv * 4 + k] = bsum[k];
  }
  __syncthreads();
  if (kh == 0) {
    float* out = fa_.part + (long)blockIdx.x * (9 * C * C);
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[((j * 2 + ah) * 16 + lg * 4 + r) * C + bh * 16 + li] = accw[j][r] + red[(((wave & 3) * 9 + j) * 4 + r) * 64 + lane];
  }
  if (fa_.bpart && threadIdx.x < C) {
    double sum = 0.0;
    for (int r = 0; r < NTHR / CV; ++r) sum += bred[r * C + threadIdx.x];
    fa_.bpart[(long)blockIdx.x * C + threadIdx.x] = (float)sum;
  }
}

// Launch: hipErrorInvalidValue when no instance exists for the combination (the caller keeps the two launches).
hipError_t dis_fb3_launch(const FbArgs& f, int inact, bool xgn, int xsrc, long grid, hipStream_t stream) {
  static bool attr_set[5] = {};
  auto launch = [&](auto kern, int slot) { return fbc_launch<F3Cfg>(kern, attr_set[slot], "conv_bwd_fused_bf16x3_kernel<32>", f, grid, stream); };
  constexpr int S = DIS_ACT_SELU;
  if ((inact != 0 && inact != S) || xsrc != 0) return hipErrorInvalidValue;
  if (xgn) return (inact || f.c.accum) ? hipErrorInvalidValue : launch(conv_bwd_fused_bf16x3_kernel<0, false, true>, 0);
  if (f.c.accum) return inact ? launch(conv_bwd_fused_bf16x3_kernel<S, true, false>, 1) : launch(conv_bwd_fused_bf16x3_kernel<0, true, false>, 2);
  return inact ? launch(conv_bwd_fused_bf16x3_kernel<S, false, false>, 3) : launch(conv_bwd_fused_bf16x3_kernel<0, false, false>, 4);
}
