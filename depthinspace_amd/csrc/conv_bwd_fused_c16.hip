// Input gradient AND weight gradient of a 3x3 stride-1 pad-1 convolution 16 -> 16 in ONE launch: the sibling of conv_bwd_fused.hip
// (32 -> 32), same idea, same arithmetic (profiles/r7_bwd_fused_c16.md).  The mixed shapes (16, 32) and (32, 16) have no kernel here and
// keep their two launches.  CG = 16 channels of gy (the conv's output), CX = 16 channels of x and gx (the conv's input):
//     gx[q][ci]        = sum_tap sum_co gy[q + 1 - tap][co] W[co][ci][tap]          (contraction over the CG channels of gy, per tile)
//     dW[tap][ci][co]  = sum_q'  x[q'][ci] gy[q' + 1 - tap][co]                     (contraction over the pixels q' a tile OWNS)
// The 18 x 18 gy halo a tile of the input gradient stages in LDS (two fp16 planes, per-tile scale) feeds both products; x and gy are
// read once.  gx is BIT-identical to conv_f16x2_kernel<16, 16>'s: the same split, the same per-tile power-of-two scale, the same
// k-steps in the same order - the five tap-PAIR k-steps of F2Cfg (k-step ks holds taps 2 ks and 2 ks + 1 in the k-slots of lane
// groups 0, 1 and 2, 3; the tenth slot is zero).
//
// What differs from the 32 -> 32 kernel:
//   * dW is 9 accumulator tiles in all.  There is no channel block to hand to each wave, so the PIXELS are split: wave w forms every
//     tile over the tile rows 4 w .. 4 w + 3 it owns in the input gradient as well (two k-steps of 32 pixels), and the four waves'
//     accumulators are added once per workgroup through LDS, in a fixed order, before the slab is written.  The running dW exponent
//     S (workgroup-uniform, leave-the-loop rescale) is the 32 -> 32 kernel's.
//   * 66 KB of LDS and 256 registers: TWO workgroups per CU (__launch_bounds__(256, 2)), i.e. two waves per SIMD, so one workgroup's
//     staging and epilogue issue under the other's products; the grid is 2 x #CUs and the channel sums take 2 x #CUs slots per sample
//     (FbArgs::c.ab_slots is given by the caller).
#include "conv_bwd_fused_common.h"

#define FC_TR 16
#define FC_TC 16
// (CG = CX = 16 makes NT = NA = NB = 1: the loops and index arithmetic over channel blocks below run once by construction.  They
//  are the text the kernel was compiled from when it was written over both channel counts, kept so that its device code stays what
//  was tested and measured.)
struct FcCfg {
  static constexpr int CG = 16, CX = 16;   // channels of gy (the conv's output) / of x and gx (the conv's input)
  static constexpr int IR = FC_TR + 2, IC = FC_TC + 2, CVG = CG / 4, NP = 2;
  static constexpr int PSG = 48, PSX = 48;   // LDS pixel strides (F2Cfg::PS)
  static constexpr int NT = CX / 16, KS = 5;   // k-steps of the input gradient: tap pairs
  static constexpr int NA = CX / 16, NB = CG / 16, NACC = 9 * NA * NB;        // dW accumulator tiles per wave: [tap][ci block][co block]
  static constexpr int NW = 4, NTHR = 64 * NW, MT = FC_TR / NW;
  static constexpr int RPR = NTHR / (16 * CVG), NMAIN = (IR + RPR - 1) / RPR;   // halo rows a round of items covers (columns 0 .. 15), such rounds
  static constexpr int NEDGE = (IR * 2 * CVG + NTHR - 1) / NTHR;              // rounds for the two right columns
  static constexpr int W_U16 = KS * NP * 4 * CX * 8, X_U16 = IR * IC * PSG, XT_U16 = FC_TR * FC_TC * PSX;
  static constexpr int NLOAD = NMAIN + NEDGE, NPIECE = MT * NT;
  static constexpr int SMALL_U16 = 32 + 64 + NW * 2 * CX * 2 + CG + 8;   // red (8 doubles), maxima [parity][gy | x][wave], abw [wave][2 CX] floats, write pad
  static constexpr int LDS_BYTES = (W_U16 + X_U16 + XT_U16 + SMALL_U16) * 2;
  static constexpr int WPC = 2;                                               // workgroups per CU
  static constexpr int PART = 9 * CX * CG;                                    // floats of a weight-gradient slab
};

// INACT / INCOEF / ACCUM / EPIAB / EPIACT / XSRC / XGN / GST: conv_bwd_fused_kernel's forms (see there).
template <int INACT, bool INCOEF, bool ACCUM, bool EPIAB, int EPIACT, int XSRC, bool XGN, bool GST>
__global__ __launch_bounds__(256, FcCfg::WPC) void conv_bwd_fused_c16_kernel(FbArgs fa_) {
  using K = FcCfg;
  const ConvArgs& a = fa_.c;
  constexpr int CG = K::CG, CX = K::CX;
  constexpr int IC = K::IC, PSG = K::PSG, PSX = K::PSX, NT = K::NT, KS = K::KS, NLOAD = K::NLOAD, NPIECE = K::NPIECE, CVG = K::CVG;
  constexpr int NP = K::NP, MT = K::MT, NW = K::NW, NTHR = K::NTHR, NA = K::NA, NB = K::NB;
  constexpr bool IN2 = INACT != 0 || INCOEF;
  // LATE: the forms whose operand takes two loads per item AND whose epilogue holds operands of its own request the next tile's halo
  // only in the last dW sub-steps (behind the epilogue) and finish its items at the top of their own tile: 48 registers less where
  // the register file is full - the other workgroup of the CU covers the wait.  The others request it in D and finish it under W.
  constexpr bool LATE = INCOEF || (INACT != 0 && ACCUM);
  constexpr bool XSH = XSRC != 0;   // x IS one of the epilogue's operands: one register set and one fetch serve both
  static_assert(EPIACT == 0 || EPIAB, "activation gradient at the output: only with the channel sums");
  static_assert(XSRC == 0 || (XSRC == 1 && EPIAB) || (XSRC == 2 && EPIACT), "shared x operand");
  static_assert(!GST || INCOEF, "gpre store: only where the operand is formed on load");
  static_assert(K::LDS_BYTES * K::WPC <= 160 * 1024, "LDS budget");
  static_assert(CG * (CX * 9 + 1) * 4 <= K::XT_U16 * 2, "the weight prologue's fp32 scratch aliases the x tile");
  static_assert((NW - 1) * K::NACC * 256 * 4 <= (K::X_U16 + K::XT_U16) * 2, "the dW exchange aliases the halo and the x tile");
  static_assert((NTHR / CVG) * CG * 8 <= K::X_U16 * 2, "the bias exchange aliases the halo");
  extern __shared__ __attribute__((aligned(16))) unsigned short smem16[];
  unsigned short* wl = smem16;                              // weights, fragment order, two planes
  unsigned short* xh = smem16 + K::W_U16;                   // the gy halo of the current tile [18 x 18 pixels][plane][channel]
  unsigned short* xt = smem16 + K::W_U16 + K::X_U16;        // the x tile of the current tile  [16 x 16 pixels][plane][channel]
  unsigned short* small = smem16 + K::W_U16 + K::X_U16 + K::XT_U16;
  double* red = (double*)small;
  float* mxs = (float*)(small + 32);      // [parity][gy | x][wave]
  float* abw = (float*)(small + 96);      // EPIAB: [wave][2 CX]
  unsigned short* pad16 = small + 96 + NW * 2 * CX * 2 + CG;   // (idle threads of the last round write pad16 - CG and pad16)

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4, tq = li >> 2, tp = li & 3;
  const int tiles_x = (a.wv + FC_TC - 1) / FC_TC, tiles_y = (a.hv + FC_TR - 1) / FC_TR;
  int rank, per, t_lo, t_hi, d_tx, d_ty, d_n;   // this workgroup's tiles: t_lo + rank, + per, ... < t_hi
  fbc_tile_share(a.n, tiles_y, tiles_x, rank, per, t_lo, t_hi, d_tx, d_ty, d_n);

  // ---- halo items of this thread.  Items 0 .. NMAIN - 1 walk the halo's columns 0 .. 15 in bands of RPR rows: thread = (band row
  // rr, column, float4 vv), item it = halo pixel (RPR it + rr, column) - ONE lane-varying offset serves them all, an item adds a
  // constant (a per-item row / column kept across the tile loop is what made the first form of this kernel spill).  The last NEDGE
  // items are the halo's two right columns.  A wave's load is 1 KB of one image row.
  float4 pre[NLOAD], pre2[IN2 ? NLOAD : 1];
  constexpr int RPR = K::RPR, NMAIN = K::NMAIN;
  const int vvi = (int)threadIdx.x % CVG, colq = ((int)threadIdx.x / CVG) & 15, rr = (int)threadIdx.x / (16 * CVG);
  const int vv4 = vvi * 16;   // byte offset of this thread's 4 channels within a pixel
  auto item_rc = [&](int it, int& r, int& c) __attribute__((always_inline)) {
    if (it < NMAIN) {
      r = RPR * it + rr;
      c = colq;
    } else {
      const int idx = (int)threadIdx.x + (it - NMAIN) * NTHR;
      r = idx / (2 * CVG);
      c = 16 + ((idx / CVG) & 1);
    }
    if (it >= NMAIN || RPR * it + RPR > K::IR) c = r < K::IR ? c : 0x40000000;   // (past the end of the halo: never in range)
  };
  auto item_own = [&](int it) -> bool {
    int r, c;
    item_rc(it, r, c);
    return r >= 1 && r <= FC_TR && c >= 1 && c <= FC_TC;
  };
  const unsigned x_bytes = (unsigned)a.hin * a.win * (CG * 4u), y_bytes = (unsigned)a.hf * a.wf * (CX * 4u);
  struct Pf {
    const float* x;
    unsigned bytes;
    int iy0, ix0, off0;
  };
  auto pf_make = [&](int n, int ty, int tx, bool live) -> Pf {
    Pf f;
    f.iy0 = ty * FC_TR - 1;
    f.ix0 = tx * FC_TC - 1;
    f.off0 = (f.iy0 * a.win + f.ix0) * (CG * 4);
    f.x = a.x + (long)n * a.hin * a.win * CG;
    f.bytes = live ? x_bytes : 0u;
    return f;
  };
  auto item_off = [&](const Pf& f, int it) -> unsigned {
    int r_, c_;
    item_rc(it, r_, c_);
    const int ix = f.ix0 + c_;
    return (unsigned)ix < (unsigned)a.win ? (unsigned)(f.off0 + (r_ * a.win + c_) * (CG * 4) + vv4) : BX_OOB;
  };
  auto pf_issue = [&](const Pf& f, int it) {
    const unsigned off = item_off(f, it);
    pre[it] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(f.x, f.bytes), off, 0, 0));
    if (IN2)
      pre2[it] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(a.xact + (f.x - a.x), f.bytes), off, 0, 0));
  };
  float4 cf_k1 = make_float4(0.f, 0.f, 0.f, 0.f);
  float cf_kx = 0.f, cf_k0 = 0.f;
  int cf_n = -1;
  // bias gradient: this thread's 4 channels over the pixels its tiles own.  fp64: a thread adds up to ~1e3 values per launch and the
  // result is held to the error of the separate weight-gradient launch, which is a few fp32 roundings of the largest entry
  double bsum[4] = {0.0, 0.0, 0.0, 0.0};
  auto prep_cf = [&](int n_) {
    if (INCOEF && n_ != cf_n) {
      cf_n = n_;
      const float* cf = a.gnb_coef + (long)n_ * (CG + 2);
      cf_k1 = *(const float4*)(cf + vvi * 4);
      cf_kx = cf[CG];
      cf_k0 = cf[CG + 1];
    }
  };
  // final fp32 values of a tile's halo items (in place) and this lane's largest magnitude; the NEXT tile's items are finished under
  // the dW products of the current one (the first tile's in the prologue)
  auto prep_item = [&](const Pf& f, int it, float& m) __attribute__((always_inline)) {
    float4 v = pre[it];
    if (INCOEF) {   // (gn_apply_coef_kernel's arithmetic, bit for bit; padding: g = q = 0 would give k0, which must not be staged)
      const float4 q = pre2[it];
      const unsigned off = item_off(f, it);
      v.x = __builtin_fmaf(v.x, cf_k1.x, __builtin_fmaf(q.x, cf_kx, cf_k0));
      v.y = __builtin_fmaf(v.y, cf_k1.y, __builtin_fmaf(q.y, cf_kx, cf_k0));
      v.z = __builtin_fmaf(v.z, cf_k1.z, __builtin_fmaf(q.z, cf_kx, cf_k0));
      v.w = __builtin_fmaf(v.w, cf_k1.w, __builtin_fmaf(q.w, cf_kx, cf_k0));
      if (INACT) {
        v.x *= act_grad_from_out(q.x, INACT), v.y *= act_grad_from_out(q.y, INACT);
        v.z *= act_grad_from_out(q.z, INACT), v.w *= act_grad_from_out(q.w, INACT);
      }
      {
        const bool inside = off < f.bytes;
        v = inside ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (GST) {
        const u32x4 sv = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(sv, bx_rsrc(a.gnb_out + (f.x - a.x), f.bytes), item_own(it) ? off : BX_OOB, 0, 0);
      }
    } else if (INACT) {
      const float4 q = pre2[it];
      v.x *= act_grad_from_out(q.x, INACT), v.y *= act_grad_from_out(q.y, INACT);
      v.z *= act_grad_from_out(q.z, INACT), v.w *= act_grad_from_out(q.w, INACT);
    }
    pre[it] = v;
    {   // (bias gradient: the pixels this tile owns; a select, not a branch)
      const bool own = item_own(it);
      bsum[0] += (double)(own ? v.x : 0.f), bsum[1] += (double)(own ? v.y : 0.f);
      bsum[2] += (double)(own ? v.z : 0.f), bsum[3] += (double)(own ? v.w : 0.f);
    }
    m = __builtin_fmaxf(__builtin_fmaxf(m, fabsf(v.x)), fabsf(v.y));
    m = __builtin_fmaxf(__builtin_fmaxf(m, fabsf(v.z)), fabsf(v.w));
  };
  auto stage_item = [&](int it, float sc) __attribute__((always_inline)) {
    const float4 v = pre[it];
    unsigned a1, a2, b1, b2;
    f2_split_pair_scaled(v.x, v.y, sc, a1, a2);
    f2_split_pair_scaled(v.z, v.w, sc, b1, b2);
    int r_, c_;
    item_rc(it, r_, c_);
    unsigned short* p = xh + (r_ * IC + c_) * PSG + vvi * 4;
    if (it >= NMAIN || RPR * it + RPR > K::IR) p = r_ < K::IR ? p : pad16 - CG;
    *(uint2*)(p) = make_uint2(a1, b1);
    *(uint2*)(p + CG) = make_uint2(a2, b2);
  };

  int tile = t_lo + rank;
  int cn = 0, cty = 0, ctx = 0;
  auto advance = [&](int& n_, int& ty_, int& tx_) { fbc_advance(n_, ty_, tx_, d_n, d_ty, d_tx, tiles_y, tiles_x); };

  // ---- centre operands: this lane's pieces (row MT wave + mt, column li, channels 16 nt + 4 lg ..) of x (fetched one tile ahead) and
  // of the epilogue's operands - gx so far (ACCUM), the GroupNorm input of the channel sums (EPIAB), the activation output (EPIACT)
  const int yrow = a.wf * (CX * 4);
  const int y_lane = ((wave * MT * a.wf + li) * CX + lg * 4) * 4;
  float4 cxw[NPIECE], cy[ACCUM ? NPIECE : 1], cab[EPIAB && XSRC != 1 ? NPIECE : 1], cact[EPIACT && XSRC != 2 ? NPIECE : 1];
  const float* wx_base = XSRC == 1 ? a.ab_x : (XSRC == 2 ? a.ab_act_y : fa_.wx);
  auto centre_off = [&](int ty, int tx, unsigned (&off)[MT]) {
    const int vy0 = ty * FC_TR + wave * MT, vx0 = tx * FC_TC + li;
    const int t0 = (ty * FC_TR * a.wf + tx * FC_TC) * (CX * 4) + y_lane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) off[mt] = (vx0 < a.wv && vy0 + mt < a.hv) ? (unsigned)(t0 + mt * yrow) : BX_OOB;
  };
  auto x_issue = [&](int n, int ty, int tx, bool live, int i0 = 0, int i1 = FcCfg::NPIECE) __attribute__((always_inline)) {
    unsigned off[MT];
    centre_off(ty, tx, off);
    const long sb = (long)n * a.hf * a.wf * CX;
    const unsigned bytes = live ? y_bytes : 0u;
#pragma unroll
    for (int i = 0; i < NPIECE; ++i)
      if (i >= i0 && i < i1)
        cxw[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(wx_base + sb, bytes), off[i / NT] + (i % NT) * 64, 0, 0));
  };
  auto epi_issue = [&](int n, const unsigned (&off)[MT]) {
    const long sb = (long)n * a.hf * a.wf * CX;
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const unsigned o = off[i / NT] + (i % NT) * 64;
      if (ACCUM) cy[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(a.y + sb, y_bytes), o, 0, 0));
      if (EPIAB && XSRC != 1) cab[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(a.ab_x + sb, y_bytes), o, 0, 0));
      if (EPIACT && XSRC != 2) cact[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(bx_rsrc(a.ab_act_y + sb, y_bytes), o, 0, 0));
    }
  };

  Pf pfc = pf_make(0, 0, 0, false);   // the current tile's halo (its items are in `pre` when an iteration starts)
  if (tile < t_hi) {
    ctx = tile % tiles_x, cty = (tile / tiles_x) % tiles_y, cn = tile / (tiles_x * tiles_y);
    pfc = pf_make(cn, cty, ctx, true);
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) pf_issue(pfc, it);
    x_issue(cn, cty, ctx, true);
  }

  // ---- weights: OIHW fp32 -> scaled fp16 planes in fragment order (conv_f16x2_kernel's prologue with 4 waves; the fp32 copy sits in
  // the x tile, which is first written after the first barrier of the tile loop)
  int sw_e = 0;
  {
    float* ws = (float*)xt;
    float* wmx = (float*)(red + 4);
    const int row = a.w_i * 9;
    const unsigned wbytes = (unsigned)((a.w_o - 1) * a.w_rs + row) * 4u;
    float m = 0.f;
    {
      constexpr int RR = CG / NW, JJ = (CX * 9 + 63) / 64;
      float v[RR][JJ];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr)
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
          const int r = wave + NW * rr, j = lane + 64 * jj;
          const unsigned off = (r < a.w_o && j < row) ? (unsigned)(r * a.w_rs + j) * 4u : BX_OOB;
          v[rr][jj] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bx_rsrc(a.w, wbytes), off, 0, 0));
        }
#pragma unroll
      for (int rr = 0; rr < RR; ++rr)
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
          const int r = wave + NW * rr, j = lane + 64 * jj;
          if (r < a.w_o && j < row) ws[r * (row + 1) + j] = v[rr][jj];
          m = fmaxf(m, fabsf(v[rr][jj]));
        }
    }
    m = f2_wave_max(m);
    if (lane == 0) wmx[wave] = m;
    if (threadIdx.x == 0) *(unsigned*)(red + 3) = 0u;   // (ab_flush's arrival counter)
    __syncthreads();
    const float4 m0 = *(const float4*)(wmx);
    sw_e = f2_scale_exp(fmaxf(fmaxf(m0.x, m0.y), fmaxf(m0.z, m0.w)));
    const float sw = __builtin_ldexpf(1.f, sw_e);
    for (int u = threadIdx.x; u < KS * 4 * CX; u += NTHR) {
      const int co = u % CX, g = (u / CX) & 3, ks = u / (4 * CX);
      unsigned pl[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v0 = fbc_weight<CG>(ws, row + 1, a.w_o, a.w_i, ks, g, 2 * j, co);
        const float v1 = fbc_weight<CG>(ws, row + 1, a.w_o, a.w_i, ks, g, 2 * j + 1, co);
        f2_split_pair(v0 * sw, v1 * sw, pl[0][j], pl[1][j]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
        *(uint4*)(wl + (((ks * NP + p) * 4 + g) * CX + co) * 8) = make_uint4(pl[p][0], pl[p][1], pl[p][2], pl[p][3]);
    }
    // (no barrier here: barrier A of the first tile separates the last read of `ws` from the first write of the x tile, barrier B
    //  publishes the weight planes)
  }

  float mg_lane = 0.f;   // this lane's largest halo magnitude of the tile that comes next (formed one tile ahead, see prep_item)
  if (!LATE && tile < t_hi) {
    prep_cf(cn);
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) prep_item(pfc, it, mg_lane);
  }
  f32x4 accw[K::NACC];   // dW over this wave's pixels: [(tap * NA + ci block) * NB + co block]
#pragma unroll
  for (int j = 0; j < K::NACC; ++j) accw[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float sA[NT][4], sB[NT][4];
  int ab_n = -1;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[nt][r] = sB[nt][r] = 0.f;
  // XGN: the affine map of the GroupNorm in front of the conv, for this lane's channels, per sample
  float4 xg_sc[XGN ? NT : 1], xg_sh[XGN ? NT : 1];
  int xg_n = -1;
#pragma unroll
  for (int nt = 0; nt < (XGN ? NT : 1); ++nt) xg_sc[nt] = xg_sh[nt] = make_float4(0.f, 0.f, 0.f, 0.f);

  // EPIAB: a sample's channel sums leave the workgroup (conv_f16x2_kernel's ab_flush with 4 waves)
  auto ab_flush = [&]() {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float va = sA[nt][r], vb = sB[nt][r];
        fbc_row_sum2(va, vb);
        if (li == 0) {
          abw[wave * 2 * CX + nt * 16 + lg * 4 + r] = va;
          abw[wave * 2 * CX + CX + nt * 16 + lg * 4 + r] = vb;
        }
        sA[nt][r] = 0.f;
        sB[nt][r] = 0.f;
      }
    unsigned arrived = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) arrived = __hip_atomic_fetch_add((unsigned*)(red + 3), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (arrived == NW - 1) {
      if (lane < 2 * CX) {
        double t = 0.0;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) t += (double)abw[wv * 2 * CX + lane];
        a.ab_out[((long)ab_n * a.ab_slots + blockIdx.x) * (2 * CX) + lane] = t;
      }
      if (lane == 0) *(unsigned*)(red + 3) = 0u;
    }
  };

  using PO = FbcOrder2;   // the three products of a k-step

  // ---- one tile: TOP (maxima | barrier A | exponents | halo and x tile split and staged | barrier B), D (the input gradient's
  // products; the next tile's loads ride in its k-steps), W (its epilogue + this wave's dW products over its four tile rows).
  unsigned cur_off[MT];
  float gmax = 0.f, xmax = 0.f;
  int sx_e = 0, ex_e = 0, S_w = 120, parity = 0;
  auto xval = [&](int i) -> float4 {   // the x value the products see: GroupNorm applied (XGN), pixels past the map zero
    float4 v = cxw[i];
    if (XGN) {
      const int nt = i % NT;
      const bool ok = cur_off[i / NT] != BX_OOB;
      v.x = v.x * xg_sc[nt].x + xg_sh[nt].x, v.y = v.y * xg_sc[nt].y + xg_sh[nt].y;
      v.z = v.z * xg_sc[nt].z + xg_sh[nt].z, v.w = v.w * xg_sc[nt].w + xg_sh[nt].w;
      v = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return v;
  };
  auto top_a = [&]() __attribute__((always_inline)) {   // up to barrier A and the exponents (not repeated when a pass restarts at this tile)
    centre_off(cty, ctx, cur_off);
    if (EPIAB && cn != ab_n) {   // (two flushes are always separated by a tile's barriers)
      if (ab_n >= 0) ab_flush();
      ab_n = cn;
    }
    if (XGN && cn != xg_n) {
      xg_n = cn;
      fbc_gn_affine<NT>(fa_, cn, (double)a.hf * a.wf * CX, lg, xg_sc, xg_sh);
    }
    if (LATE) {
      prep_cf(cn);
      mg_lane = 0.f;
#pragma unroll
      for (int it = 0; it < NLOAD; ++it) prep_item(pfc, it, mg_lane);
    }
    const float mg = f2_wave_max(mg_lane);
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const float4 v = xval(i);
      mx = __builtin_fmaxf(__builtin_fmaxf(mx, fabsf(v.x)), fabsf(v.y));
      mx = __builtin_fmaxf(__builtin_fmaxf(mx, fabsf(v.z)), fabsf(v.w));
    }
    mx = f2_wave_max(mx);
    if (lane == 0) {
      mxs[parity * 2 * NW + wave] = mg;
      mxs[parity * 2 * NW + NW + wave] = mx;
    }
    // barrier A: every wave has finished the previous tile (halo and x tile may be overwritten), the maxima are visible
    __syncthreads();
    const float4 m0 = *(const float4*)(mxs + parity * 2 * NW), m1 = *(const float4*)(mxs + parity * 2 * NW + NW);
    parity ^= 1;
    gmax = fmaxf(fmaxf(m0.x, m0.y), fmaxf(m0.z, m0.w));
    xmax = fmaxf(fmaxf(m1.x, m1.y), fmaxf(m1.z, m1.w));
    sx_e = f2_scale_exp(gmax);
    ex_e = f2_scale_exp(xmax);
  };
  f32x4 acc[MT][NT];
  auto rest = [&]() __attribute__((always_inline)) {
    // ---- staging: the halo with its own per-tile scale, x with 2^(S - sx_e) (a term of dW carries 2^S; where the halo or the x tile
    // is all zero the exponent does not matter)
    {
      const float sc = __builtin_ldexpf(1.f, sx_e);
#pragma unroll
      for (int it = 0; it < NLOAD; ++it) stage_item(it, sc);
      const int es = S_w - sx_e < ex_e ? S_w - sx_e : ex_e;
      const float scx = __builtin_ldexpf(1.f, es);
#pragma unroll
      for (int i = 0; i < NPIECE; ++i) {
        const float4 va = xval(i);
        unsigned a1, a2, b1, b2;
        f2_split_pair_scaled(va.x, va.y, scx, a1, a2);
        f2_split_pair_scaled(va.z, va.w, scx, b1, b2);
        unsigned short* p = xt + ((wave * MT + i / NT) * FC_TC + li) * PSX + (i % NT) * 16 + lg * 4;
        *(uint2*)(p) = make_uint2(a1, b1);
        *(uint2*)(p + CX) = make_uint2(a2, b2);
      }
    }
    // (this tile's epilogue operands, the next tile's halo and x pieces are requested in D's k-steps)
    int n1 = cn, ty1 = cty, tx1 = ctx;
    advance(n1, ty1, tx1);
    const bool live1 = tile + per < t_hi;
    const Pf pfn = pf_make(n1, ty1, tx1, live1);
    if (!LATE) prep_cf(n1);   // (the current tile's items are final: the coefficients may move on to the next tile's sample)
    float mg_next = 0.f;
    // barrier B: halo, x tile (and, first tile, the weight planes) are complete
    __syncthreads();

    // ---------------- input gradient: KS k-steps x (MT rows x NT channel blocks) x 3 products, conv_f16x2_kernel's order.
    // k-step ks multiplies halo pixel (row + ky, column + kx): lane groups 0, 1 take tap 2 ks, groups 2, 3 tap 2 ks + 1 (the tenth
    // slot's weights are zero; its pixels are tap 8's).
    {
      const int xa_lane = (wave * MT * IC + li) * PSG + (lg & 1) * 8;
      const bool hi_tap = (lg >> 1) != 0;
      // ONE fragment set: with two workgroups per CU the other workgroup's wave covers the latency of these reads, and the registers
      // of a second set are what the epilogue forms lack (a spilling instance loses its prefetch to scratch waits).  The reads are
      // issued in the order the products need them (pixel plane 1 x weight plane 0 first).
      s16x8 fa[NP][MT], fw[NP][NT];
      auto load_frag = [&](int ks) __attribute__((always_inline)) {
        const int t0 = 2 * ks, t1 = 2 * ks + 1 > 8 ? 8 : 2 * ks + 1;
        const int xoff = hi_tap ? ((t1 / 3) * IC + t1 % 3) * PSG : ((t0 / 3) * IC + t0 % 3) * PSG;
        const int wt = ks;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
          const int pw = pp, pa = NP - 1 - pp;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) fw[pw][nt] = *(const s16x8*)(wl + (((wt * NP + pw) * 4 + lg) * CX + nt * 16 + li) * 8);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) fa[pa][mt] = *(const s16x8*)(xh + xa_lane + xoff + mt * IC * PSG + pa * CG);
        }
      };
      fbc_static_for<0, KS>([&](auto ksc) __attribute__((always_inline)) {
        constexpr int ks = decltype(ksc)::value;
        load_frag(ks);
        // the next tile's loads that ride in this k-step (their registers were emptied by the staging above)
        constexpr int LKS = 4;
#pragma unroll
        for (int it = 0; it < NLOAD; ++it)
          if (!LATE && it * LKS / NLOAD == ks) pf_issue(pfn, it);
        if (ks == KS - 1) {   // (the epilogue's operands and the next tile's x: late, they only wait in registers)
          epi_issue(cn, cur_off);
          if (!XSH) x_issue(n1, ty1, tx1, live1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                  __builtin_bit_cast(f16x8_t, fw[PO::PB[q]][nt]), __builtin_bit_cast(f16x8_t, fa[PO::PA[q]][mt]),
                  (ks == 0 && q == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[mt][nt], 0, 0, 0);   // (the first product starts from a zero literal)
        __builtin_amdgcn_sched_barrier(0);
      });
    }

    // ---------------- epilogue of the input gradient (conv_f16x2_kernel's arithmetic, undeferred): piece i rides under the dW products
    const float* cur_y = a.y + (long)cn * a.hf * a.wf * CX;
    const float desc = __builtin_ldexpf(1.f, -(sx_e + sw_e));
    auto epi_piece = [&](int i) __attribute__((always_inline)) {
      const int mt = i / NT, nt = i % NT;
      const float livef = cur_off[mt] != BX_OOB ? 1.f : 0.f;
      const f32x4 o = fbc_epi_value<ACCUM, EPIACT>(acc[mt][nt], desc, cy[ACCUM ? i : 0], XSRC == 2 ? cxw[i] : cact[EPIACT && XSRC != 2 ? i : 0]);
      const u32x4 ov = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
      __builtin_amdgcn_raw_buffer_store_b128(ov, bx_rsrc(cur_y, y_bytes), cur_off[mt] + nt * 64, 0, 0);
      if (EPIAB) {
        const float4 xv = XSRC == 1 ? cxw[i] : cab[EPIAB && XSRC != 1 ? i : 0];
        fbc_ab_add(o, livef, xv, sA[nt], sB[nt]);
      }
      if (XSH) x_issue(n1, ty1, tx1, live1, i, i + 1);   // (the shared register is free again: the next tile's piece)
    };

    // ---------------- weight gradient: this wave's 9 accumulator tiles over the 64 pixels of its tile rows 4 w .. 4 w + 3: two
    // k-steps of 32 pixels (tile rows 4 w + 2 s, + 1), per k-step the x^T fragments (planes) against the gy fragments of the 9 tap
    // shifts - centre pixel (r', c') meets the halo pixel (r' + 2 - ky, c' + 2 - kx), so tap row ky of k-step s reads the halo row pair
    // (4 w + 2 s + 2 - ky, + 1).  One fragment set per tap (see D); the input gradient's epilogue and the next tile's halo
    // arithmetic ride in the six sub-steps.
    {
      s16x8 fx[NA][NP];        // x^T: [ci block][plane]
      const int hr0 = wave * MT;
      auto load_x = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int ab = 0; ab < NA; ++ab) {
          const unsigned short* xq = xt + ((hr0 + 2 * s) * FC_TC + 4 * lg + tq) * PSX + ab * 16 + tp * 4;
#pragma unroll
          for (int p = 0; p < NP; ++p) fx[ab][p] = fbc_tr_read8(xq + p * CX, xq + FC_TC * PSX + p * CX);
        }
      };
      // tap (ky, kx) of k-step s: halo rows row0, row0 + 1 shifted by 2 - kx columns; one fragment set per tap
      auto mm_tap = [&](int row0, int ky, int kx) __attribute__((always_inline)) {
        s16x8 G[NB][NP];
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) {
          const unsigned short* gq = xh + (row0 * IC + (4 * lg + tq) + 2 - kx) * PSG + bb * 16 + tp * 4;
#pragma unroll
          for (int p = 0; p < NP; ++p) G[bb][p] = fbc_tr_read8(gq + p * CG, gq + IC * PSG + p * CG);
        }
#pragma unroll
        for (int ab = 0; ab < NA; ++ab)
#pragma unroll
          for (int bb = 0; bb < NB; ++bb)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              const int j = ((ky * 3 + kx) * NA + ab) * NB + bb;
              accw[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, fx[ab][PO::PA[q]]),
                                                               __builtin_bit_cast(f16x8_t, G[bb][PO::PB[q]]), accw[j], 0, 0, 0);
            }
      };
      auto ride = [&](int slot) __attribute__((always_inline)) {   // slot 0 .. 5
#pragma unroll
        for (int i = 0; i < NPIECE; ++i)
          if (i * (LATE ? 4 : 6) / NPIECE == slot) epi_piece(i);
#pragma unroll
        for (int it = 0; it < NLOAD; ++it) {
          if (!LATE && it * 6 / NLOAD == slot) prep_item(pfn, it, mg_next);   // the next tile's halo items (requested in D) become final
          if (LATE && 4 + it * 2 / NLOAD == slot) pf_issue(pfn, it);          // ... or are requested now, behind the epilogue
        }
      };
      fbc_static_for<0, 6>([&](auto sc_) __attribute__((always_inline)) {
        constexpr int slot = decltype(sc_)::value, s = slot / 3, ky = slot % 3;
        if (ky == 0) load_x(s);
        ride(slot);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) mm_tap(hr0 + 2 * s + 2 - ky, ky, kx);
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    // the next tile becomes the current one
    cn = n1, cty = ty1, ctx = tx1;
    tile += per;
    pfc = pfn;
    if (!LATE) mg_lane = mg_next;
  };

  int flushed = 0;
  bool resume = false;
  float* out = fa_.part + (long)blockIdx.x * K::PART;
  // the workgroup's dW leaves for its slab: waves 1 .. 3 hand their accumulators to wave 0 through LDS (the halo and the x tile, which
  // nobody reads between the barriers below), wave 0 adds them in wave order, scales by 2^-S and writes (or adds to what an earlier
  // pass left).  Element (tile j, register r) of lane (lg, li) is dW[tap][16 ab + 4 lg + r][16 bb + li].
  auto slab_write = [&](bool add) {
    float* ex = (float*)xh;
    __syncthreads();   // (every wave has left the products that read the halo and the x tile)
    if (wave > 0) {
#pragma unroll
      for (int j = 0; j < K::NACC; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) ex[(((wave - 1) * K::NACC + j) * 4 + r) * 64 + lane] = accw[j][r];
    }
    __syncthreads();
    if (wave == 0) {
      const float dsc = __builtin_ldexpf(1.f, -S_w);
      const __amdgpu_buffer_rsrc_t orsrc = bx_rsrc(out, K::PART * 4u);
      // (one lane-varying offset, formed here from a thread index the compiler cannot tie to the tile loop's - kept across the loop
      //  such offsets were spilled; an element's constant part travels in the scalar offset)
      int tl = (int)threadIdx.x;
      asm volatile("" : "+v"(tl));
      const unsigned o_lane = (unsigned)((((tl >> 4) & 3) * 4 * CG + (tl & 15)) * 4);
#pragma unroll
      for (int j = 0; j < K::NACC; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = accw[j][r];
#pragma unroll
          for (int wv = 0; wv < NW - 1; ++wv) v += ex[((wv * K::NACC + j) * 4 + r) * 64 + (tl & 63)];
          const int tap = j / (NA * NB), ab = (j / NB) % NA, bb = j % NB;
          const int oc = (((tap * CX + ab * 16 + r) * CG) + bb * 16) * 4;
          v *= dsc;
          if (add) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(orsrc, o_lane, oc, 0));
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orsrc, o_lane, oc, 0);
        }
    }
    __syncthreads();   // (the exchange has been read: the staging of the next pass may overwrite it)
  };
  for (;;) {   // one pass per dW exponent: almost always exactly one
#pragma unroll
    for (int j = 0; j < K::NACC; ++j) accw[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    S_w = 120;
    bool s_set = false, need = false;
    while (tile < t_hi) {
      if (!resume) top_a();
      resume = false;
      const bool adds = xmax > 0.f && gmax > 0.f;   // (workgroup-uniform) this tile has something to add to dW
      if (s_set && adds && ex_e + sx_e < S_w) {     // (rare) a larger product magnitude than the exponent allows: the accumulators leave first
        need = true;
        break;
      }
      if (!s_set && adds) {   // the first tile with something to add sets the exponent, FBC_SMARGIN bits of headroom
        S_w = ex_e + sx_e - FBC_SMARGIN;
        s_set = true;
      }
      rest();
    }
    if (!need) break;
    slab_write(flushed != 0);
    flushed = 1;
    resume = true;
  }

  // ---------------- the workgroup's results leave: dW slab, channel sums, bias partials
  slab_write(flushed != 0);
  if (EPIAB) {
    __syncthreads();   // (a flush inside the last iteration and the final one must not overlap: see conv_f16x2_kernel)
    if (ab_n >= 0) ab_flush();
  }
  if (fa_.bpart) {
    __syncthreads();   // (every wave is done with the halo: the exchange below aliases it)
    double* bred = (double*)xh;
    const int vv = threadIdx.x % CVG, row = threadIdx.x / CVG;
#pragma unroll
    for (int j = 0; j < 4; ++j) bred[row * CG + vv * 4 + j] = bsum[j];
    __syncthreads();
    if (threadIdx.x < CG) {
      double sum = 0.0;
      for (int r = 0; r < NTHR / CVG; ++r) sum += bred[r * CG + threadIdx.x];
      const float hi = (float)sum;   // (two floats per partial: [workgroup][CG] sums, then [workgroup][CG] remainders)
      fa_.bpart[(long)blockIdx.x * CG + threadIdx.x] = hi;
      fa_.bpart[((long)gridDim.x + blockIdx.x) * CG + threadIdx.x] = (float)(sum - (double)hi);
    }
  }
}

int dis_fc_wpc(int cg, int cx) { return (cg == FcCfg::CG && cx == FcCfg::CX) ? FcCfg::WPC : 0; }

// Launch (f.c.cx channels of gy, f.c.cy of x): hipErrorInvalidValue when no instance exists for the combination (the caller keeps the
// two launches).
hipError_t dis_fc_launch(const FbArgs& f, int inact, bool xgn, int xsrc, long grid, hipStream_t stream) {
  if (dis_fc_wpc(f.c.cx, f.c.cy) <= 0) return hipErrorInvalidValue;
  static bool attr_set[FBC_NFORMS] = {};
  return fbc_dispatch(f.c, inact, xgn, xsrc, [&](auto form) {
    using F = decltype(form);
    return fbc_launch<FcCfg>(conv_bwd_fused_c16_kernel<F::INACT, F::INCOEF, F::ACCUM, F::EPIAB, F::EPIACT, F::XSRC, F::XGN, F::GST>,
                             attr_set[F::SLOT], "conv_bwd_c16_fused_kernel<16,16>", f, grid, stream);
  });
}
