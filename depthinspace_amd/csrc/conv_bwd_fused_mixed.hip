// Input gradient AND weight gradient of a 3x3 stride-1 pad-1 convolution between 16 and 32 channels in ONE launch: the sibling of
// conv_bwd_fused_c16.hip (16 -> 16) for the pairs (cin, cout) = (16, 32) and (32, 16), same idea, same arithmetic
// (profiles/r10_bwd_fused_mixed.md).  CG channels of gy (the conv's output), CX channels of x and gx (the conv's input):
//     gx[q][ci]        = sum_tap sum_co gy[q + 1 - tap][co] W[co][ci][tap]          (contraction over the CG channels of gy, per tile)
//     dW[tap][ci][co]  = sum_q'  x[q'][ci] gy[q' + 1 - tap][co]                     (contraction over the pixels q' a tile OWNS)
// The 18 x 18 gy halo a tile of the input gradient stages in LDS (two fp16 planes, per-tile scale) feeds both products; x and gy are
// read once.  gx is BIT-identical to conv_f16x2_kernel<CG, CX>'s: the same 16 x 16 tile, the same split, the same per-tile
// power-of-two scale, the same k-steps in the same order - for CG = 16 the five tap-PAIR k-steps of F2Cfg (k-step ks holds taps 2 ks
// and 2 ks + 1 in the k-slots of lane groups 0, 1 and 2, 3; the tenth slot is zero), for CG = 32 the nine taps, kx outer.
//
// What differs from the 16 -> 16 kernel:
//   * dW is 18 accumulator tiles of 16 x 16 (9 taps x 2 channel blocks).  EIGHT waves: in the input gradient wave w owns the tile rows
//     2 w, 2 w + 1 (conv_f16x2_kernel's share); in the weight gradient wave w = 4 cb + pq forms the 9 tiles of channel block cb (of
//     gy for CG = 32, of x for CX = 32) over the pixel quarter pq (tile rows 4 pq .. 4 pq + 3: two k-steps of 32 pixels).  The four
//     quarters are added once per workgroup through LDS, in a fixed order, before the slab is written.  No float atomics.
//   * 93 - 95 KB of LDS: ONE 512-thread workgroup per CU, which is still two waves per SIMD - one wave's staging and epilogue issue
//     under the other's products.  The grid is #CUs and the channel sums take #CUs slots per sample.
//   * Only the forms the mixed layers of the step use exist (operand gy SELU'(y), not accumulating): the plain epilogue, and the
//     epilogue gx SELU'(x) with the channel sums of g and g x2, where x - the conv's input - is fetched once for both of its uses.
#include "conv_bwd_fused_common.h"

#define FM_TR 16
#define FM_TC 16
template <int CG_, int CX_>
struct FmCfg {
  static constexpr int CG = CG_, CX = CX_;   // channels of gy (the conv's output) / of x and gx (the conv's input)
  static_assert((CG == 16 && CX == 32) || (CG == 32 && CX == 16), "the mixed pairs");
  static constexpr int IR = FM_TR + 2, IC = FM_TC + 2, CVG = CG / 4, NP = 2;
  static constexpr int PSG = CG == 32 ? 80 : 48, PSX = CX == 32 ? 80 : 48;   // LDS pixel strides (F2Cfg::PS)
  static constexpr int NT = CX / 16, KS = CG == 32 ? 9 : 5;                  // k-steps of the input gradient: taps or tap pairs
  static constexpr int NW = 8, NTHR = 64 * NW, MT = FM_TR / NW;              // input gradient: MT tile rows per wave
  static constexpr int NQ = 4, QR = FM_TR / NQ, NACC = 9;                    // weight gradient: pixel quarters, their rows, tiles per wave
  static_assert(NW == NQ * (CG / 16) * (CX / 16) && QR == 4, "a wave per (channel block, pixel quarter)");
  static constexpr int RPR = NTHR / (16 * CVG), NMAIN = (IR + RPR - 1) / RPR;   // halo rows a round of items covers (columns 0 .. 15), such rounds
  static constexpr int NEDGE = (IR * 2 * CVG + NTHR - 1) / NTHR;              // rounds for the two right columns
  static constexpr int W_U16 = KS * NP * 4 * CX * 8, X_U16 = IR * IC * PSG, XT_U16 = FM_TR * FM_TC * PSX;
  static constexpr int NLOAD = NMAIN + NEDGE, NPIECE = MT * NT;
  static constexpr int SMALL_U16 = 32 + 64 + NW * 2 * CX * 2 + CG + 8;   // red (8 doubles), maxima [parity][gy | x][wave], abw [wave][2 CX] floats, write pad
  static constexpr int LDS_BYTES = (W_U16 + X_U16 + XT_U16 + SMALL_U16) * 2;
  static constexpr int WPC = 1;                                               // workgroups per CU
  static constexpr int PART = 9 * CX * CG;                                    // floats of a weight-gradient slab
};

// INACT / EPIAB / EPIACT / XSRC: conv_bwd_fused_kernel's flags of these names (see there); its INCOEF, ACCUM, XGN and GST are off.
template <int CG, int CX, int INACT, bool EPIAB, int EPIACT, int XSRC>
__global__ __launch_bounds__(512) void conv_bwd_fused_mixed_kernel(FbArgs fa_) {
  using K = FmCfg<CG, CX>;
  const ConvArgs& a = fa_.c;
  constexpr int IC = K::IC, PSG = K::PSG, PSX = K::PSX, NT = K::NT, KS = K::KS, NLOAD = K::NLOAD, NPIECE = K::NPIECE, CVG = K::CVG;
  constexpr int NP = K::NP, MT = K::MT, NW = K::NW, NTHR = K::NTHR, NQ = K::NQ, QR = K::QR;
  constexpr bool IN2 = INACT != 0;
  constexpr bool XSH = XSRC != 0;   // x IS one of the epilogue's operands: one register set and one fetch serve both
  static_assert(EPIACT == 0 || EPIAB, "activation gradient at the output: only with the channel sums");
  static_assert(XSRC == 0 || (XSRC == 1 && EPIAB) || (XSRC == 2 && EPIACT), "shared x operand");
  static_assert(K::LDS_BYTES * K::WPC <= 160 * 1024, "LDS budget");
  static_assert(CG * (CX * 9 + 1) * 4 <= K::XT_U16 * 2, "the weight prologue's fp32 scratch aliases the x tile");
  static_assert((NW - NW / NQ) * K::NACC * 256 * 4 <= (K::X_U16 + K::XT_U16) * 2, "the dW exchange aliases the halo and the x tile");
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
  const int tiles_x = (a.wv + FM_TC - 1) / FM_TC, tiles_y = (a.hv + FM_TR - 1) / FM_TR;
  int rank, per, t_lo, t_hi, d_tx, d_ty, d_n;   // this workgroup's tiles: t_lo + rank, + per, ... < t_hi
  fbc_tile_share(a.n, tiles_y, tiles_x, rank, per, t_lo, t_hi, d_tx, d_ty, d_n);

  // ---- halo items of this thread.  Items 0 .. NMAIN - 1 walk the halo's columns 0 .. 15 in bands of RPR rows: thread = (band row
  // rr, column, float4 vv), item it = halo pixel (RPR it + rr, column) - ONE lane-varying offset serves them all, an item adds a
  // constant.  The last NEDGE items are the halo's two right columns.
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
    return r >= 1 && r <= FM_TR && c >= 1 && c <= FM_TC;
  };
  const unsigned x_bytes = (unsigned)a.hin * a.win * (CG * 4u), y_bytes = (unsigned)a.hf * a.wf * (CX * 4u);
  struct Pf {
    const float* x;
    unsigned bytes;
    int iy0, ix0, off0;
  };
  auto pf_make = [&](int n, int ty, int tx, bool live) -> Pf {
    Pf f;
    f.iy0 = ty * FM_TR - 1;
    f.ix0 = tx * FM_TC - 1;
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
  // bias gradient: this thread's 4 channels over the pixels its tiles own.  fp64: a thread adds up to ~1e3 values per launch and the
  // result is held to the error of the separate weight-gradient launch, which is a few fp32 roundings of the largest entry
  double bsum[4] = {0.0, 0.0, 0.0, 0.0};
  // final fp32 values of a tile's halo items (in place) and this lane's largest magnitude; the NEXT tile's items are finished under
  // the dW products of the current one (the first tile's in the prologue)
  auto prep_item = [&](int it, float& m) __attribute__((always_inline)) {
    float4 v = pre[it];
    if (INACT) {
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
  // of the epilogue's operands - the GroupNorm input of the channel sums (EPIAB), the activation output (EPIACT)
  const int yrow = a.wf * (CX * 4);
  const int y_lane = ((wave * MT * a.wf + li) * CX + lg * 4) * 4;
  float4 cxw[NPIECE], cab[EPIAB && XSRC != 1 ? NPIECE : 1], cact[EPIACT && XSRC != 2 ? NPIECE : 1];
  const float* wx_base = XSRC == 1 ? a.ab_x : (XSRC == 2 ? a.ab_act_y : fa_.wx);
  auto centre_off = [&](int ty, int tx, unsigned (&off)[MT]) {
    const int vy0 = ty * FM_TR + wave * MT, vx0 = tx * FM_TC + li;
    const int t0 = (ty * FM_TR * a.wf + tx * FM_TC) * (CX * 4) + y_lane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) off[mt] = (vx0 < a.wv && vy0 + mt < a.hv) ? (unsigned)(t0 + mt * yrow) : BX_OOB;
  };
  auto x_issue = [&](int n, int ty, int tx, bool live, int i0 = 0, int i1 = FmCfg<CG, CX>::NPIECE) __attribute__((always_inline)) {
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

  // ---- weights: OIHW fp32 -> scaled fp16 planes in fragment order (conv_f16x2_kernel's prologue; the fp32 copy sits in the x tile,
  // which is first written after the first barrier of the tile loop)
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
    const float4 m0 = *(const float4*)(wmx), m1 = *(const float4*)(wmx + 4);
    sw_e = f2_scale_exp(fmaxf(fmaxf(fmaxf(m0.x, m0.y), fmaxf(m0.z, m0.w)), fmaxf(fmaxf(m1.x, m1.y), fmaxf(m1.z, m1.w))));
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
  if (tile < t_hi) {
#pragma unroll
    for (int it = 0; it < NLOAD; ++it) prep_item(it, mg_lane);
  }
  // dW of this wave: channel block cb over the pixel quarter pq, one tile per tap
  const int pq = wave % NQ, cb = wave / NQ;
  const int xcb = CX == 32 ? cb * 16 : 0, gcb = CG == 32 ? cb * 16 : 0;   // the block's first channel of x / of gy
  f32x4 accw[K::NACC];
#pragma unroll
  for (int j = 0; j < K::NACC; ++j) accw[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float sA[NT][4], sB[NT][4];
  int ab_n = -1;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[nt][r] = sB[nt][r] = 0.f;

  // EPIAB: a sample's channel sums leave the workgroup (conv_f16x2_kernel's ab_flush)
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
  // products; the next tile's loads ride in its k-steps), W (its epilogue + this wave's dW products over its pixel quarter).
  unsigned cur_off[MT];
  float gmax = 0.f, xmax = 0.f;
  int sx_e = 0, ex_e = 0, S_w = 120, parity = 0;
  auto top_a = [&]() __attribute__((always_inline)) {   // up to barrier A and the exponents (not repeated when a pass restarts at this tile)
    centre_off(cty, ctx, cur_off);
    if (EPIAB && cn != ab_n) {   // (two flushes are always separated by a tile's barriers)
      if (ab_n >= 0) ab_flush();
      ab_n = cn;
    }
    const float mg = f2_wave_max(mg_lane);
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const float4 v = cxw[i];
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
    gmax = 0.f, xmax = 0.f;
#pragma unroll
    for (int h = 0; h < NW / 4; ++h) {
      const float4 m0 = *(const float4*)(mxs + parity * 2 * NW + 4 * h), m1 = *(const float4*)(mxs + parity * 2 * NW + NW + 4 * h);
      gmax = fmaxf(gmax, fmaxf(fmaxf(m0.x, m0.y), fmaxf(m0.z, m0.w)));
      xmax = fmaxf(xmax, fmaxf(fmaxf(m1.x, m1.y), fmaxf(m1.z, m1.w)));
    }
    parity ^= 1;
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
        const float4 va = cxw[i];
        unsigned a1, a2, b1, b2;
        f2_split_pair_scaled(va.x, va.y, scx, a1, a2);
        f2_split_pair_scaled(va.z, va.w, scx, b1, b2);
        unsigned short* p = xt + ((wave * MT + i / NT) * FM_TC + li) * PSX + (i % NT) * 16 + lg * 4;
        *(uint2*)(p) = make_uint2(a1, b1);
        *(uint2*)(p + CX) = make_uint2(a2, b2);
      }
    }
    // (this tile's epilogue operands, the next tile's halo and x pieces are requested in D's k-steps)
    int n1 = cn, ty1 = cty, tx1 = ctx;
    advance(n1, ty1, tx1);
    const bool live1 = tile + per < t_hi;
    const Pf pfn = pf_make(n1, ty1, tx1, live1);
    float mg_next = 0.f;
    // barrier B: halo, x tile (and, first tile, the weight planes) are complete
    __syncthreads();

    // ---------------- input gradient: KS k-steps x (MT rows x NT channel blocks) x 3 products, conv_f16x2_kernel's order.
    // k-step ks multiplies halo pixel (row + ky, column + kx) - CG = 32: tap (ky, kx) = (ks % 3, ks / 3), weights packed tap-major;
    // CG = 16: lane groups 0, 1 take tap 2 ks, groups 2, 3 tap 2 ks + 1 (the tenth slot's weights are zero; its pixels are tap 8's).
    {
      const int xa_lane = (wave * MT * IC + li) * PSG + (CG == 32 ? lg * 8 : (lg & 1) * 8);
      const bool hi_tap = (lg >> 1) != 0;
      // ONE fragment set: the SIMD's other wave covers the latency of these reads.  The reads are issued in the order the products
      // need them (pixel plane 1 x weight plane 0 first).
      s16x8 fa[NP][MT], fw[NP][NT];
      auto load_frag = [&](int ks) __attribute__((always_inline)) {
        int xoff, wt;
        if (KS == 9) {
          const int kx = ks / 3, ky = ks % 3;
          xoff = (ky * IC + kx) * PSG;
          wt = ky * 3 + kx;
        } else {
          const int t0 = 2 * ks, t1 = 2 * ks + 1 > 8 ? 8 : 2 * ks + 1;
          xoff = hi_tap ? ((t1 / 3) * IC + t1 % 3) * PSG : ((t0 / 3) * IC + t0 % 3) * PSG;
          wt = ks;
        }
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
        constexpr int LKS = KS == 9 ? 6 : 4;
#pragma unroll
        for (int it = 0; it < NLOAD; ++it)
          if (it * LKS / NLOAD == ks) pf_issue(pfn, it);
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
      const f32x4 o = fbc_epi_value<false, EPIACT>(acc[mt][nt], desc, cxw[i], XSRC == 2 ? cxw[i] : cact[EPIACT && XSRC != 2 ? i : 0]);
      const u32x4 ov = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
      __builtin_amdgcn_raw_buffer_store_b128(ov, bx_rsrc(cur_y, y_bytes), cur_off[mt] + nt * 64, 0, 0);
      if (EPIAB) {
        const float4 xv = XSRC == 1 ? cxw[i] : cab[EPIAB && XSRC != 1 ? i : 0];
        fbc_ab_add(o, livef, xv, sA[nt], sB[nt]);
      }
      if (XSH) x_issue(n1, ty1, tx1, live1, i, i + 1);   // (the shared register is free again: the next tile's piece)
    };

    // ---------------- weight gradient: this wave's 9 accumulator tiles (channel block cb) over the 64 pixels of the tile rows
    // 4 pq .. 4 pq + 3: two k-steps of 32 pixels (tile rows 4 pq + 2 s, + 1), per k-step the x^T fragments (planes) against the gy
    // fragments of the 9 tap shifts - centre pixel (r', c') meets the halo pixel (r' + 2 - ky, c' + 2 - kx), so tap row ky of
    // k-step s reads the halo row pair (4 pq + 2 s + 2 - ky, + 1).  One fragment set per tap (see D); the input gradient's epilogue
    // and the next tile's halo arithmetic ride in the six sub-steps.
    {
      s16x8 fx[NP];        // x^T: [plane]
      const int hr0 = pq * QR;
      auto load_x = [&](int s) __attribute__((always_inline)) {
        const unsigned short* xq = xt + ((hr0 + 2 * s) * FM_TC + 4 * lg + tq) * PSX + xcb + tp * 4;
#pragma unroll
        for (int p = 0; p < NP; ++p) fx[p] = fbc_tr_read8(xq + p * CX, xq + FM_TC * PSX + p * CX);
      };
      // tap (ky, kx) of k-step s: halo rows row0, row0 + 1 shifted by 2 - kx columns; one fragment set per tap
      auto mm_tap = [&](int row0, int ky, int kx) __attribute__((always_inline)) {
        s16x8 G[NP];
        const unsigned short* gq = xh + (row0 * IC + (4 * lg + tq) + 2 - kx) * PSG + gcb + tp * 4;
#pragma unroll
        for (int p = 0; p < NP; ++p) G[p] = fbc_tr_read8(gq + p * CG, gq + IC * PSG + p * CG);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int j = ky * 3 + kx;
          accw[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, fx[PO::PA[q]]),
                                                           __builtin_bit_cast(f16x8_t, G[PO::PB[q]]), accw[j], 0, 0, 0);
        }
      };
      auto ride = [&](int slot) __attribute__((always_inline)) {   // slot 0 .. 5
#pragma unroll
        for (int i = 0; i < NPIECE; ++i)
          if (i * 6 / NPIECE == slot) epi_piece(i);
#pragma unroll
        for (int it = 0; it < NLOAD; ++it)
          if (it * 6 / NLOAD == slot) prep_item(it, mg_next);   // the next tile's halo items (requested in D) become final
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
    mg_lane = mg_next;
  };

  int flushed = 0;
  bool resume = false;
  float* out = fa_.part + (long)blockIdx.x * K::PART;
  // the workgroup's dW leaves for its slab: the waves of the pixel quarters 1 .. 3 hand their accumulators to quarter 0's wave of the
  // same channel block through LDS (the halo and the x tile, which nobody reads between the barriers below); that wave adds them in
  // quarter order, scales by 2^-S and writes (or adds to what an earlier pass left).  Element (tap j, register r) of lane (lg, li)
  // is dW[tap][xcb + 4 lg + r][gcb + li].
  auto slab_write = [&](bool add) {
    float* ex = (float*)xh;
    __syncthreads();   // (every wave has left the products that read the halo and the x tile)
    if (pq > 0) {
#pragma unroll
      for (int j = 0; j < K::NACC; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) ex[(((cb * (NQ - 1) + pq - 1) * K::NACC + j) * 4 + r) * 64 + lane] = accw[j][r];
    }
    __syncthreads();
    if (pq == 0) {
      const float dsc = __builtin_ldexpf(1.f, -S_w);
      const __amdgpu_buffer_rsrc_t orsrc = bx_rsrc(out, K::PART * 4u);
      // (one lane-varying offset, formed here from a thread index the compiler cannot tie to the tile loop's; an element's constant
      //  part and the wave's channel block travel in the scalar offset)
      int tl = (int)threadIdx.x;
      asm volatile("" : "+v"(tl));
      const unsigned o_lane = (unsigned)((((tl >> 4) & 3) * 4 * CG + (tl & 15)) * 4);
      const int o_cb = __builtin_amdgcn_readfirstlane((xcb * CG + gcb) * 4);
#pragma unroll
      for (int j = 0; j < K::NACC; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = accw[j][r];
#pragma unroll
          for (int qq = 0; qq < NQ - 1; ++qq) v += ex[(((cb * (NQ - 1) + qq) * K::NACC + j) * 4 + r) * 64 + (tl & 63)];
          const int oc = o_cb + ((j * CX + r) * CG) * 4;
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

int dis_fm_wpc(int cg, int cx) { return ((cg == 16 && cx == 32) || (cg == 32 && cx == 16)) ? 1 : 0; }

// Launch (f.c.cx channels of gy, f.c.cy of x): hipErrorInvalidValue when no instance exists for the combination (the caller keeps the
// two launches).  Forms: operand gy SELU'(y), not accumulating - plain epilogue (conv3), or the epilogue of
// dis_conv2d_dgrad_bf16x3_act_gnsums_res with x = ab_act_y fetched once (final_conv, ref_conv's 16-channel source).
template <int CG, int CX>
static hipError_t fm_launch(const FbArgs& f, int inact, bool xgn, int xsrc, long grid, hipStream_t stream) {
  const ConvArgs& a = f.c;
  constexpr int S = DIS_ACT_SELU;
  if (inact != S || a.gnb_coef || a.gnb_out || a.accum || xgn) return hipErrorInvalidValue;
  static bool attr_set[2] = {};
  if (!a.ab_out && !a.ab_act_y && xsrc == 0)
    return fbc_launch<FmCfg<CG, CX>>(conv_bwd_fused_mixed_kernel<CG, CX, S, false, 0, 0>, attr_set[0], "conv_bwd_fused_mixed_kernel", f,
                                     grid, stream);
  if (a.ab_out && a.ab_act_y && xsrc == 2)
    return fbc_launch<FmCfg<CG, CX>>(conv_bwd_fused_mixed_kernel<CG, CX, S, true, S, 2>, attr_set[1], "conv_bwd_fused_mixed_kernel", f,
                                     grid, stream);
  return hipErrorInvalidValue;
}
hipError_t dis_fm_launch(const FbArgs& f, int inact, bool xgn, int xsrc, long grid, hipStream_t stream) {
  if (f.c.cx == 32 && f.c.cy == 16) return fm_launch<32, 16>(f, inact, xgn, xsrc, grid, stream);
  if (f.c.cx == 16 && f.c.cy == 32) return fm_launch<16, 32>(f, inact, xgn, xsrc, grid, stream);
  return hipErrorInvalidValue;
}
