// Shared parts of the one-launch 3x3 conv backward kernels - conv_bwd_fused.hip (32 -> 32, two-term fp16), conv_bwd_fused_c16.hip
// (16 -> 16, two-term fp16), conv_bwd_fused_mixed.hip (16 <-> 32, two-term fp16) and conv_bwd_fused_bf16x3.hip (32 -> 32, three-term
// bf16); included by these four files only.
// What is here is a pure function of its arguments: the small device helpers, the walk over the tiles, the table that maps a call's
// form to a kernel instance, and the launch helper.  The phases of the kernels themselves stay in their files: the 32 -> 32 two-term
// kernel fills the register file, and moving its text moves its registers (profiles/r9_bwd_fused_shared.md).
#pragma once
#include "conv_args.h"
#include <type_traits>

// 8 x 16-bit of a transposing LDS read pair (ds_read_b64_tr_b16): the x^T and shifted gy fragments of the weight-gradient products
typedef short fbc_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ s16x8 fbc_tr_read8(const unsigned short* p0, const unsigned short* p1) {
  const fbc_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fbc_s16x4*)p0);
  const fbc_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fbc_s16x4*)p1);
  return (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <int I, int N, class F>
__device__ __forceinline__ void fbc_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    fbc_static_for<I + 1, N>(f);
  }
}
// The tap / channel -> k-slot map of the weight planes, input-gradient order (flipped taps, transposed), for CG channels of gy:
// conv_f16x2.hip's f2_weight / conv2d.hip's bx_weight in mode 1.  CG = 32: k-step ks is tap ks, lane group lg holds channels
// 8 lg ..; CG = 16: k-step ks is the tap pair 2 ks, 2 ks + 1 in lane groups 0, 1 and 2, 3 (the tenth slot is zero).
template <int CG>
__device__ __forceinline__ float fbc_weight(const float* w, int stride_row, int wo, int wi, int ks, int lg, int j, int co) {
  if constexpr (CG == 32) {
    const int c = 8 * lg + j;
    return (c < wo && co < wi) ? w[c * stride_row + co * 9 + (8 - ks)] : 0.f;
  } else {
    static_assert(CG == 16, "16 or 32 channels of gy");
    const int tap = 2 * ks + (lg >> 1);
    const int c = 8 * (lg & 1) + j;
    if (tap > 8) return 0.f;
    return (c < wo && co < wi) ? w[c * stride_row + co * 9 + (8 - tap)] : 0.f;
  }
}
// Product orders, operand planes (A, B) of product q.  Two-term fp16: a2 b1, a1 b2, a1 b1 (conv_f16x2_kernel's); three-term bf16:
// the six products smallest terms first (conv_bf16x3_kernel's).
struct FbcOrder2 {
  static constexpr int PA[3] = {1, 0, 0};
  static constexpr int PB[3] = {0, 1, 0};
};
struct FbcOrder3 {
  static constexpr int PA[6] = {2, 1, 0, 1, 0, 0};
  static constexpr int PB[6] = {0, 1, 2, 0, 1, 0};
};

// The walk over the n * tiles_y * tiles_x tiles of a launch.  A grid that is a multiple of 8 is dealt round-robin to the 8 XCDs; an XCD
// takes a contiguous share [t_lo, t_hi) of the tiles (its L2 sees neighbouring halos) and its `per` workgroups walk the share with
// stride `per`: workgroup `rank` runs tiles t_lo + rank, + per, ... < t_hi.  (tx, ty, n) of the next tile follow from the current
// one's by adding the stride's own (d_tx, d_ty, d_n) with two carries (fbc_advance): no division in the tile loop.
// (Plain ints, not a struct the kernels' lambdas would capture: that form moved the register allocation of 11 of the 29 instances.)
__device__ __forceinline__ void fbc_tile_share(int n, int tiles_y, int tiles_x, int& rank, int& per, int& t_lo, int& t_hi, int& d_tx,
                                               int& d_ty, int& d_n) {
  const int ntiles = n * tiles_y * tiles_x;
  const int nxcd = (gridDim.x % 8 == 0) ? 8 : 1;
  const int xcd = blockIdx.x % nxcd;
  rank = blockIdx.x / nxcd, per = gridDim.x / nxcd;
  t_lo = (int)((long)ntiles * xcd / nxcd), t_hi = (int)((long)ntiles * (xcd + 1) / nxcd);
  d_tx = per % tiles_x, d_ty = (per / tiles_x) % tiles_y, d_n = per / (tiles_x * tiles_y);
}
__device__ __forceinline__ void fbc_advance(int& n_, int& ty_, int& tx_, int d_n, int d_ty, int d_tx, int tiles_y, int tiles_x) {
  tx_ += d_tx, ty_ += d_ty, n_ += d_n;
  if (tx_ >= tiles_x) tx_ -= tiles_x, ++ty_;
  if (ty_ >= tiles_y) ty_ -= tiles_y, ++n_;
}

// XGN: the affine map of the GroupNorm in front of the conv for sample n - v -> v sc + sh with sc = rstd gamma, sh = beta - sc mean -
// for this lane's channels 16 nt + 4 lg .. (count: elements of a sample)
template <int NT>
__device__ __forceinline__ void fbc_gn_affine(const FbArgs& fa, int n, double count, int lg, float4* sc, float4* sh) {
  float mean, rstd;
  gn_moments(fa.wx_gn_stats, n, count, fa.wx_gn_eps, &mean, &rstd);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float4 g_ = *(const float4*)(fa.wx_gn_gamma + nt * 16 + lg * 4), b_ = *(const float4*)(fa.wx_gn_beta + nt * 16 + lg * 4);
    sc[nt] = make_float4(rstd * g_.x, rstd * g_.y, rstd * g_.z, rstd * g_.w);
    sh[nt] = make_float4(b_.x - sc[nt].x * mean, b_.y - sc[nt].y * mean, b_.z - sc[nt].z * mean, b_.w - sc[nt].w * mean);
  }
}

// sums of va and of vb over the 16 lanes of a DPP row (the 16 pixels of a tile row), valid in every lane of the row
__device__ __forceinline__ void fbc_row_sum2(float& va, float& vb) {
#define FBC_ROW(ctrl)                                                                               \
  va += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(va), ctrl, 0xf, 0xf, true)); \
  vb += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(vb), ctrl, 0xf, 0xf, true));
  FBC_ROW(0xB1) FBC_ROW(0x4E) FBC_ROW(0x124) FBC_ROW(0x128)
#undef FBC_ROW
}

// Bits of headroom the dW exponent of the two-term kernels keeps when it is (re)set: a later tile may be 2^6 larger before the
// accumulators have to move again (the policy itself is the pass loop of each kernel).  -DFB_SMARGIN=n on a build of the whole library
// sets it for BOTH two-term kernels (the 16 -> 16 kernel's own FC_SMARGIN used to be fixed at 6); scripts/diag/fb_variant.sh, which
// recompiles conv_bwd_fused.hip alone, still changes the 32 -> 32 kernel only.
#ifndef FB_SMARGIN
#define FB_SMARGIN 6
#endif
constexpr int FBC_SMARGIN = FB_SMARGIN;

// Epilogue of the input gradient (conv_f16x2_kernel's arithmetic): the accumulator descaled, + gx so far (ACCUM), times act'(actq)
// (EPIACT); fbc_ab_add: its terms of the channel sums - g and g x of a pixel inside the map (livef 1, else 0)
template <bool ACCUM, int EPIACT>
__device__ __forceinline__ f32x4 fbc_epi_value(const f32x4& acc, float desc, const float4& old, const float4& actq) {
  f32x4 o = acc * desc;
  if (ACCUM) o += (f32x4){old.x, old.y, old.z, old.w};
  if (EPIACT)
    o *= (f32x4){act_grad_from_out(actq.x, EPIACT), act_grad_from_out(actq.y, EPIACT), act_grad_from_out(actq.z, EPIACT),
                 act_grad_from_out(actq.w, EPIACT)};
  return o;
}
__device__ __forceinline__ void fbc_ab_add(const f32x4& o, float livef, const float4& xv, float (&sA)[4], float (&sB)[4]) {
  const float g0 = o[0] * livef, g1 = o[1] * livef, g2 = o[2] * livef, g3 = o[3] * livef;
  sA[0] += g0, sA[1] += g1, sA[2] += g2, sA[3] += g3;
  sB[0] = __builtin_fmaf(g0, xv.x, sB[0]), sB[1] = __builtin_fmaf(g1, xv.y, sB[1]);
  sB[2] = __builtin_fmaf(g2, xv.z, sB[2]), sB[3] = __builtin_fmaf(g3, xv.w, sB[3]);
}

// ---- host side ----
// A form of the two-term kernels: the template arguments of its instance (conv_bwd_fused_kernel's, see there) and its slot in the
// launch helper's table.
template <int INACT_, bool INCOEF_, bool ACCUM_, bool EPIAB_, int EPIACT_, int XSRC_, bool XGN_, bool GST_, int SLOT_>
struct FbcForm {
  static constexpr int INACT = INACT_, EPIACT = EPIACT_, XSRC = XSRC_, SLOT = SLOT_;
  static constexpr bool INCOEF = INCOEF_, ACCUM = ACCUM_, EPIAB = EPIAB_, XGN = XGN_, GST = GST_;
};
constexpr int FBC_NFORMS = 12;
// Which form serves a call: `launch` is called with the FbcForm of the one instance that computes it and its result returned;
// hipErrorInvalidValue when there is none (the caller keeps the two launches).  Decided from: plain or coef operand (c.gnb_coef),
// c.accum, channel sums (c.ab_out), activation gradient at the output (c.ab_act_y), xsrc, xgn, gpre store (c.gnb_out), inact.
template <class L>
static hipError_t fbc_dispatch(const ConvArgs& a, int inact, bool xgn, int xsrc, L&& launch) {
  constexpr int S = DIS_ACT_SELU;
  if (inact != 0 && inact != S) return hipErrorInvalidValue;
  const bool coef = a.gnb_coef != nullptr, gst = a.gnb_out != nullptr, ab = a.ab_out != nullptr, epiact = a.ab_act_y != nullptr;
  if (!coef) {
    // plain operand (gy itself, or gy act'(y)): no epilogue forms
    if (ab || gst || xgn || xsrc) return hipErrorInvalidValue;
    if (a.accum) return inact ? launch(FbcForm<S, false, true, false, 0, 0, false, false, 0>{})
                              : launch(FbcForm<0, false, true, false, 0, 0, false, false, 1>{});
    return inact ? launch(FbcForm<S, false, false, false, 0, 0, false, false, 2>{})
                 : launch(FbcForm<0, false, false, false, 0, 0, false, false, 3>{});
  }
  if (ab && !a.accum && !epiact && xsrc == 1 && xgn) {   // conv2d_gn_in: the GroupNorm input of the sums is the conv's input
    if (gst) return inact ? hipErrorInvalidValue : launch(FbcForm<0, true, false, true, 0, 1, true, true, 4>{});
    return inact ? launch(FbcForm<S, true, false, true, 0, 1, true, false, 5>{})
                 : launch(FbcForm<0, true, false, true, 0, 1, true, false, 6>{});
  }
  if (gst || xgn) return hipErrorInvalidValue;
  if (ab && a.accum && epiact && xsrc == 2 && inact == S)   // ResNetBlock chain: x = SELU(GroupNorm(x2) + res) is the conv's input
    return launch(FbcForm<S, true, true, true, S, 2, false, false, 7>{});
  if (ab && a.accum && !epiact && xsrc == 0 && inact == S)  // two-consumer GroupNorm output (Block2D3D conv1_1)
    return launch(FbcForm<S, true, true, true, 0, 0, false, false, 8>{});
  if (!ab && a.accum && xsrc == 0 && inact == S) return launch(FbcForm<S, true, true, false, 0, 0, false, false, 9>{});
  if (!ab && !a.accum && xsrc == 0)
    return inact ? launch(FbcForm<S, true, false, false, 0, 0, false, false, 10>{})
                 : launch(FbcForm<0, true, false, false, 0, 0, false, false, 11>{});
  return hipErrorInvalidValue;
}

// One launch of a kernel instance with K::LDS_BYTES of dynamic LDS (the attribute is set once per instance: attr_set is the
// instance's own flag) and K::NTHR threads
template <class K, class Kern>
static hipError_t fbc_launch(Kern kern, bool& attr_set, const char* tag, const FbArgs& f, long grid, hipStream_t stream) {
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  DIS_TAG(tag);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(K::NTHR), K::LDS_BYTES, stream, f);
  return hipSuccess;
}
