// Host-side planning shared by the two streaming conv families, conv_gen.hip (fp32 tensors, dis_convg_*) and conv_bf16.hip (bf16
// activation storage, dis_convb_*): how (mode, k, stride, pad) becomes launches with their tap lists, and the pieces of the halo
// and weight-gradient plans that do not depend on a family's tile constants.  Plain C++17 - no HIP, no device code - so that
// tests/test_conv_plan_cpu.py can compile it with a host compiler and check the tap arithmetic against the definition of the modes.
#pragma once
#include "../../include/dis_hip.h"

#define CONV_PLAN_MAXTAPS 49   // tdy / tdx hold this many taps (CG_MAXTAPS, CB_MAXTAPS)

static inline int floordiv2(int v) { return (v >= 0) ? v / 2 : -((-v + 1) / 2); }

static inline bool conv_plan_supported(int mode, int k, int stride) {
  return k * k <= CONV_PLAN_MAXTAPS && (stride == 1 || stride == 2) && mode >= 0 && mode <= 3;
}
// the input gradient of a stride-2 conv and the transposed conv write every second output pixel per launch: four parity classes
static inline bool conv_plan_phased(int mode, int stride) {
  return (mode == DIS_CONVG_CONV_DGRAD || mode == DIS_CONVG_TCONV) && stride == 2;
}

// Taps of parity class (py, px) of the stride-2 transposed form, out[2 vy + py] = sum_ky in[vy + (py + pad - ky) / 2] W[ky] over the
// ky that make the quotient whole (the same in x): input offsets to tdy / tdx, weight positions ky * k + kx to tsrc.  Returns the
// number of taps; null arrays: count only.
static inline int conv_plan_class_taps(int k, int pad, int py, int px, short* tdy, short* tdx, short* tsrc) {
  int nt = 0;
  for (int ky = 0; ky < k; ++ky) {
    if ((py + pad - ky) & 1) continue;
    for (int kx = 0; kx < k; ++kx) {
      if ((px + pad - kx) & 1) continue;
      if (tdy) {
        tdy[nt] = (short)floordiv2(py + pad - ky);
        tdx[nt] = (short)floordiv2(px + pad - kx);
        tsrc[nt] = (short)(ky * k + kx);
      }
      ++nt;
    }
  }
  return nt;
}

// The launches of one dis_convg_run / dis_convb_run call.  `a` arrives with everything but the plan filled in; per launch the driver
// fills hv wv S osy ooy osx oox ntaps tdy tdx nph (ph_k0 ph_kn ph_oy ph_ox when nph = 4) of a copy and calls
//   run(args, slice, s_ci, s_co, tsrc, halo_only) -> status
// slice: the packing slice of the launch (0 .. 3); s_ci / s_co: floats between the input / output channels of the raw weight;
// tsrc[t]: position of tap t inside a k x k filter; halo_only: the four classes in ONE launch (they read the same input tile),
// offered first when try_fused is set - DIS_ERR_UNSUPPORTED from it falls back to one launch per class.
template <class A, class Run>
static inline int conv_plan_run(A& a, int mode, int k, int stride, int pad, int hin, int win, int hout, int wout, int cin_w,
                                int cout_w, bool try_fused, Run&& run) {
  if (hin <= 0 || win <= 0 || hout <= 0 || wout <= 0 || cin_w <= 0 || cout_w <= 0 || k <= 0 || pad < 0) return DIS_ERR_BAD_SHAPE;
  if (!conv_plan_supported(mode, k, stride)) return DIS_ERR_UNSUPPORTED;
  const bool direct = mode == DIS_CONVG_CONV || mode == DIS_CONVG_TCONV_DGRAD;
  if (mode == DIS_CONVG_CONV) {
    if (hout != (hin + 2 * pad - k) / stride + 1 || wout != (win + 2 * pad - k) / stride + 1) return DIS_ERR_BAD_SHAPE;
  } else if (mode == DIS_CONVG_TCONV_DGRAD && stride != 2) {
    return DIS_ERR_UNSUPPORTED;
  }
  // direct form: out[vy][vx] = sum_taps in[vy*S + ky - pad][vx*S + kx - pad] * W
  //   conv: w[co][ci][ky][kx] (co rows of cin_w);  tconv dgrad: w[ci_t = out][co_t = in][ky][kx]
  // transposed form: out[oy][ox] = sum_{ky,kx : parity} in[(oy + pad - ky)/S][(ox + pad - kx)/S] * W
  //   conv dgrad:  w[ci_in(= conv cout)][co_out(= conv cin)]  stored as w[conv_co][conv_ci][ky][kx]
  //   tconv fwd :  w[ci][co][ky][kx]
  const long kk = (long)k * k;
  const long s_ci = direct ? kk : (long)cout_w * kk, s_co = direct ? (long)cin_w * kk : kk;
  short tsrc[CONV_PLAN_MAXTAPS];
  a.nph = 1;
  if (direct || stride == 1) {   // one launch over the whole output: the k x k window, flipped in the transposed form
    a.hv = hout; a.wv = wout; a.S = stride; a.osy = 1; a.ooy = 0; a.osx = 1; a.oox = 0;
    a.ntaps = k * k;
    for (int ky = 0; ky < k; ++ky)
      for (int kx = 0; kx < k; ++kx) {
        a.tdy[ky * k + kx] = (short)(direct ? ky - pad : pad - ky);
        a.tdx[ky * k + kx] = (short)(direct ? kx - pad : pad - kx);
        tsrc[ky * k + kx] = (short)(ky * k + kx);
      }
    return run(a, 0, s_ci, s_co, tsrc, false);
  }
  if (try_fused) {   // taps listed class by class
    A b = a;
    b.hv = (hout + 1) / 2; b.wv = (wout + 1) / 2; b.S = 1;
    b.osy = 2; b.ooy = 0; b.osx = 2; b.oox = 0;
    b.nph = 4;
    int nt = 0;
    bool ok = true;
    for (int ph = 0; ph < 4; ++ph) {
      const int py = ph >> 1, px = ph & 1;
      const int c = conv_plan_class_taps(k, pad, py, px, b.tdy + nt, b.tdx + nt, tsrc + nt);
      b.ph_k0[ph] = (unsigned char)nt; b.ph_kn[ph] = (unsigned char)c;
      b.ph_oy[ph] = (unsigned char)py; b.ph_ox[ph] = (unsigned char)px;
      ok = ok && c > 0;
      nt += c;
    }
    b.ntaps = nt;
    if (ok) {
      const int rc = run(b, 0, s_ci, s_co, tsrc, true);
      if (rc != DIS_ERR_UNSUPPORTED) return rc;
    }
  }
  for (int ph = 0; ph < 4; ++ph) {   // every class packs into its own slice
    const int py = ph >> 1, px = ph & 1;
    A b = a;
    b.hv = (hout - py + 1) / 2; b.wv = (wout - px + 1) / 2; b.S = 1;
    b.osy = 2; b.ooy = py; b.osx = 2; b.oox = px;
    b.ntaps = conv_plan_class_taps(k, pad, py, px, b.tdy, b.tdx, tsrc);
    if (b.hv <= 0 || b.wv <= 0) continue;
    // no tap reaches this parity class (cannot happen for k >= 2): outputs would be bias only
    if (b.ntaps == 0) return DIS_ERR_UNSUPPORTED;
    const int rc = run(b, ph, s_ci, s_co, tsrc, false);
    if (rc != DIS_OK) return rc;
  }
  return DIS_OK;
}

// Largest need(hv, wv, ntaps) over the launches conv_plan_run makes without the fused form (the *_splitk_workspace queries);
// launches: their number, if asked for.
template <class Need>
static inline long conv_plan_max_need(int mode, int k, int stride, int pad, int hout, int wout, Need&& need, int* launches = nullptr) {
  long best = 0;
  int nl = 0;
  if (!conv_plan_phased(mode, stride)) {
    best = need((long)hout, (long)wout, k * k);
    nl = 1;
  } else {
    for (int ph = 0; ph < 4; ++ph) {
      const int py = ph >> 1, px = ph & 1;
      const long hv = (hout - py + 1) / 2, wv = (wout - px + 1) / 2;
      if (hv <= 0 || wv <= 0) continue;
      const long v = need(hv, wv, conv_plan_class_taps(k, pad, py, px, nullptr, nullptr, nullptr));
      best = v > best ? v : best;
      ++nl;
    }
  }
  if (launches) *launches = nl;
  return best;
}

// ---- halo forms (ch2_plan / ch2_run, cb_halo_plan / cb_run_halo): the parts that do not depend on a family's tiles ----
struct ConvTapBox { int dy0, dy1, dx0, dx1; };
template <class A>
static inline ConvTapBox conv_plan_tap_box(const A& a) {
  ConvTapBox b = {a.tdy[0], a.tdy[0], a.tdx[0], a.tdx[0]};
  for (int t = 1; t < a.ntaps; ++t) {
    b.dy0 = a.tdy[t] < b.dy0 ? a.tdy[t] : b.dy0; b.dy1 = a.tdy[t] > b.dy1 ? a.tdy[t] : b.dy1;
    b.dx0 = a.tdx[t] < b.dx0 ? a.tdx[t] : b.dx0; b.dx1 = a.tdx[t] > b.dx1 ? a.tdx[t] : b.dx1;
  }
  return b;
}
// column walk (KC instances of the halo kernels): a full K x K stride-1 window on 16-row tiles with streamed weights, the two
// instances that exist; two LDS buffers of one column (frag = 16-byte weight vectors per cout column and tap) must fit lds_max
// next to the halo.  Sets kc, GT and wsz16 when the plan qualifies.
template <class A>
static inline void conv_plan_column_walk(A& a, const ConvTapBox& b, int bn, int frag, long lds_max) {
  const int K = b.dy1 - b.dy0 + 1;
  if (a.nph == 1 && a.S == 1 && a.TP == 1 && !a.res && a.trh == 16 && b.dx1 - b.dx0 + 1 == K && a.ntaps == K * K &&
      ((K == 7 && bn == 32) || (K == 5 && bn == 64))) {
    const long wsz = 2L * K * frag * bn * 16 / 2;   // two buffers of one column (16-bit words)
    if (256 + 2 * wsz + (long)a.HR * a.HC * a.PS * 2 <= lds_max) {
      a.kc = K;
      a.GT = K;
      a.wsz16 = (int)wsz;
    }
  }
}
// ... its tap order: (dx, dy) ascending - slot (dx - dx0) * kc + (dy - dy0); the window is full.  Reorders a's taps and writes the
// weight positions of the new order to tsrc_out.
template <class A>
static inline void conv_plan_column_order(A& a, const short* tsrc, short* tsrc_out) {
  short ty[CONV_PLAN_MAXTAPS], tx[CONV_PLAN_MAXTAPS];
  for (int t = 0; t < a.ntaps; ++t) {
    const int slot = (a.tdx[t] - a.dx0) * a.kc + (a.tdy[t] - a.dy0);
    ty[slot] = a.tdy[t]; tx[slot] = a.tdx[t]; tsrc_out[slot] = tsrc[t];
  }
  for (int t = 0; t < a.ntaps; ++t) a.tdy[t] = ty[t], a.tdx[t] = tx[t];
}
// persistent grid: as many workgroups as stay resident (lds bytes each out of lds_cu, at most wpc_max per CU) on ncu CUs, no
// more than there are units of work, a multiple of the 8 XCDs
static inline long conv_plan_persistent_grid(long lds, long lds_cu, long wpc_max, int ncu, long units) {
  long wpc = lds_cu / lds;
  wpc = wpc > wpc_max ? wpc_max : (wpc < 1 ? 1 : wpc);
  long grid = wpc * ncu;
  if (grid > units) grid = units;
  if (grid >= 8) grid -= grid % 8;
  return grid;
}

// ---- weight gradient (convg_wgrad_kernel, convb_wgrad_kernel): 32 mtw x 32 ntw channel tiles per tap, split-K over the pixels ----
struct WgradSplitPlan { int mtw, ntw, nxb, ngb, nsplit, mper; };
static inline WgradSplitPlan wgrad_split_plan(int n, int hG, int wG, int cX, int cG, int k) {
  WgradSplitPlan p;
  p.mtw = cX > 32 ? 2 : 1;
  p.ntw = cG > 32 ? 2 : 1;
  const int TX = 32 * p.mtw, TG = 32 * p.ntw;
  p.nxb = (cX + TX - 1) / TX;
  p.ngb = (cG + TG - 1) / TG;
  const long base = (long)k * k * p.nxb * p.ngb;
  const long M = (long)n * hG * wG;
  long sp = (2048 + base - 1) / base;
  const long maxsp = (M + 255) / 256;  // at least 256 pixels (8 k-steps) per split
  if (sp > maxsp) sp = maxsp;
  if (sp < 1) sp = 1;
  long mp = (M + sp - 1) / sp;
  mp = (mp + 31) / 32 * 32;
  sp = (M + mp - 1) / mp;
  p.nsplit = (int)sp;
  p.mper = (int)mp;
  return p;
}
