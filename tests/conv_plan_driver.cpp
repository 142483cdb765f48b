// Stand-alone driver of depthinspace_amd/csrc/conv_plan.h for tests/test_conv_plan_cpu.py (host code only, no GPU, no HIP).
// stdin: one shape per line, "mode k stride pad hin win hout wout".  stdout, per shape and per form - "fused" (the one-launch
// four-phase form offered and accepted), "split" (not offered), "fallback" (offered, refused with DIS_ERR_UNSUPPORTED):
//   FORM <name>
//   L <slice> <halo_only> <hv> <wv> <S> <osy> <ooy> <osx> <oox> <nph> <ntaps> <s_ci> <s_co>     one per launch
//   P <k0> <kn> <oy> <ox>                                                                        nph of them when nph > 1
//   T <dy> <dx> <tsrc>                                                                           ntaps of them
//   RC <status>
// and, once per shape, "NEED <launches>": the launch count of the workspace companion.
#include <cstdio>
#include <cstring>

#include "conv_plan.h"

struct PlanArgs {   // the fields of GenArgs / GenArgsB the driver fills, arrays of their sizes
  int hv, wv, S, osy, ooy, osx, oox, ntaps, nph;
  short tdy[CONV_PLAN_MAXTAPS], tdx[CONV_PLAN_MAXTAPS];
  unsigned char ph_k0[4], ph_kn[4], ph_oy[4], ph_ox[4];
};

int main() {
  int mode, k, stride, pad, hin, win, hout, wout;
  const int cin_w = 3, cout_w = 5;
  while (std::scanf("%d %d %d %d %d %d %d %d", &mode, &k, &stride, &pad, &hin, &win, &hout, &wout) == 8) {
    std::printf("CASE %d %d %d %d %d %d %d %d\n", mode, k, stride, pad, hin, win, hout, wout);
    static const char* const forms[3] = {"fused", "split", "fallback"};
    for (int form = 0; form < 3; ++form) {
      std::printf("FORM %s\n", forms[form]);
      PlanArgs a;
      std::memset(&a, 0x7f, sizeof a);   // (a field the driver forgets shows up as garbage in the plan)
      const int rc = conv_plan_run(a, mode, k, stride, pad, hin, win, hout, wout, cin_w, cout_w, form != 1,
                                   [&](const PlanArgs& b, int slice, long s_ci, long s_co, const short* tsrc, bool halo_only) {
                                     std::printf("L %d %d %d %d %d %d %d %d %d %d %d %ld %ld\n", slice, (int)halo_only, b.hv, b.wv, b.S,
                                                 b.osy, b.ooy, b.osx, b.oox, b.nph, b.ntaps, s_ci, s_co);
                                     if (b.nph > 1)
                                       for (int p = 0; p < b.nph; ++p)
                                         std::printf("P %d %d %d %d\n", b.ph_k0[p], b.ph_kn[p], b.ph_oy[p], b.ph_ox[p]);
                                     for (int t = 0; t < b.ntaps; ++t) std::printf("T %d %d %d\n", b.tdy[t], b.tdx[t], tsrc[t]);
                                     return halo_only && form == 2 ? DIS_ERR_UNSUPPORTED : DIS_OK;
                                   });
      std::printf("RC %d\n", rc);
    }
    int launches = -1;
    conv_plan_max_need(mode, k, stride, pad, hout, wout, [](long, long, int) { return 0L; }, &launches);
    std::printf("NEED %d\n", launches);
  }
  return 0;
}
