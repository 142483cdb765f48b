// CPU-only check of the host side of the three one-launch 3x3 conv backward entry points (dis_conv2d_bwd_fused_f16x2, ..._f16x2_c16,
// ..._bf16x3): prints their workspace queries and the return code of 6798 bad calls - every argument check reached, alone and in
// combination with the others; a call that passes them all is refused for its size, so nothing is ever launched and no GPU is needed.
// Two builds of the library answer alike when the two outputs are equal:
//   clang++ -O1 scripts/diag/bwd_fused_errcodes.cpp -o /tmp/errcodes -ldl
//   /tmp/errcodes <libA.so> 1 > a.txt; /tmp/errcodes <libB.so> 1 > b.txt; cmp a.txt b.txt     (1 = DIS_ACT_SELU)
// also under DIS_CONV_SPLIT=bf16x3 and DIS_BWD_FUSED=0.  With -fsanitize=address,undefined on the line above it loads
// libdis_hip_asan.so (make asan) without a preload.
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
typedef int (*f16_t)(const float*, const float*, const float*, int, float*, const float*, int, int, int, float*, int, const float*,
                     const float*, double*, const float*, const double*, const float*, const float*, float, float*, float*, float*, int,
                     int, int, int, int, void*);
typedef int (*c16_t)(const float*, const float*, const float*, int, float*, const float*, int, int, int, float*, int, const float*,
                     const float*, double*, int, const float*, const double*, const float*, const float*, float, float*, float*, float*,
                     int, int, int, int, void*);
typedef int (*b3_t)(const float*, const float*, int, const float*, int, int, int, float*, int, const float*, const double*, const float*,
                    const float*, float, float*, float*, float*, int, int, int, int, int, void*);
typedef long (*ws1_t)(int);
typedef long (*ws2_t)(int, int);

int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  f16_t f16 = (f16_t)dlsym(h, "dis_conv2d_bwd_fused_f16x2");
  c16_t c16 = (c16_t)dlsym(h, "dis_conv2d_bwd_fused_f16x2_c16");
  b3_t b3 = (b3_t)dlsym(h, "dis_conv2d_bwd_fused_bf16x3");
  ws1_t ws = (ws1_t)dlsym(h, "dis_conv2d_bwd_fused_workspace"), ws3 = (ws1_t)dlsym(h, "dis_conv2d_bwd_fused_bf16x3_workspace");
  ws2_t wsc = (ws2_t)dlsym(h, "dis_conv2d_bwd_fused_c16_workspace");
  if (!f16 || !c16 || !b3 || !ws || !ws3 || !wsc) return 3;
  for (int c = 0; c <= 64; c += 16) printf("ws %d: %ld %ld | %ld %ld %ld\n", c, ws(c), ws3(c), wsc(c, c), wsc(16, c), wsc(c, 32));
  float buf[64];
  double dbuf[8];
  float* P = buf;
  double* D = dbuf;
  const int HUGE_H = 40000, HUGE_W = 40000;   // hin * win * c * 4 >= 0x7fff0000: refused before anything is launched
  int k = 0;
  // every argument as a small table: index of the mutation -> call.  Base call: all pointers valid, shape huge (so a call that
  // passes every check still returns before the launch).
  for (int null_g = 0; null_g < 2; ++null_g)
    for (int shape = 0; shape < 2; ++shape)
      for (int chan = 0; chan < 4; ++chan)       // 0 ok, 1 w_o wrong, 2 w_i wrong, 3 c wrong
        for (int act = 0; act < 3; ++act)        // 0 none, 1 selu (DIS_ACT_SELU looked up below), 2 invalid
          for (int qn = 0; qn < 2; ++qn)         // q null
            for (int cf = 0; cf < 2; ++cf)       // coef given
              for (int gp = 0; gp < 2; ++gp)     // gpre_out given
                for (int ab = 0; ab < 5; ++ab)   // 0 none, 1 ab_out+ab_x, 2 ab_out only, 3 act_y without ab_out, 4 all three
                  for (int acc = 0; acc < 2; ++acc)
                    for (int sl = 0; sl < 2; ++sl)      // c16: ab_slots 0 / 4
                      for (int gn = 0; gn < 3; ++gn)    // 0 none, 1 stats only, 2 all
                        for (int rs = 0; rs < 3; ++rs)  // 0 zero strides, 1 w stride too small, 2 grad_w stride not a multiple of 9
                        {
                          ++k;
                          if ((k * 2654435761u >> 8) % 37 != 0 && k > 400) continue;   // (a fixed sample of the 276 k combinations + the first 400)
                          for (int fam = 0; fam < 3; ++fam) {
                            const int C = fam == 1 ? 16 : 32;
                            const int w_o = chan == 1 ? C + 16 : C, w_i = chan == 2 ? C / 2 : C, c = chan == 3 ? 24 : C;
                            const int in_act = act == 0 ? 0 : (act == 1 ? atoi(argv[2]) : 77);
                            const float* g = null_g ? nullptr : P;
                            const float* q = qn ? nullptr : P;
                            const float* coef = cf ? P : nullptr;
                            float* gpre = gp ? P : nullptr;
                            double* ab_out = (ab == 1 || ab == 2 || ab == 4) ? D : nullptr;
                            const float* ab_x = (ab == 1 || ab == 4) ? P : nullptr;
                            const float* ab_y = (ab == 3 || ab == 4) ? P : nullptr;
                            const double* st = gn ? D : nullptr;
                            const float* gam = gn == 2 ? P : nullptr;
                            const int n = shape ? 0 : 1;
                            const int wrs = rs == 1 ? w_i * 9 - 1 : 0, gwrs = rs == 2 ? C * 9 + 1 : 0;
                            int r;
                            if (fam == 0)
                              r = f16(g, q, coef, in_act, gpre, P, w_o, w_i, wrs, P, acc, ab_x, ab_y, ab_out, P, st, gam, gam, 1e-5f, P, P, P, n,
                                      HUGE_H, HUGE_W, c, gwrs, nullptr);
                            else if (fam == 1)
                              r = c16(g, q, coef, in_act, gpre, P, w_o, w_i, wrs, P, acc, ab_x, ab_y, ab_out, sl * 4, P, st, gam, gam, 1e-5f, P, P, P,
                                      n, HUGE_H, HUGE_W, gwrs, nullptr);
                            else
                              r = b3(g, q, in_act, P, w_o, w_i, wrs, P, acc, P, st, gam, gam, 1e-5f, P, P, P, n, HUGE_H, HUGE_W, c, gwrs, nullptr);
                            printf("%d %d%d%d%d%d%d%d%d%d%d%d%d fam%d -> %d\n", k, null_g, shape, chan, act, qn, cf, gp, ab, acc, sl, gn, rs, fam, r);
                          }
                        }
  return 0;
}
