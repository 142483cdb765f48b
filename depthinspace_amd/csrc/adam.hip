// Fused Adam over a flat fp32 parameter buffer (torch.optim.Adam defaults, reference train_val.py:55-56).
#include "common.h"

const char* g_dis_last_kernel = nullptr;
// diagnostics: kernel family of the most recent conv dispatch of this process ("" if none since the last clear)
extern "C" int dis_last_kernel(char* name, int cap, int clear) {
  if (!name) return DIS_ERR_NULL;
  if (cap <= 0) return DIS_ERR_BAD_SHAPE;
  const char* r = g_dis_last_kernel ? g_dis_last_kernel : "";
  int i = 0;
  for (; i < cap - 1 && r[i]; ++i) name[i] = r[i];
  name[i] = 0;
  if (clear) g_dis_last_kernel = nullptr;
  return DIS_OK;
}

// omb1 / omb2 = (1 - beta) evaluated in double precision on the host and rounded once, as torch.optim.Adam's python floats
// are (1.f - 0.999f in fp32 is off by 1.3e-5 relative).
__global__ void adam_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                            float4* __restrict__ v, long count4, float lr, float b1, float b2, float omb1, float omb2,
                            float eps, float bc1, float bc2_sqrt, float gscale) {
  const float step = lr / bc1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < count4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
    float* P = (float*)&pp; float* G = (float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = G[k] * gscale;
      M[k] = M[k] * b1 + gr * omb1;
      V[k] = V[k] * b2 + (gr * gr) * omb2;
      const float denom = sqrtf(V[k]) / bc2_sqrt + eps;
      P[k] = P[k] - step * (M[k] / denom);
    }
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

extern "C" int dis_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count,
                             float lr, double beta1, double beta2, float eps, int step_count, float grad_scale,
                             void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq) return DIS_ERR_NULL;
  if (count <= 0 || step_count <= 0) return DIS_ERR_BAD_SHAPE;
  if (count % 4 != 0) return DIS_ERR_UNSUPPORTED;   // the flat buffer is padded by the caller
  const double bc1 = 1.0 - pow(beta1, (double)step_count);
  const double bc2 = 1.0 - pow(beta2, (double)step_count);
  hipLaunchKernelGGL(adam_kernel, dim3(dis_ew_grid(count / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (float4*)param, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, count / 4, lr,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, (float)bc1,
                     (float)sqrt(bc2), grad_scale);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}

// Graph-safe form: the step counter and the two bias corrections live on the device.  `state` is 4 x 32 bit:
// [0] int step count (number of steps taken so far), [1] float 1 - beta1^step, [2] float sqrt(1 - beta2^step), [3] unused.
// A one-thread kernel advances it, the update kernel reads it, so a hipGraph that captured ONE optimiser step applies
// step k's correction at its k-th replay (with the host-side form above the capture-time correction would be replayed).
__global__ void adam_advance_kernel(int* __restrict__ state, double b1, double b2) {
  const int step = state[0] + 1;
  state[0] = step;
  ((float*)state)[1] = (float)(1.0 - pow(b1, (double)step));
  ((float*)state)[2] = (float)sqrt(1.0 - pow(b2, (double)step));
}
__global__ void adam_dev_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                float4* __restrict__ v, long count4, float lr, float b1, float b2, float omb1, float omb2,
                                float eps, const int* __restrict__ state, float gscale) {
  const float bc1 = ((const float*)state)[1], bc2_sqrt = ((const float*)state)[2];
  const float step = lr / bc1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < count4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
    float* P = (float*)&pp; float* G = (float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = G[k] * gscale;
      M[k] = M[k] * b1 + gr * omb1;
      V[k] = V[k] * b2 + (gr * gr) * omb2;
      const float denom = sqrtf(V[k]) / bc2_sqrt + eps;
      P[k] = P[k] - step * (M[k] / denom);
    }
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}
extern "C" int dis_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count,
                                 float lr, double beta1, double beta2, float eps, int* state, float grad_scale,
                                 void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !state) return DIS_ERR_NULL;
  if (count <= 0) return DIS_ERR_BAD_SHAPE;
  if (count % 4 != 0) return DIS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, beta1, beta2);
  hipLaunchKernelGGL(adam_dev_kernel, dim3(dis_ew_grid(count / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (float4*)param, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, count / 4, lr,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, (const int*)state,
                     grad_scale);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}

// Hyper-parameters and the clip / skip decision on the device: the learning rate and max_norm are read from `hyper`, the
// global gradient norm is reduced by the call itself, so a captured step honours a learning rate the host changed between
// replays and clips (or skips a non-finite gradient) without the host ever looking at the gradient.
//   mode bit 0: clip by global norm (torch.nn.utils.clip_grad_norm_), bit 1: skip the step when the norm is not finite.
// The norm repeats bit for bit: workgroup b sums ADAM_NORM_CHUNK float4 of its own, every order of summation is fixed
// (per-thread fp64 accumulator in index order, DPP wave sum, waves in order, then the partials in order), and the number of
// workgroups depends on `count` alone.
#define ADAM_MODE_CLIP 1
#define ADAM_MODE_SKIP 2
#define ADAM_NORM_BLOCK 256
#define ADAM_NORM_PER_THREAD 8
#define ADAM_NORM_CHUNK (ADAM_NORM_BLOCK * ADAM_NORM_PER_THREAD)   // float4 per workgroup

static inline long adam_norm_blocks(long count4) { return (count4 + ADAM_NORM_CHUNK - 1) / ADAM_NORM_CHUNK; }

__global__ void __launch_bounds__(ADAM_NORM_BLOCK)
adam_norm_partials_kernel(const float4* __restrict__ g, long count4, float gscale, double* __restrict__ partials) {
  __shared__ double sm[ADAM_NORM_BLOCK / DIS_WAVE];
  const long base = (long)blockIdx.x * ADAM_NORM_CHUNK + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < ADAM_NORM_PER_THREAD; ++j) {
    const long i = base + (long)j * ADAM_NORM_BLOCK;
    if (i < count4) {
      const float4 gg = g[i];
      const double a = (double)(gg.x * gscale), b = (double)(gg.y * gscale), c = (double)(gg.z * gscale),
                   d = (double)(gg.w * gscale);
      acc += (a * a + b * b) + (c * c + d * d);
    }
  }
  const double r = block_sum_d(acc, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// One workgroup: (mode != 0) the partials in a fixed order -> stats {norm, clip coefficient, skipped steps, skipped this call};
// then thread 0 advances `state` exactly as adam_advance_kernel does, unless the step is skipped.
__global__ void __launch_bounds__(ADAM_NORM_BLOCK)
adam_hyper_advance_kernel(int* __restrict__ state, double b1, double b2, const float* __restrict__ hyper,
                          const double* __restrict__ partials, long nparts, double* __restrict__ stats, int mode) {
  __shared__ double sm[ADAM_NORM_BLOCK / DIS_WAVE];
  bool skip = false;
  if (mode != 0) {
    double acc = 0.0;
    for (long i = threadIdx.x; i < nparts; i += ADAM_NORM_BLOCK) acc += partials[i];
    const double norm2 = block_sum_d(acc, sm);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(norm2);
    double clip = 1.0;
    if (mode & ADAM_MODE_CLIP) {
      clip = (double)hyper[1] / (norm + 1e-6);
      if (clip > 1.0) clip = 1.0;   // (a NaN stays a NaN, as torch.clamp(max=1) leaves it)
    }
    skip = (mode & ADAM_MODE_SKIP) && !isfinite(norm2);
    stats[0] = norm;
    stats[1] = clip;
    if (skip) stats[2] = stats[2] + 1.0;
    stats[3] = skip ? 1.0 : 0.0;
  }
  if (threadIdx.x != 0 || skip) return;
  const int step = state[0] + 1;
  state[0] = step;
  ((float*)state)[1] = (float)(1.0 - pow(b1, (double)step));
  ((float*)state)[2] = (float)sqrt(1.0 - pow(b2, (double)step));
}

// adam_dev_kernel term for term; lr from hyper[0], the gradient multiplier grad_scale * (float)clip formed once per thread
// (clip == 1: grad_scale itself, the bits of dis_adam_step_dev), nothing touched when the step is skipped
__global__ void adam_hyper_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                  float4* __restrict__ v, long count4, const float* __restrict__ hyper, float b1, float b2,
                                  float omb1, float omb2, float eps, const int* __restrict__ state,
                                  const double* __restrict__ stats, int mode, float gscale) {
  float mult = gscale;
  if (mode != 0) {
    if ((mode & ADAM_MODE_SKIP) && stats[3] != 0.0) return;
    mult = gscale * (float)stats[1];
  }
  const float lr = hyper[0];
  const float bc1 = ((const float*)state)[1], bc2_sqrt = ((const float*)state)[2];
  const float step = lr / bc1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < count4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
    float* P = (float*)&pp; float* G = (float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = G[k] * mult;
      M[k] = M[k] * b1 + gr * omb1;
      V[k] = V[k] * b2 + (gr * gr) * omb2;
      const float denom = sqrtf(V[k]) / bc2_sqrt + eps;
      P[k] = P[k] - step * (M[k] / denom);
    }
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

extern "C" long dis_adam_step_hyper_workspace(long count) {
  if (count <= 0 || count % 4 != 0) return -1;
  return adam_norm_blocks(count / 4);
}

extern "C" int dis_adam_step_hyper(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long count,
                                   const float* hyper, double beta1, double beta2, float eps, int* state, double* stats,
                                   double* partials, int mode, float grad_scale, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper || !state) return DIS_ERR_NULL;
  if (mode != 0 && (!stats || !partials)) return DIS_ERR_NULL;
  if (count <= 0) return DIS_ERR_BAD_SHAPE;
  if (count % 4 != 0) return DIS_ERR_UNSUPPORTED;
  if (mode & ~(ADAM_MODE_CLIP | ADAM_MODE_SKIP)) return DIS_ERR_UNSUPPORTED;
  const long count4 = count / 4, nparts = adam_norm_blocks(count4);
  if (nparts > 0x7fffffffL) return DIS_ERR_UNSUPPORTED;
  if (mode != 0)
    hipLaunchKernelGGL(adam_norm_partials_kernel, dim3((unsigned)nparts), dim3(ADAM_NORM_BLOCK), 0, (hipStream_t)stream,
                       (const float4*)grad, count4, grad_scale, partials);
  hipLaunchKernelGGL(adam_hyper_advance_kernel, dim3(1), dim3(mode != 0 ? ADAM_NORM_BLOCK : 1), 0, (hipStream_t)stream,
                     state, beta1, beta2, hyper, (const double*)partials, nparts, stats, mode);
  hipLaunchKernelGGL(adam_hyper_kernel, dim3(dis_ew_grid(count4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (float4*)param, (const float4*)grad, (float4*)exp_avg, (float4*)exp_avg_sq, count4, hyper,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, (const int*)state,
                     (const double*)stats, mode, grad_scale);
  DIS_CHECK_LAUNCH();
  return DIS_OK;
}
