// mocca_optim.hip -- clip_grad_norm_, Adam's step and the epoch's shuffle of a PPO update on the device (include/mocca.h mocca_adam_step /
// mocca_ppo_update).  Arithmetic contract, layouts and the order of sums: mocca_optim.h.  Plain HIP, wave64, no MFMA, no atomics; every launch
// is asynchronous on the caller's stream, allocates nothing and reads nothing on the host.
#include "mocca_optim.h"

#include "mocca_philox.h"

// every f32 / f64 operation below is the IEEE operation written: a * b + c stays two roundings (the contract names each of them)
#pragma clang fp contract(off)

namespace mocca_optim {

constexpr int NORM_UNROLL = 16;   // loads in flight per thread of launch A; the adds keep their ascending order

// launch A (header): one workgroup
__global__ __launch_bounds__(OPT_BLOCK) void adam_norm_kernel(AdamArgs a) {
  __shared__ double sq[OPT_BLOCK];
  const int tid = threadIdx.x, n = a.n_params;
  double s = 0.0;
  int i = tid;
#pragma unroll 1
  for (; i + (NORM_UNROLL - 1) * OPT_BLOCK < n; i += NORM_UNROLL * OPT_BLOCK) {
    float g[NORM_UNROLL];
#pragma unroll
    for (int k = 0; k < NORM_UNROLL; ++k) g[k] = a.grad[i + k * OPT_BLOCK];
#pragma unroll
    for (int k = 0; k < NORM_UNROLL; ++k) s += (double)g[k] * (double)g[k];
  }
  for (; i < n; i += OPT_BLOCK) { const double g = (double)a.grad[i]; s += g * g; }
  sq[tid] = s;
  __syncthreads();
  for (int h = OPT_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) sq[tid] += sq[tid + h];
    __syncthreads();
  }
  if (tid != 0) return;
  const double S = sq[0];
  AdamRecord r{};
  if (!isfinite(S)) {   // the step is skipped: launch B writes nothing
    r.skip = 1;
    *a.rec = r;
    a.clock[3] = a.clock[3] + 1.0;
    if (a.stats) a.stats[6] = 0.0f;
    return;
  }
  const double nrm = sqrt(S);
  r.coef = a.max_grad_norm > 0.0 ? (float)fmin(1.0, a.max_grad_norm / (nrm + 1e-6)) : 1.0f;
  const double p1 = a.clock[1] * a.beta1, p2 = a.clock[2] * a.beta2;
  a.clock[0] = a.clock[0] + 1.0;
  a.clock[1] = p1;
  a.clock[2] = p2;
  r.ss = (float)(a.lr / (1.0 - p1));
  r.bc = (float)sqrt(1.0 - p2);
  r.b2 = (float)a.beta2;
  r.w1 = (float)(1.0 - a.beta1);
  r.w2 = (float)(1.0 - a.beta2);
  r.e = (float)a.eps;
  *a.rec = r;
  if (a.stats) a.stats[6] = r.coef;
}

// launch B (header): thread i steps params[i]
__global__ __launch_bounds__(OPT_BLOCK) void adam_apply_kernel(AdamArgs a) {
  const int i = blockIdx.x * OPT_BLOCK + threadIdx.x;
  const AdamRecord r = *a.rec;
  if (r.skip || i >= a.n_params) return;
  float m = a.m[i], v = a.v[i], p = a.params[i];
  const float g = a.grad[i] * r.coef;
  float d = g - m;
  d = d * r.w1;
  m = m + d;
  v = v * r.b2;
  float q = g * g;
  q = q * r.w2;
  v = v + q;
  float s = sqrtf(v);
  s = __fdiv_rn(s, r.bc);
  s = s + r.e;
  float u = __fdiv_rn(m, s);
  u = r.ss * u;
  p = p - u;
  a.m[i] = m;
  a.v[i] = v;
  a.params[i] = p;
}

// the shuffle (header): thread b writes perm[b]
__global__ __launch_bounds__(OPT_BLOCK) void shuffle_kernel(ShuffleArgs a) {
  const int b = blockIdx.x * OPT_BLOCK + threadIdx.x;
  if (b >= a.n) return;
  const unsigned long long t = (unsigned long long)a.clock[0];
  const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32);
  uint32_t x = (uint32_t)b;
  do {
    uint32_t L = x >> a.half, R = x & a.mask;
#pragma unroll 1
    for (uint32_t round = 0; round < (uint32_t)FEISTEL_ROUNDS; ++round) {
      uint32_t f[4];
      philox4x32(R, round, t_lo, t_hi, a.seed_lo, a.seed_hi, f);
      const uint32_t next = L ^ (f[0] & a.mask);
      L = R;
      R = next;
    }
    x = (L << a.half) | R;
  } while (x >= (uint32_t)a.n);
  a.perm[b] = (int64_t)x;
}

void launch_adam(hipStream_t s, const AdamArgs& a) {
  hipLaunchKernelGGL(adam_norm_kernel, dim3(1), dim3(OPT_BLOCK), 0, s, a);
  hipLaunchKernelGGL(adam_apply_kernel, dim3((a.n_params + OPT_BLOCK - 1) / OPT_BLOCK), dim3(OPT_BLOCK), 0, s, a);
}

void launch_shuffle(hipStream_t s, const ShuffleArgs& a) {
  hipLaunchKernelGGL(shuffle_kernel, dim3((a.n + OPT_BLOCK - 1) / OPT_BLOCK), dim3(OPT_BLOCK), 0, s, a);
}

}  // namespace mocca_optim
