// mocca_rollout.hip -- the end of a PPO rollout on the device (include/mocca.h mocca_gae / mocca_obs_stats): returns and advantages by GAE
// with proper time limits, the advantages' moments and normalisation, and the running observation statistics.  Arithmetic contract,
// layouts and summation orders: mocca_rollout.h.  Plain HIP, wave64, no MFMA, no atomics; every launch is asynchronous on the caller's
// stream, allocates nothing and reads nothing on the host.
//
// The recurrence is one multiply-add of work per env and step: the kernels are bound by the latency of their loads, so each keeps several
// independent loads in flight (GAE_UNROLL steps of a chain whose loads do not depend on it; eight rows of a feature's column).
#include "mocca_rollout.h"

// every f32 / f64 operation below is the IEEE operation written: a * b + c stays two roundings (the contract names each of them)
#pragma clang fp contract(off)

namespace mocca_ro {

__device__ __forceinline__ double wave_sum(double v) {   // a fixed tree over the 64 lanes: the same bits in every lane, every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(GAE_BLOCK) void gae_kernel(GaeArgs a) {
  __shared__ double WS[GAE_BLOCK / 64][2];
  const int e = blockIdx.x * GAE_BLOCK + threadIdx.x;
  const size_t N = (size_t)a.n_envs;
  const float g = a.g, c = a.c, s = a.s;
  double s1 = 0.0, s2 = 0.0;
  if (e < a.n_envs) {
    int t = a.n_steps - 1;
    float gae = 0.0f;
    float v_next = a.value[(size_t)(t + 1) * N + e];
    auto step = [&](size_t i, float r, float v, float m, float bm) {
      const float delta = ((r * s) + ((g * v_next) * m)) - v;
      gae = (delta + ((c * m) * gae)) * bm;
      if (a.adv) a.adv[i] = gae;
      if (a.returns) a.returns[i] = gae + v;
      const double d = (double)gae;
      s1 += d;
      s2 += d * d;
      v_next = v;
    };
#pragma unroll 1
    for (int k = a.n_steps % GAE_UNROLL; k > 0; --k, --t) {   // the ragged top of the rollout, then whole groups
      const size_t i = (size_t)t * N + e;
      step(i, a.rew[i], a.value[i], a.masks[i + N], a.bad_masks[i + N]);
    }
#pragma unroll 1
    for (; t >= 0; t -= GAE_UNROLL) {
      float r[GAE_UNROLL], v[GAE_UNROLL], m[GAE_UNROLL], bm[GAE_UNROLL];
#pragma unroll
      for (int j = 0; j < GAE_UNROLL; ++j) {
        const size_t i = (size_t)(t - j) * N + e;
        r[j] = a.rew[i]; v[j] = a.value[i]; m[j] = a.masks[i + N]; bm[j] = a.bad_masks[i + N];
      }
#pragma unroll
      for (int j = 0; j < GAE_UNROLL; ++j) step((size_t)(t - j) * N + e, r[j], v[j], m[j], bm[j]);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { WS[wave][0] = s1; WS[wave][1] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p1 = WS[0][0], p2 = WS[0][1];
#pragma unroll
    for (int w = 1; w < GAE_BLOCK / 64; ++w) { p1 += WS[w][0]; p2 += WS[w][1]; }
    a.partials[2 * (size_t)blockIdx.x] = p1;
    a.partials[2 * (size_t)blockIdx.x + 1] = p2;
  }
}

__global__ __launch_bounds__(NORM_BLOCK) void moments_kernel(MomentsArgs a) {
  __shared__ double P[2 * NORM_BLOCK];
  __shared__ float MS[2];
  const int tid = threadIdx.x;
  double S1 = 0.0, S2 = 0.0;
  for (int base = 0; base < a.n_partials; base += NORM_BLOCK) {   // staged through LDS NORM_BLOCK pairs at a time, added in index order
    if (base + tid < a.n_partials) {
      P[2 * tid] = a.partials[2 * (size_t)(base + tid)];
      P[2 * tid + 1] = a.partials[2 * (size_t)(base + tid) + 1];
    }
    __syncthreads();
    if (tid == 0) {
      const int m = a.n_partials - base < NORM_BLOCK ? a.n_partials - base : NORM_BLOCK;
      for (int j = 0; j < m; ++j) { S1 += P[2 * j]; S2 += P[2 * j + 1]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double B = (double)a.count;
    double ss = S2 - S1 * S1 / B;
    ss = ss > 0.0 ? ss : (ss == ss ? 0.0 : ss);          // rounding may leave a constant batch below zero; a NaN stays one
    const float mean = (float)(S1 / B), sd = (float)sqrt(ss / (B - 1.0));
    MS[0] = mean; MS[1] = sd;
    if (blockIdx.x == 0 && a.moments) { a.moments[0] = mean; a.moments[1] = sd; }
  }
  if (!a.normalise) return;
  __syncthreads();
  const float mean = MS[0], den = MS[1] + a.eps;
  const long long stride = (long long)gridDim.x * NORM_BLOCK;
  for (long long i = (long long)blockIdx.x * NORM_BLOCK + tid; i < a.count; i += stride) a.adv[i] = __fdiv_rn(a.adv[i] - mean, den);
}

__global__ __launch_bounds__(OBS_BLOCK) void obs_partials_kernel(ObsArgs a, int span) {
  __shared__ double L[2 * OBS_BLOCK];
  const int tid = threadIdx.x, k0 = tid & (span - 1), r = tid / span, sub = OBS_BLOCK / span;
  const long long row0 = (long long)blockIdx.x * a.rows_per_block;
  const long long row1 = row0 + a.rows_per_block < a.n_rows ? row0 + a.rows_per_block : a.n_rows;
  const size_t stride = (size_t)a.row_stride;
  for (int k = k0; k < a.dim; k += OBS_BLOCK) {          // (a second pass only where dim > OBS_BLOCK: then span = OBS_BLOCK, every thread has k0 < dim)
    const double mu = a.state[1 + k];
    const float* col = a.rows + k;
    double sd = 0.0, sdd = 0.0;
    long long row = row0 + r;
    for (; row + 7ll * sub < row1; row += 8ll * sub) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = col[(size_t)(row + (long long)j * sub) * stride];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double d = (double)x[j] - mu;
        sd += d;
        sdd += d * d;
      }
    }
    for (; row < row1; row += sub) {
      const double d = (double)col[(size_t)row * stride] - mu;
      sd += d;
      sdd += d * d;
    }
    if (sub == 1) {
      double* out = a.partials + ((size_t)blockIdx.x * a.dim + k) * 2;
      out[0] = sd; out[1] = sdd;
    } else {
      L[2 * tid] = sd; L[2 * tid + 1] = sdd;
    }
  }
  if (sub == 1) return;                                  // (uniform over the workgroup)
  if (k0 >= a.dim) { L[2 * tid] = 0.0; L[2 * tid + 1] = 0.0; }
  __syncthreads();
  if (r == 0 && k0 < a.dim) {                            // the sub-rows of feature k0, in index order
    double sd = L[2 * k0], sdd = L[2 * k0 + 1];
    for (int j = 1; j < sub; ++j) { sd += L[2 * (j * span + k0)]; sdd += L[2 * (j * span + k0) + 1]; }
    double* out = a.partials + ((size_t)blockIdx.x * a.dim + k0) * 2;
    out[0] = sd; out[1] = sdd;
  }
}

__global__ __launch_bounds__(OBS_MERGE_BLOCK) void obs_merge_kernel(ObsArgs a, int span) {
  __shared__ double L[2 * OBS_MERGE_BLOCK];
  const int tid = threadIdx.x, k = tid & (span - 1), grp = tid / span, groups = OBS_MERGE_BLOCK / span;
  const double count = a.state[0];
  const int per = (a.n_blocks + groups - 1) / groups;
  const int b0 = grp * per, b1 = b0 + per < a.n_blocks ? b0 + per : a.n_blocks;
  double sd = 0.0, sdd = 0.0;
  if (k < a.dim) {
    const double* p = a.partials + 2 * (size_t)k;
    const size_t bs = 2 * (size_t)a.dim;
    int b = b0;
    for (; b + 3 < b1; b += 4) {
      double u[4], w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { u[j] = p[(size_t)(b + j) * bs]; w[j] = p[(size_t)(b + j) * bs + 1]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) { sd += u[j]; sdd += w[j]; }
    }
    for (; b < b1; ++b) { sd += p[(size_t)b * bs]; sdd += p[(size_t)b * bs + 1]; }
  }
  L[2 * tid] = sd; L[2 * tid + 1] = sdd;
  __syncthreads();
  if (grp != 0 || k >= a.dim) return;
  for (int j = 1; j < groups; ++j) { sd += L[2 * (j * span + k)]; sdd += L[2 * (j * span + k) + 1]; }
  const double n = (double)a.n_rows, mean = a.state[1 + k], var = a.state[1 + a.dim + k];
  const double md = sd / n;
  const double bmean = mean + md, bvar = sdd / n - md * md;
  const double delta = bmean - mean, tot = count + n;
  const double mean2 = mean + delta * n / tot;
  const double var2 = (var * count + bvar * n + delta * delta * count * n / tot) / tot;
  a.state[1 + k] = mean2;
  a.state[1 + a.dim + k] = var2;
  if (k == 0) a.state[0] = tot;
  if (a.mean_out) a.mean_out[k] = (float)mean2;
  if (a.inv_std_out) a.inv_std_out[k] = __fdiv_rn(1.0f, sqrtf((float)var2 + a.eps));
}

void launch_gae(hipStream_t s, const GaeArgs& a) {
  hipLaunchKernelGGL(gae_kernel, dim3(gae_blocks(a.n_envs)), dim3(GAE_BLOCK), 0, s, a);
}

void launch_moments(hipStream_t s, const MomentsArgs& a) {
  long long blocks = 1;
  if (a.normalise) {
    blocks = (a.count + (long long)NORM_BLOCK * NORM_PER_THREAD - 1) / ((long long)NORM_BLOCK * NORM_PER_THREAD);
    blocks = blocks > NORM_MAX_BLOCKS ? NORM_MAX_BLOCKS : blocks;
  }
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)blocks), dim3(NORM_BLOCK), 0, s, a);
}

void launch_obs_stats(hipStream_t s, const ObsArgs& a) {
  hipLaunchKernelGGL(obs_partials_kernel, dim3(a.n_blocks), dim3(OBS_BLOCK), 0, s, a, obs_span(a.dim, OBS_BLOCK));
  hipLaunchKernelGGL(obs_merge_kernel, dim3(1), dim3(OBS_MERGE_BLOCK), 0, s, a, obs_span(a.dim, OBS_MERGE_BLOCK));
}

}  // namespace mocca_ro
