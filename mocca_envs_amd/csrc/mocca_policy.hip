// mocca_policy.hip -- a trainer's Gaussian actor-critic on the device: observation normalisation, actor and critic MLPs, the action sample,
// its log-probability and the value for all N envs in ONE launch (mocca_act; mocca_act_step runs it ahead of the step kernel).  Layout of the
// parameters and the keying of the in-kernel noise: mocca_policy.h.
//
// Arithmetic: the controller kernel's contract (mocca_controller.hip).  f32 in, f32 accumulate on the matrix cores
// (v_mfma_f32_16x16x4_f32); an output is the sum of FOUR partial sums, one accumulator per MFMA j of a 16-wide k-group (the k with
// k mod 4 = j), each in ascending k, added as (p0 + p1) + (p2 + p3) ahead of the bias and the activation.  The layer loop is the one that
// kernel and mocca_ppo.hip run too (mocca_mlp.h: mfma_layer), here over a wider LDS row than the controller's (the input may be
// [obs | scan], up to 336 floats).
//
// A workgroup of four waves owns POL_TILE envs of ONE net (blockIdx.y: 0 actor, 1 critic).  The activations of the tile stay in LDS from the
// normalised input to the head, X[env][feature], two buffers; the weights stream from L2 in fragment order.  The head's outputs go to LDS
// like a hidden layer's; then ONE lane per env forms, in ascending j,
//     action[j] = mean[j] + exp(log_std[j]) * eps[j]            logp = sum_j ( -1/2 eps[j]^2 - log_std[j] - 1/2 log 2 pi )
// (actor workgroups) or stores the value (critic workgroups).  The in-kernel noise of the tile is drawn by all 256 lanes (16 envs x 16 Philox
// blocks of two normals) ahead of the layers.  The order of every sum is fixed and does not depend on N: same inputs -> same bits.  No
// atomics, no host state.
//
// The mirror-symmetric instance (SYM; header: Symmetry) gives the 16 MFMA columns to 8 envs x {as given, mirrored}: the staging writes column
// 8 + c from the raw row of env c through in_perm / in_sign ahead of the same normalisation, the layer loop is the plain one, and the head
// stage's lane folds the two columns of its env into one mean (or value).
#include <hip/hip_runtime.h>

#include "mocca_mlp.h"
#include "mocca_philox.h"
#include "mocca_policy.h"

namespace mocca_pol {

using namespace mocca_ctrl;   // CL_*, CTRL_ACT_*
using namespace mocca_mlp;   // f32x4, mfma_layer, activate, normalise

constexpr int LDS_STRIDE = POL_MAX_IN + 4;   // floats per env row: 16-byte aligned rows, rows 0..7 start on different bank groups (340 = 20 mod 32)
constexpr int TILE = POL_TILE;          // MFMA columns of a workgroup: 16 envs, or (SYM) POL_SYM_TILE envs and their mirror images
static_assert(TILE == 16, "one 16-env MFMA sub-tile per workgroup; the noise stage deals 16 envs x 16 Philox blocks to 256 lanes");
static_assert(2 * POL_SYM_TILE == TILE, "the symmetric instance: column c the env as given, column POL_SYM_TILE + c its mirror image");
static_assert(POL_MAX_WIDTH <= POL_MAX_IN && POL_MAX_ACTION <= 32, "LDS rows hold the widest layer; 16 Philox blocks give 32 normals");

// PRIV (header: Privileged critic): the plain layout with the critic's workgroups staging their own rows under their own statistics
template <bool SYM, bool PRIV = false>
__global__ __launch_bounds__(256, 2) void policy_kernel(PolicyArgs a) {
  static_assert(!(SYM && PRIV), "the privileged critic has no mirror tables");
  constexpr int ENVS = SYM ? POL_SYM_TILE : TILE;   // envs of a workgroup
  __shared__ __attribute__((aligned(16))) float X[2][TILE * LDS_STRIDE];
  __shared__ float Z[ENVS * POL_MAX_ACTION];   // the tile's noise, Z[env][j]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int env0 = blockIdx.x * ENVS, net = blockIdx.y;
  const int col = lane & 15;

  // input: the first in_dim floats of the env's row, normalised, zeros up to in_pad; rows past the batch are zeros (nothing of them is stored).
  // SYM: column e >= ENVS is the mirror image of env e - ENVS, formed from the RAW row (the statistics are not symmetric) and normalised by k
  // PRIV: a second copy of the loop, not one loop over parameters -- folded into one lambda the two moved instructions in both existing
  // instances, which are held to the instruction streams they had (profiles/kernel_resources_priv_critic.md)
  if (PRIV && net == 1) {   // the critic's own rows and statistics: the loop below, field for field
    const bool norm = a.params[a.flags_off] != 0.0f;
    const float *mu = a.params + a.critic_mean_off, *is = a.params + a.critic_inv_std_off;
    for (int i = tid; i < TILE * a.critic_in_pad; i += 256) {
      const int e = i / a.critic_in_pad, k = i - e * a.critic_in_pad, env = env0 + e;
      float v = 0.0f;
      if (env < a.n_envs && k < a.critic_in_dim) {
        v = a.critic_in[(size_t)env * a.critic_stride + k];
        if (norm) v = normalise(v, mu[k], is[k], a.clip);
      }
      X[0][e * LDS_STRIDE + k] = v;
    }
  } else {
    const bool norm = a.params[a.flags_off] != 0.0f;
    const float *mu = a.params + a.mean_off, *is = a.params + a.inv_std_off;
    for (int i = tid; i < TILE * a.in_pad; i += 256) {
      const int e = i / a.in_pad, k = i - e * a.in_pad, env = env0 + (SYM ? e & (ENVS - 1) : e);
      float v = 0.0f;
      if (env < a.n_envs && k < a.in_dim) {
        if (SYM && e >= ENVS) v = a.in[(size_t)env * a.in_stride + a.in_perm[k]] * a.in_sign[k];
        else v = a.in[(size_t)env * a.in_stride + k];
        if (norm) v = normalise(v, mu[k], is[k], a.clip);
      }
      X[0][e * LDS_STRIDE + k] = v;
    }
  }
  // in-kernel noise (header: Noise): lane (env e = tid / 16, block p = tid % 16) draws the normals 2 p and 2 p + 1 of env e
  if (net == 0 && !a.deterministic && !a.eps) {
    const int e = tid >> 4, p = tid & 15, env = env0 + e;
    if (e < ENVS && env < a.n_envs && 2 * p < a.act_dim) {
      const uint32_t* tk = a.task + (size_t)env * a.task_words;
      uint32_t w[4];
      philox4x32(16u * (uint32_t)(a.env_offset + env) + (uint32_t)p, tk[a.tw_t], tk[a.tw_episode], 1u, a.seed_lo, a.seed_hi, w);
      const float u1 = (float)((w[0] >> 8) + 1u) * (1.0f / 16777216.0f), u2 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);
      const float r = sqrtf(-2.0f * logf(u1)), th = 6.28318530717958647692f * u2;
      Z[e * POL_MAX_ACTION + 2 * p] = r * cosf(th);
      Z[e * POL_MAX_ACTION + 2 * p + 1] = r * sinf(th);
    }
  }
  __syncthreads();

  const int first = net == 0 ? 0 : a.n_actor, count = net == 0 ? a.n_actor : a.n_critic;
  int cur = 0;
#pragma unroll 1
  for (int li = 0; li < count; ++li) {
    const int32_t* lr = a.layers + (size_t)(first + li) * CTRL_LAYER_WORDS;
    const int act = lr[CL_ACT];
    const float* B = a.params + lr[CL_B_OFF];
    float* Xout = X[cur ^ 1];
    // epilogue: bias, activation, then LDS (the next layer, or the head stage)
    mfma_layer<LDS_STRIDE>((const f32x4*)(a.params + lr[CL_W_OFF]), lr[CL_IN_PAD] >> 4, lr[CL_OUT_PAD] >> 4, X[cur], wave, lane, [&](int o, f32x4 sum) {
      const f32x4 bias = *(const f32x4*)(B + o);
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = activate(sum[r] + bias[r], act);
      *(f32x4*)&Xout[col * LDS_STRIDE + o] = y;
    });
    __syncthreads();
    cur ^= 1;
  }

  // head stage: one lane per env
  const int env = env0 + tid;
  if (tid >= ENVS || env >= a.n_envs) return;
  const float* head = &X[cur][tid * LDS_STRIDE];
  const float* mirror = &X[cur][(SYM ? ENVS + tid : tid) * LDS_STRIDE];   // SYM: the head of the env's mirrored column
  if (net == 1) {
    a.value[env] = SYM ? 0.5f * (head[0] + mirror[0]) : head[0];
    return;
  }
  const float* log_std = a.params + a.log_std_off;
  const int A = a.act_dim;
  float lp = 0.0f;
  for (int j = 0; j < A; ++j) {
    float m = head[j], ls = log_std[j];
    if (SYM) {   // header: Symmetry -- one f32 operation per line of it, in that order
      const int pj = a.act_perm[j];
      const float mm = mirror[pj] * a.act_sign[j];
      m = 0.5f * (m + mm);
      ls = 0.5f * (ls + log_std[pj]);
    }
    float e = 0.0f, act = m;
    if (!a.deterministic) {
      e = a.eps ? a.eps[(size_t)env * A + j] : Z[tid * POL_MAX_ACTION + j];
      act = m + expf(ls) * e;
    }
    lp += (-0.5f * e) * e - ls - 0.91893853320467274178f;
    a.action[(size_t)env * A + j] = act;
    if (a.mean) a.mean[(size_t)env * A + j] = m;
  }
  if (a.logp) a.logp[env] = lp;
}

// plain row-major parameters -> the image (header: Image); one thread per image float
__global__ __launch_bounds__(256) void repack_kernel(RepackArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.image_floats) return;
  float v = 0.0f;
  for (int r = 0; r < a.n_rows; ++r) {
    const RepackRow& row = a.rows[r];
    if (i < row.dst || i >= row.dst_end) continue;
    const int idx = i - row.dst;
    if (row.src < 0) { v = idx < row.out ? row.fill : 0.0f; break; }   // a constant in the first `out` floats
    if (row.in_pad == 0) {   // a plain array, zero padded
      v = idx < row.out ? a.src[row.src + idx] : 0.0f;
      break;
    }
    // weights: [ot][kg][lane][4], the float4 of lane l in block (ot, kg) is W[16 ot + (l & 15)][16 kg + 4 (l >> 4) + 0..3]
    const int nkg = row.in_pad >> 4;
    const int ot = idx / (nkg * 256), rem = idx - ot * nkg * 256, kg = rem >> 8, l = (rem & 255) >> 2, j = rem & 3;
    const int orow = 16 * ot + (l & 15), k = 16 * kg + 4 * (l >> 4) + j;
    // transposed (mocca_ppo.h: Image): the row's matrix is the source's transpose, its element [orow][k] the source's [k][orow]
    const size_t at = row.transposed ? (size_t)k * row.out + orow : (size_t)orow * row.in + k;
    v = orow < row.out && k < row.in ? a.src[row.src + at] : 0.0f;
    break;
  }
  a.image[i] = v;
}

void launch_policy(hipStream_t s, const PolicyArgs& a) {
  if (a.in_perm) hipLaunchKernelGGL((policy_kernel<true>), dim3((a.n_envs + POL_SYM_TILE - 1) / POL_SYM_TILE, a.value ? 2 : 1), dim3(256), 0, s, a);
  else if (a.critic_in_dim) hipLaunchKernelGGL((policy_kernel<false, true>), dim3((a.n_envs + TILE - 1) / TILE, a.value ? 2 : 1), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((policy_kernel<false>), dim3((a.n_envs + TILE - 1) / TILE, a.value ? 2 : 1), dim3(256), 0, s, a);
}

void launch_repack(hipStream_t s, const RepackArgs& a) {
  hipLaunchKernelGGL(repack_kernel, dim3((a.image_floats + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mocca_pol
