// mocca_controller.hip -- the base controller of the planner envs on the device: actor and critic MLPs for all N envs in ONE launch
// (mocca_plan_step runs it ahead of the step kernel).  Layout of the parameters: mocca_controller.h.
//
// Arithmetic: f32 in, f32 accumulate on the matrix cores (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain), because the
// reference runs this network in torch f32 and the critic's value enters the reward.
//
// A workgroup of four waves owns TILE envs of ONE net (blockIdx.y: 0 actor, 1 critic -- the nets share nothing but the input).  The
// activations of the tile stay in LDS from the input to the head, X[env][feature], two buffers (layer l reads one, writes the other: one
// barrier per layer); the weights stream from L2 in fragment order.  Per layer the 16-row output tiles are dealt to the waves round
// robin (wave w: tiles w, w + 4, w + 8, w + 12), so no weight is read twice by a workgroup; Y^T = W X^T: the A operand is the weight
// fragment, the B operand one ds_read_b128 of the activations that serves four MFMAs and every output tile of the wave.
// Summation: an output is the sum of FOUR partial sums, one accumulator per MFMA j of a 16-wide k-group (the k with k mod 4 = j), each in
// ascending k, added as (p0 + p1) + (p2 + p3) ahead of the bias: chains a quarter as long as one running sum's and about half its rounding
// error -- what a blocked CPU GEMM's summation gives (the reference's torch forward is the yardstick of tests/test_gpu_planner_controller.py).
// The order does not depend on N: same inputs -> same bits.  No atomics, no host state.
#include <hip/hip_runtime.h>

#include "mocca_controller.h"

namespace mocca_ctrl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDS_STRIDE = CTRL_MAX_WIDTH + 4;   // floats per env row: 16-byte aligned rows, rows 0..7 start on different bank groups
constexpr int IN_PAD = 80;                       // the 65-float input, padded to the MFMA tile
constexpr int NP = 4;                            // partial sums per output (header comment: Summation)
constexpr int NT = 4;                            // output tiles per wave: 16 tiles of 16 rows (width 256) over 4 waves

__device__ __forceinline__ float activate(float x, int act) {
  switch (act) {
    case CTRL_ACT_RELU: return fmaxf(x, 0.0f);
    case CTRL_ACT_TANH: return tanhf(x);
    case CTRL_ACT_SOFTSIGN: return x / (1.0f + fabsf(x));
    default: return x;
  }
}

template <int TILE>
__global__ __launch_bounds__(256, 2) void controller_kernel(ControllerArgs a) {
  constexpr int ES = TILE / 16;   // 16-env sub-tiles: each weight fragment is used ES times
  __shared__ __attribute__((aligned(16))) float X[2][TILE * LDS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int env0 = blockIdx.x * TILE, net = blockIdx.y;
  const int col = lane & 15, quad = lane >> 4;

  // input: [robot_state(50), plan(15) * action_scale, zeros]; rows past the batch are zeros (their outputs are not stored).  With
  // observation statistics attached (norm_mean != null: wave-uniform) the 65 entries are normalised by the policy kernel's line
  // (mocca_policy.hip: input), the padding stays zeros
  const bool norm = a.norm_mean != nullptr;
  for (int i = tid; i < TILE * IN_PAD; i += 256) {
    const int e = i / IN_PAD, k = i - e * IN_PAD, env = env0 + e;
    float v = 0.0f;
    if (env < a.n_envs) {
      if (k < CTRL_ROBOT_STATE) v = a.robot_state[(size_t)env * CTRL_RS_STRIDE + k];
      else if (k < CTRL_IN) v = a.plan[(size_t)env * CTRL_PLAN + (k - CTRL_ROBOT_STATE)] * a.action_scale;
    }
    if (norm && env < a.n_envs && k < CTRL_IN) v = fminf(fmaxf((v - a.norm_mean[k]) * a.norm_inv_std[k], -a.norm_clip), a.norm_clip);
    X[0][e * LDS_STRIDE + k] = v;
  }
  __syncthreads();

  const int first = net == 0 ? 0 : a.n_actor, count = net == 0 ? a.n_actor : a.n_critic;
  int cur = 0;
#pragma unroll 1
  for (int li = 0; li < count; ++li) {
    const int32_t* lr = a.layers + (size_t)(first + li) * CTRL_LAYER_WORDS;
    const int nkg = lr[CL_IN_PAD] >> 4, n_ot = lr[CL_OUT_PAD] >> 4, out_dim = lr[CL_OUT], act = lr[CL_ACT];
    const f32x4* W = (const f32x4*)(a.params + lr[CL_W_OFF]);
    const float* B = a.params + lr[CL_B_OFF];
    const int nt_w = wave < n_ot ? (n_ot - wave + 3) >> 2 : 0;   // output tiles of this wave (wave-uniform)
    const float* Xin = X[cur];
    float* Xout = X[cur ^ 1];

    f32x4 acc[NT][ES][NP];   // [..][j]: the partial sum fed by MFMA j of every k-group
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int es = 0; es < ES; ++es)
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[t][es][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (nt_w > 0) {
      // weight fragments of this wave's tiles at k-group kg (tiles past the wave's last re-read that one: loaded, never multiplied)
      const f32x4* wp[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int ot = wave + 4 * (t < nt_w ? t : nt_w - 1);
        wp[t] = W + (size_t)ot * nkg * 64 + lane;
      }
      // the weights come from L2 (hundreds of cycles): the fragments of k-groups kg + 1 and kg + 2 are in flight while kg multiplies
      f32x4 w0[NT], w1[NT], w2[NT];
      auto load = [&](f32x4 (&w)[NT], int kg) {
        const int kc = kg < nkg ? kg : nkg - 1;
#pragma unroll
        for (int t = 0; t < NT; ++t) w[t] = wp[t][(size_t)kc * 64];
      };
      auto multiply = [&](const f32x4 (&w)[NT], int kg) {
        f32x4 b[ES];
#pragma unroll
        for (int es = 0; es < ES; ++es) b[es] = *(const f32x4*)&Xin[(es * 16 + col) * LDS_STRIDE + kg * 16 + quad * 4];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (t < nt_w) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int es = 0; es < ES; ++es) acc[t][es][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][j], b[es][j], acc[t][es][j], 0, 0, 0);
          }
      };
      // three k-groups per trip: the three fragment sets rotate by name, not by register moves
      load(w0, 0); load(w1, 1);
#pragma unroll 1
      for (int kg = 0; kg < nkg; kg += 3) {
        load(w2, kg + 2); multiply(w0, kg);
        if (kg + 1 >= nkg) break;
        load(w0, kg + 3); multiply(w1, kg + 1);
        if (kg + 2 >= nkg) break;
        load(w1, kg + 4); multiply(w2, kg + 2);
      }
      // epilogue: lane holds rows 16 ot + 4 quad + 0..3 of env column `col`; bias, activation, then LDS (next layer) or the outputs (head)
      const bool head = li == count - 1;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nt_w) {
          const int o = (wave + 4 * t) * 16 + quad * 4;
          const f32x4 bias = *(const f32x4*)(B + o);
#pragma unroll
          for (int es = 0; es < ES; ++es) {
            const f32x4 sum = (acc[t][es][0] + acc[t][es][1]) + (acc[t][es][2] + acc[t][es][3]);
            f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = activate(sum[r] + bias[r], act);
            if (!head) {
              *(f32x4*)&Xout[(es * 16 + col) * LDS_STRIDE + o] = y;
            } else {
              const int env = env0 + es * 16 + col;
              if (env < a.n_envs) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (o + r < out_dim) {
                    if (net == 0) a.action[(size_t)env * CTRL_ACTION + o + r] = y[r];
                    else a.value[env] = y[r];
                  }
              }
            }
          }
        }
    }
    __syncthreads();
    cur ^= 1;
  }
}

void launch_controller(hipStream_t s, const ControllerArgs& a) {
  hipLaunchKernelGGL(controller_kernel<CTRL_TILE>, dim3((a.n_envs + CTRL_TILE - 1) / CTRL_TILE, 2), dim3(256), 0, s, a);
}

}  // namespace mocca_ctrl
