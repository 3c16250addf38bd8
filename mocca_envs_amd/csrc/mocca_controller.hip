// mocca_controller.hip -- the base controller of the planner envs on the device: actor and critic MLPs for all N envs in ONE launch
// (mocca_plan_step runs it ahead of the step kernel).  Layout of the parameters: mocca_controller.h.
//
// Arithmetic: f32 in, f32 accumulate on the matrix cores (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain), because the
// reference runs this network in torch f32 and the critic's value enters the reward.
//
// A workgroup of four waves owns CTRL_TILE envs of ONE net (blockIdx.y: 0 actor, 1 critic -- the nets share nothing but the input).  The
// activations of the tile stay in LDS from the input to the head, X[env][feature], two buffers (layer l reads one, writes the other: one
// barrier per layer); the weights stream from L2 in fragment order.  Per layer the 16-row output tiles are dealt to the waves round
// robin (wave w: tiles w, w + 4, w + 8, w + 12), so no weight is read twice by a workgroup; Y^T = W X^T: the A operand is the weight
// fragment, the B operand one ds_read_b128 of the activations that serves four MFMAs and every output tile of the wave.
// Summation: an output is the sum of FOUR partial sums, one accumulator per MFMA j of a 16-wide k-group (the k with k mod 4 = j), each in
// ascending k, added as (p0 + p1) + (p2 + p3) ahead of the bias: chains a quarter as long as one running sum's and about half its rounding
// error -- what a blocked CPU GEMM's summation gives (the reference's torch forward is the yardstick of tests/test_gpu_planner_controller.py).
// The order does not depend on N: same inputs -> same bits.  No atomics, no host state.  The layer loop itself is mocca_mlp.h's mfma_layer,
// which the policy kernel and PPO's gradient run too; this kernel's own are the input stage and the head's store.
#include <hip/hip_runtime.h>

#include "mocca_controller.h"
#include "mocca_mlp.h"

namespace mocca_ctrl {

using namespace mocca_mlp;    // f32x4, mfma_layer, activate, normalise

constexpr int LDS_STRIDE = CTRL_MAX_WIDTH + 4;   // floats per env row: 16-byte aligned rows, rows 0..7 start on different bank groups
constexpr int IN_PAD = 80;                       // the 65-float input, padded to the MFMA tile
constexpr int TILE = CTRL_TILE;
static_assert(TILE == 16, "one 16-env MFMA sub-tile per workgroup: mfma_layer's 16 columns");

__global__ __launch_bounds__(256, 2) void controller_kernel(ControllerArgs a) {
  __shared__ __attribute__((aligned(16))) float X[2][TILE * LDS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int env0 = blockIdx.x * TILE, net = blockIdx.y;
  const int col = lane & 15;

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
    if (norm && env < a.n_envs && k < CTRL_IN) v = normalise(v, a.norm_mean[k], a.norm_inv_std[k], a.norm_clip);
    X[0][e * LDS_STRIDE + k] = v;
  }
  __syncthreads();

  const int first = net == 0 ? 0 : a.n_actor, count = net == 0 ? a.n_actor : a.n_critic;
  int cur = 0;
#pragma unroll 1
  for (int li = 0; li < count; ++li) {
    const int32_t* lr = a.layers + (size_t)(first + li) * CTRL_LAYER_WORDS;
    const int out_dim = lr[CL_OUT], act = lr[CL_ACT];
    const float* B = a.params + lr[CL_B_OFF];
    float* Xout = X[cur ^ 1];
    const bool head = li == count - 1;
    // epilogue: bias, activation, then LDS (next layer) or, from the accumulators' lanes, the outputs (head)
    mfma_layer<LDS_STRIDE>((const f32x4*)(a.params + lr[CL_W_OFF]), lr[CL_IN_PAD] >> 4, lr[CL_OUT_PAD] >> 4, X[cur], wave, lane, [&](int o, f32x4 sum) {
      const f32x4 bias = *(const f32x4*)(B + o);
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = activate(sum[r] + bias[r], act);
      if (!head) {
        *(f32x4*)&Xout[col * LDS_STRIDE + o] = y;
      } else {
        const int env = env0 + col;
        if (env < a.n_envs) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (o + r < out_dim) {
              if (net == 0) a.action[(size_t)env * CTRL_ACTION + o + r] = y[r];
              else a.value[env] = y[r];
            }
        }
      }
    });
    __syncthreads();
    cur ^= 1;
  }
}

void launch_controller(hipStream_t s, const ControllerArgs& a) {
  hipLaunchKernelGGL(controller_kernel, dim3((a.n_envs + CTRL_TILE - 1) / CTRL_TILE, 2), dim3(256), 0, s, a);
}

}  // namespace mocca_ctrl
