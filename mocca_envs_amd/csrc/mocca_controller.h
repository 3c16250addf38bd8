// mocca_controller.h -- layout of the planner envs' base controller as the controller kernel reads it (mocca_controller.hip), and the
// host-side launcher.  mocca_set_base_controller (mocca_api_policy.hip) checks the caller's plain row-major layers and has the repack kernel
// (mocca_policy.hip) build this image on the device.
//
// The base controller of Walker3DPlannerEnv / MikePlannerEnv (env_locomotion.py:1029-1040, :1091-1101) is an actor-critic pair of MLPs over
// one 65-float input, [robot_state(50), plan(15) * action_scale]: the actor's 21 outputs are the joint actions of the step, the critic's one
// output enters the reward.
//
// Layer table: n_layers_total rows of CTRL_LAYER_WORDS int32, the actor's layers first (input to head), then the critic's.
// Parameters: one f32 array; a layer's weights at w_off, its bias at b_off (float offsets, multiples of 4: 16-byte loads).
//   weights  [out_pad / 16][in_pad / 16][64][4]: the float4 of lane l in block (ot, kg) is W[16 ot + (l & 15)][16 kg + 4 (l >> 4) + 0..3] --
//            the A operands of four consecutive v_mfma_f32_16x16x4_f32 of one wave, so that a wave's weight load is one coalesced 1 KB read
//   bias     [out_pad]
// in_pad / out_pad round the widths up to the 16 x 16 MFMA tile (65 -> 80, 21 -> 32, 1 -> 16); the padding is zeros and every activation
// maps 0 to 0, so padded rows and columns add exact zeros.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocca_ctrl {

constexpr int CTRL_LAYER_WORDS = 8;
enum : int { CL_NET = 0, CL_IN = 1, CL_OUT = 2, CL_IN_PAD = 3, CL_OUT_PAD = 4, CL_ACT = 5, CL_W_OFF = 6, CL_B_OFF = 7 };
enum : int { CTRL_ACT_IDENTITY = 0, CTRL_ACT_RELU = 1, CTRL_ACT_TANH = 2, CTRL_ACT_SOFTSIGN = 3 };
constexpr int CTRL_ROBOT_STATE = 50, CTRL_PLAN = 15, CTRL_IN = CTRL_ROBOT_STATE + CTRL_PLAN, CTRL_ACTION = 21;
constexpr int CTRL_MAX_WIDTH = 256, CTRL_MAX_LAYERS = 8;
constexpr int CTRL_RS_STRIDE = 64;   // floats per env of the handle's robot_state buffer (256-byte rows)

struct ControllerArgs {
  const float* params;          // device
  const int32_t* layers;        // device, [n_actor + n_critic][CTRL_LAYER_WORDS]
  int n_actor, n_critic;
  const float* robot_state;     // [N][CTRL_RS_STRIDE]
  const float* plan;            // [N][CTRL_PLAN]
  float action_scale;
  float* action;                // [N][CTRL_ACTION], not clipped (apply_action clips, robots.py:33)
  float* value;                 // [N]
  int n_envs;
  // observation statistics of a controller trained by this project's PPO (mocca_set_base_controller_norm), or norm_mean == null: each of the
  // 65 inputs becomes clamp((v - norm_mean[k]) * norm_inv_std[k], -norm_clip, +norm_clip) after the scale and before both nets
  const float* norm_mean;       // device, [CTRL_IN]
  const float* norm_inv_std;    // device, [CTRL_IN]
  float norm_clip;
};

constexpr int CTRL_TILE = 16;        // envs per workgroup (32 and 64 measured slower at 4096 envs: profiles/HISTORY.md)
void launch_controller(hipStream_t s, const ControllerArgs& a);

}  // namespace mocca_ctrl
