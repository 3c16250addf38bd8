// mocca_policy.h -- layout of a trainer's Gaussian actor-critic as the policy kernel reads it (mocca_policy.hip), and the host-side launchers.
// mocca_set_policy (mocca_api_policy.hip) checks the caller's shapes and sizes this image; mocca_update_policy fills it from plain row-major
// parameters on the device (one repack kernel); mocca_act / mocca_act_step launch the kernel.
//
// The policy of a SymmetricRL / ALLSTEPS / a2c-ppo-acktr trainer: a diagonal-Gaussian actor (an MLP that gives the mean, a state-independent
// log_std), a critic MLP over the same input, and optionally a running observation normalisation in front of both.
//
// Layer table: the controller's (mocca_controller.h): n_layers_total rows of CTRL_LAYER_WORDS int32, the actor's layers first, then the
// critic's; w_off / b_off point into the image below.
// Image: one f32 array.
//   per layer   weights [out_pad / 16][in_pad / 16][64][4] in MFMA fragment order, then bias [out_pad] -- exactly the controller's layout
//   log_std     [POL_MAX_ACTION], zeros past act_dim
//   flags       [4]: flags[0] != 0: normalise the input (the repack kernel sets it when the caller's parameters carry mean / inv_std -- a
//               DEVICE word, so that an update between two replays of a captured launch switches it without a recapture)
//   mean        [in_pad], zeros past in_dim
//   inv_std     [in_pad], zeros past in_dim        x = clamp((x - mean[k]) * inv_std[k], -clip, +clip), f32, in that operation order
//   critic_mean, critic_inv_std   [critic_in_pad] each, zeros past critic_in_dim: ONLY in the image of a policy with a privileged critic
//               (below); a plain policy's image has neither and its offsets are what they were
//   transposed  behind everything above (the policy kernel reads none of it): the weights of every layer but a net's first once more,
//               transposed, for mocca_ppo_grad's backward (mocca_ppo.h: Image)
//
// Noise.  mocca_act has three modes: deterministic (eps = 0: the action is the mean), caller noise (eps_dev [N][act_dim]) and, the default,
// noise drawn in the kernel: Philox4x32-10 under the handle's seed key with the counter
//     ( 16 * env + (j >> 1),  task word MOCCA_TW_T,  task word MOCCA_TW_EPISODE,  1 )
// env = MOCCA_PARAM_ENV_OFFSET + index: the GLOBAL env id; the fourth word is 1 where the env's own draws (mocca_device.h rng_uniform) use 0,
// so the two streams never collide; word 0 is 32 bits wide, so global env ids stay below 2^28 (mocca_act refuses a handle whose ids reach it).
// Output words 0 and 1 give u1 = ((w0 >> 8) + 1) / 2^24 in (0, 1] and u2 = (w1 >> 8) / 2^24 in [0, 1);
// Box-Muller, r = sqrt(-2 log u1), gives eps[2 (j >> 1)] = r cos(2 pi u2) and eps[2 (j >> 1) + 1] = r sin(2 pi u2).  The noise is a function
// of device state only (seed, env id, the env's step and episode counters): the kernel keeps no host state and can be captured; a shard
// reproduces its rows of the whole batch; restoring state and task replays the noise.  CONSEQUENCE: two mocca_act calls without a
// mocca_step in between draw the SAME noise (the step counter has not moved).
//
// Symmetry.  With mirror tables attached (mocca_set_policy_symmetry: in_perm / in_sign [in_dim], act_perm / act_sign [act_dim], each an
// involution with (M x)[k] = sign[k] * x[perm[k]] and sign[perm[k]] = sign[k]) the kernel's symmetric instance runs; the policy is
//     mean_sym(s) = 1/2 ( f(n(s)) + M_a f(n(M_o s)) )        value_sym(s) = 1/2 ( V(n(s)) + V(n(M_o s)) )
// with n the normalisation above.  Columns: the 16 MFMA columns of a workgroup are POL_SYM_TILE = 8 envs x {as given, mirrored}: column c < 8
// is env env0 + c, column 8 + c its mirror image; the grid is ceil(N / 8) x {actor, critic}.  Staging of a mirrored column, feature k:
//     v = in[env][in_perm[k]] * in_sign[k]          then, as for the plain column,  clamp((v - mean[k]) * inv_std[k], -clip, +clip)
// -- the mirror acts on the RAW row and the statistics are indexed by k: running statistics are not symmetric, and only so is the pair
// {n(s), n(M_o s)} exactly swapped when the input is mirrored.  The layer loop is the plain one: the two columns of an env are the same dot
// products in the same order wherever they sit.  Head stage: one lane per env, j ascending, each line ONE f32 operation in this order:
//     m      = head[c][j]
//     m'     = head[8 + c][act_perm[j]] * act_sign[j]
//     mean   = 0.5f * (m + m')
//     ls     = 0.5f * (log_std[j] + log_std[act_perm[j]])               the symmetrised log_std
//     action = mean + expf(ls) * eps[j]
//     logp  += (-0.5f * eps[j]) * eps[j] - ls - 0.9189385...
//     value  = 0.5f * (v + v')                                          critic workgroups
// mean_dev receives `mean`; deterministic: action = mean bit for bit.  The noise is the plain instance's: same keying, each env's normals drawn
// once, so for the same seed, env and counters both instances see the same eps.  CONSEQUENCE: act(M_o s) = M_a act(s) and value(M_o s) =
// value(s) hold numerically (==; a sum that cancels may come out as -0 on one side and +0 on the other): the combine is commutative.
//
// Privileged critic (mocca_set_policy_priv: an asymmetric actor-critic).  The critic has an input of its own: critic_in_dim floats per row
// (1 .. POL_MAX_IN: the LDS row is the same) from a second buffer `critic_in` with its own stride, and its own statistics critic_mean /
// critic_inv_std behind inv_std in the image.  policy_kernel<false, true> is the plain instance with the staging of the critic's workgroups
// (net == 1, uniform over the workgroup) reading feature k < critic_in_dim of critic_in[env * critic_stride + k], normalised as
// clamp((x - critic_mean[k]) * critic_inv_std[k], -clip, +clip) -- the same f32 operations in the same order, the same clip and the same flag
// word as the actor's -- and padded with zeros to critic_in_pad.  The actor's workgroups, the layer loop and the head stage are the plain
// instance's: action, logp and mean are the bits of a plain policy with the same actor, the value those of a plain policy of in_dim =
// critic_in_dim with the same critic on the critic's rows.  No mirror tables: the symmetric instance has no such twin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mocca_controller.h"

namespace mocca_pol {

using mocca_ctrl::CTRL_LAYER_WORDS;
constexpr int POL_MAX_IN = 336;       // input floats after padding to 16: obs_dim 36 .. 65, or [obs | scan] up to 65 + 256
constexpr int POL_MAX_ACTION = 32;    // actor head
constexpr int POL_MAX_WIDTH = mocca_ctrl::CTRL_MAX_WIDTH, POL_MAX_LAYERS = mocca_ctrl::CTRL_MAX_LAYERS;
constexpr int POL_FLAG_WORDS = 4;
constexpr int POL_TILE = 16;          // envs per workgroup (the controller measured 16 as best: profiles/HISTORY.md)
constexpr int POL_SYM_TILE = 8;       // envs per workgroup of the symmetric instance: each takes two of the 16 MFMA columns

struct PolicyArgs {
  const float* params;          // device: the image
  const int32_t* layers;        // device, [n_actor + n_critic][CTRL_LAYER_WORDS]
  int n_actor, n_critic;
  int log_std_off, flags_off, mean_off, inv_std_off;   // float offsets into the image
  const float* in;              // [N][in_stride], the first in_dim floats of a row are read
  int in_stride, in_dim, in_pad, act_dim;
  float clip;
  const float* eps;             // [N][act_dim] caller noise, or null
  int deterministic;
  const uint32_t* task;         // the handle's task records (MOCCA_TW_T, MOCCA_TW_EPISODE), read only for in-kernel noise
  int task_words, tw_t, tw_episode;
  int env_offset;
  uint32_t seed_lo, seed_hi;
  float* action;                // [N][act_dim], not clipped (apply_action clips; a2c-ppo-acktr stores the raw sample)
  float* logp;                  // [N] or null
  float* value;                 // [N] or null: the critic's workgroups are not launched
  float* mean;                  // [N][act_dim] or null
  int n_envs;
  // the mirror tables (header: Symmetry), device; in_perm null: the plain instance
  const int32_t* in_perm;       // [in_dim]
  const float* in_sign;         // [in_dim]
  const int32_t* act_perm;      // [act_dim]
  const float* act_sign;        // [act_dim]
  // the privileged critic (header: Privileged critic); critic_in_dim 0: both nets read `in`.  At the END: the members above keep their offsets
  const float* critic_in;       // [N][critic_stride], the first critic_in_dim floats of a row are read by the critic's workgroups
  int critic_stride, critic_in_dim, critic_in_pad;
  int critic_mean_off, critic_inv_std_off;   // float offsets into the image
};

// one row of the repack kernel's table, one per layer and one per tail array (log_std, mean, inv_std, critic_mean, critic_inv_std: out = 1 row,
// no fragment order)
struct RepackRow {
  int32_t dst, dst_end;         // image range [dst, dst_end)
  int32_t src;                  // offset in the caller's parameters, < 0: the first `out` floats are `fill`, the rest zeros
  int32_t in, out, in_pad;      // weights: W[out][in] -> fragment order over in_pad columns; in_pad = 0: a plain array of `out` floats, zero padded
  float fill;
  int32_t transposed;           // weights: != 0: the row's matrix [out][in] is the transpose of the source's W[in][out] (mocca_ppo.h: Image)
};
constexpr int POL_MAX_REPACK_ROWS = 6 * POL_MAX_LAYERS + 6;   // weights + bias of 16 layers, log_std, flags, mean, inv_std, critic_mean, critic_inv_std; 16 transposed copies
struct RepackArgs {
  const float* src;
  float* image;
  int n_rows, image_floats;
  RepackRow rows[POL_MAX_REPACK_ROWS];
};

void launch_policy(hipStream_t s, const PolicyArgs& a);
void launch_repack(hipStream_t s, const RepackArgs& a);

}  // namespace mocca_pol
