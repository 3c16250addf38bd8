// mocca_ppo.h -- the body of a PPO minibatch step up to optimizer.step() as kernels (mocca_ppo.hip): evaluate_actions, the clipped
// surrogate, the value loss and loss.backward() for the Gaussian actor-critic of mocca_policy.h, plain, mirror-symmetric, plain with the
// mirror-symmetry loss added, or plain on mirror-duplicated rows.  mocca_ppo_grad / mocca_ppo_grad_sym / mocca_ppo_grad_mirror /
// mocca_ppo_grad_dup (mocca_api_trainer.hip) check the caller's arguments, own the scratch and launch them.  The loss and the per-row formulas: include/mocca.h.
//
// Image.  The kernels read the policy image of mocca_policy.h and, behind it, a SECOND copy of every layer's weights but a net's first,
// transposed: layer l's W[out][in] as the [in_pad / 16][out_pad / 16][64][4] fragment order of W^T (in and out swap roles and padding), so
// that dA_{l-1} = W^T dZ_l runs through the forward's MFMA loop.  The repack kernel writes both copies in its one launch (RepackRow.transposed);
// PpoArgs.wt_off[layer] is the float offset of a layer's transposed copy, -1 for a first layer.
//
// Scratch (f32, owned by the handle), B_pad = B rounded up to 16 (the symmetric call: below), layer = row of the layer table:
//   A0      [B_pad][in_pad]               the normalised input (written by the actor's workgroups)
//   A[l]    [B_pad][out_pad_l]            layer l's output activation y
//   dZ[l]   [B_pad][out_pad_l]            dL/d(pre-activation) of layer l; between the forward and the backward: act'(x) of layer l
//   R       [B_pad][PPO_ROW_COLS]         per row: 0 .. 31 the log_std gradient terms, 32 surrogate, 33 value loss, 34 old_logp - logp,
//                                         35 clipped (0 / 1), 36 the mirror term (mirror loss) or a twin's old_logp - logp (duplicated
//                                         rows), else 0, 37 .. 47 zeros
//   P       [n_chunks][p_floats]          chunk partials of the padded gradient: a layer's dW[out_pad][in_pad] row-major at the image's
//                                         w_off, its db[out_pad] at b_off, the column sums of R at log_std_off
//   Q       [reduce blocks] f64           sums of grad^2 of the reduce kernel's workgroups
// Rows past B are zeros everywhere, so the row loops of launch 2 have no bounds logic.
//
// Launch 1 (ppo_rows_kernel): grid ceil(B / 16) x {actor, critic}, 256 threads.  A workgroup gathers its 16 rows through idx, normalises them
// as the policy kernel does and runs that kernel's layer loop (same operand layout, same order of sums; tanh alone differs: (float)tanh((double)x), rounded once,
// where the policy kernel calls tanhf -- so logp and value recomputed at unchanged weights differ from what mocca_act stored by an ulp or
// two and the first minibatch's ratio is 1 +- 1e-6, not exactly 1), storing every layer's output.  Head stage: one lane per row forms the row's loss terms and dL/dhead.  Backward, from the head down:
//     dZ_l = dA_l * act'(x_l)      tanh: sech^2 x;  relu: x > 0;  softsign: 1 / (1 + |x|)^2;  identity: 1    (formed in the forward from the
//                                  pre-activation x and parked in dZ_l: 1 - y y from the output cancels where a unit saturates)
//     dA_{l-1} = W_l^T dZ_l        the forward's MFMA loop over the transposed copy; not formed for a net's first layer
// Launch 2 (ppo_wgrad_kernel): one wave per (tile, row chunk).  A weight tile is 16 x 16 of dW_l = sum_rows dZ_l[row][o] A_{l-1}[row][k]:
// v_mfma_f32_16x16x4_f32 over the chunk's rows in ascending order, 16 rows per trip into FOUR accumulators (MFMA j takes rows 4 j .. 4 j + 3
// of the trip), combined (p0 + p1) + (p2 + p3).  A column tile sums 16 columns of dZ_l (db_l) or of R: lane (quad, column) adds rows quad,
// quad + 4, .. in f64, the four quads are added (q0 + q1) + (q2 + q3).  The chunk count is a function of B alone (ppo_chunks): the result
// does not depend on the device.
// Launch 3 (ppo_reduce_kernel): one thread per gradient float, un-padded, in mocca_update_policy's order: adds the chunks' partials in chunk
// order in f32, scales nothing (the 1 / B is in dL/dhead), adds -entropy_coef to log_std's; a workgroup adds its squares in f64 in a fixed tree.
// Launch 4 (ppo_stats_kernel): ONE workgroup adds the workgroups' squares in index order in f64 and writes stats[0..7].
// No atomics; every sum's order is a function of B and the shapes alone: the same inputs give the same bits.
//
// Symmetric policy (mocca_ppo_grad_sym; mocca_policy.h: Symmetry).  The same four launches on TWICE the columns: ppo_rows_kernel<true>
// gives its 16 MFMA columns to PPO_SYM_TILE = 8 minibatch rows x {as given, mirrored}, policy_kernel<true>'s layout -- column c is row
// row0 + c, column 8 + c its mirror image, staged as obs[src * stride + in_perm[k]] * in_sign[k] ahead of the same normalisation --, the grid
// is ceil(B / 8) x {actor, critic}, and column e of workgroup t owns SCRATCH ROW 16 t + e of A0, A[l], dZ[l] and R: B_pad = 16 ceil(B / 8), twice
// the plain call's rows.  The layer loop and the backward loop are the plain instance's (LDS is unchanged).  Head stage: lane c < 8 reads
// the heads of columns c and 8 + c, forms the symmetrised mean, log_std and value, runs the plain per-row lines on them and hands
// each head its half (include/mocca.h); R's terms go to the as-given column's row, the mirrored column's R row and every row of a column
// without a minibatch row are zeros.  Launch 2 is unchanged: summing dZ^T A over the scratch rows adds both passes' weight gradients, in
// scratch-row order.  Launch 3 forms log_std's entries as 0.5f * (T[j] + T[act_perm[j]]) from the chunk sums T; launch 4 takes the entropy
// of the symmetrised log_std.  Both select that arithmetic by PpoArgs.mode == PPO_SYM.
//
// Mirror loss (mocca_ppo_grad_mirror; include/mocca.h).  The PLAIN policy with w mean_rows mean_j (f1[j] - act_sign[j] f2[act_perm[j]])^2 added
// to the loss, f2 the actor on the mirror image.  ppo_rows_kernel<PPO_MIRROR> is the symmetric instance -- its staging, column layout,
// scratch-row ownership, B_pad, layer loop and backward loop -- with another head stage: lane c < 8 runs the plain per-row lines on the
// as-given column's heads (mean f1, log_std and value un-symmetrised), adds the mirror term's gradient u to dL/df1 and hands the mirrored
// actor column -(u * act_sign) through act_perm; the row's term goes to column 36 of R.  The critic has no mirror term: its workgroups still
// stage 8 + 8 columns, but the mirrored ones are NOT LIVE -- zero activations and zero slopes stored, zero dA --, so their scratch rows add
// exactly nothing to the critic's dW and db in launch 2.  Launches 3 and 4 use the plain log_std arithmetic (mode, not the tables, selects
// it); launch 4 writes stats[7] = (column 36's sum) * ib, which the plain and symmetric modes leave 0.
//
// Duplicated rows (mocca_ppo_grad_dup; include/mocca.h).  The PLAIN policy and the plain loss over 2 B samples: every row and its mirror image
// (M_o s, M_a a), which borrows the row's old_logp, adv, returns and old_value.  ppo_rows_kernel<PPO_DUP> is the symmetric instance -- its
// staging, column layout, scratch-row ownership, B_pad, layer loop and backward loop -- with the PLAIN head stage on all 16 columns: lanes
// 0 .. 15 each run the per-row lines on their own column's heads, a lane >= 8 reading the action as action[act_perm[j]] * act_sign[j]; each
// writes dA for its own column alone and its R terms to its own scratch row (a mirrored column's row also old_logp - logp in column 36).
// Actor AND critic mirrored columns are live; columns without a minibatch row stay zeros.  PpoArgs.inv_b is 1 / (2 B) and n_samples 2 B.
// Launch 2 is unchanged; launches 3 and 4 use the plain log_std arithmetic, and launch 4 writes stats[7] from column 36 as it does for the
// mirror loss: the twins' share of stats[3].
//
// Distillation (mocca_distill_grad; include/mocca.h).  A supervised head on the same machinery: the loss is distill_coef mean_rows mean_j
// (mean_j - target_j)^2 + value_coef 0.5 mean (v - value_target)^2.  ppo_rows_kernel<PPO_DISTIL> is the PLAIN instance -- one column per row, its
// staging with idx and the normalisation, its layer loop with activate_once, activations and slopes to scratch, its backward -- and only the head
// stage differs: the actor's lane forms d = mean - target per action, hands u = ((d * ib) * ia) * k2 to the backward, writes +0 to the row's
// log_std terms and the row's sum of d^2 (f64) times ia to column 36 of R; the critic's lane forms the squared error against value_target, or
// zeros where that is NULL.  PpoArgs carries the targets in `action`, the value targets in `returns` and k2 = f32(2 distill_coef) in `mirror_k2`;
// old_logp, adv and old_value are not read, entropy_coef is 0.  Launches 2 to 4 are unchanged (launch 4 writes stats[7] from column 36, as for
// the mirror loss); the scratch is the plain call's.
//
// Privileged critic (mocca_ppo_grad_priv; mocca_policy.h: Privileged critic).  PPO's loss separates: the surrogate and the entropy depend on the
// actor and log_std alone, the value term on the critic alone.  ppo_rows_kernel<PPO_PRIV> is the PLAIN instance -- one column per row, its layer
// loop, head stage and backward -- with the staging of the critic's workgroups (net == 1, uniform over the workgroup) reading feature k <
// critic_in_dim of critic_obs[src * critic_stride + k] under critic_mean / critic_inv_std (the same f32 operations, clip and flag word), padded
// with zeros to critic_in_pad, and writing the tile to a second scratch array
//   A0c     [B_pad][critic_in_pad]        the critic's normalised input (written by the CRITIC's workgroups; rows past B zeros)
// which launch 2 reads as the input of the critic's first layer: PpoArgs.a0c_off, equal to a0_off in every other mode.  That layer's dW tiles
// cover critic_in_pad (the table's own in_pad), and n_head follows the table's own in.  Launches 3 and 4 are the plain ones (column 36 of R
// is zeros: stats[7] = 0).  Every sum's order is the plain call's, so the actor's and log_std's gradients are the bits of mocca_ppo_grad on
// a plain policy with the same actor, the critic's those of a plain policy of in_dim = critic_in_dim with the same critic on the critic's rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mocca_policy.h"

namespace mocca_ppo {

constexpr int PPO_ROW_COLS = 48;         // floats per row of R
constexpr int PPO_COL_SURR = 32, PPO_COL_VLOSS = 33, PPO_COL_DLOGP = 34, PPO_COL_CLIPPED = 35, PPO_COL_MIRROR = 36;
enum PpoMode { PPO_PLAIN = 0, PPO_SYM = 1, PPO_MIRROR = 2, PPO_DUP = 3, PPO_DISTIL = 4, PPO_PRIV = 5 };   // mocca_ppo_grad, _sym, _mirror, _dup; mocca_distill_grad; mocca_ppo_grad_priv
constexpr int PPO_MAX_CHUNKS = 16;       // row chunks of launch 2
constexpr int PPO_CHUNK_MIN_ROWS = 512;  // a chunk holds at least this many rows
constexpr int PPO_REDUCE_BLOCK = 256;
constexpr int PPO_MAX_TABLE = 2 * mocca_pol::POL_MAX_LAYERS;
constexpr long long PPO_MAX_ROWS = 1ll << 22;
constexpr int PPO_SYM_TILE = mocca_pol::POL_SYM_TILE;   // minibatch rows per workgroup of the symmetric instance: each takes two of the 16 MFMA columns
constexpr long long PPO_MAX_ROWS_SYM = PPO_MAX_ROWS / 2;   // the same bound on the scratch's rows

struct PpoArgs {
  // the policy: image, layer table, shapes (PolicyArgs of the handle)
  const float* params;
  const int32_t* layers;
  int n_actor, n_critic;
  int log_std_off, flags_off, mean_off, inv_std_off;
  int in_dim, in_pad, act_dim;
  float norm_clip;
  int wt_off[PPO_MAX_TABLE];             // transposed copies (header: Image)
  // the mirror tables (mocca_policy.h: Symmetry), device; null in PPO_PLAIN.  mode, not the tables, selects every kernel's arithmetic
  const int32_t *in_perm, *act_perm;     // [in_dim], [act_dim]
  const float *in_sign, *act_sign;
  int mode;                              // PpoMode
  float mirror_k2;                       // PPO_MIRROR: f32(2 mirror_coef); PPO_DISTIL: f32(2 distill_coef)
  // the minibatch
  const float* obs; int obs_stride;
  const float *action, *old_logp, *adv, *returns, *old_value;
  const int64_t* idx;                    // [B] or null: rows 0 .. B - 1.  PPO_DISTIL: action = the target rows [R][act_dim], returns = value_target or null
  int n_rows, b_pad;                     // B; the scratch's rows: B rounded up to 16, symmetric: 16 ceil(B / 8)
  float clip, value_coef, entropy_coef, inv_b;
  int value_clip;
  // scratch (header: Scratch); float offsets of A[l] / dZ[l] from `scratch`
  float* scratch;
  long long a0_off, a_off[PPO_MAX_TABLE], dz_off[PPO_MAX_TABLE], r_off, p_off;
  int p_floats, n_chunks, chunk_rows;    // chunk_rows: a multiple of 16
  int n_tiles;                           // weight and column tiles of launch 2
  double* sq_part;                       // Q
  int n_head, n_reduce_blocks;
  float* grad;                           // [n_head]
  float* stats;                          // [8] or null
  int n_samples;                         // what stats[4]'s count is divided by: B, PPO_DUP: 2 B
  // the privileged critic (header: Privileged critic), read by PPO_PRIV alone.  At the END: the members above keep their offsets
  const float* critic_obs; int critic_stride;   // the storage's critic rows [R][critic_stride], gathered through the same idx
  int critic_in_dim, critic_in_pad;
  int critic_mean_off, critic_inv_std_off;
  long long a0c_off;                     // A0c: what launch 2 reads as the input of the critic's FIRST layer; every other mode: a0_off
};

// row chunks of launch 2 for a minibatch of b_pad rows: a function of B alone
inline void ppo_chunks(int b_pad, int* n_chunks, int* chunk_rows) {
  int c = (b_pad + PPO_CHUNK_MIN_ROWS - 1) / PPO_CHUNK_MIN_ROWS;
  if (c > PPO_MAX_CHUNKS) c = PPO_MAX_CHUNKS;
  const int rows = ((b_pad / 16 + c - 1) / c) * 16;
  *chunk_rows = rows;
  *n_chunks = (b_pad + rows - 1) / rows;
}

void launch_ppo(hipStream_t s, const PpoArgs& a);

}  // namespace mocca_ppo
