// mocca_api_trainer.hip -- the C ABI of a PPO trainer's update on the device (include/mocca.h): GAE and the observation statistics
// (mocca_rollout.h), the gradient calls of PPO's loss and of distillation (mocca_ppo.h), Adam's step and the update loops (mocca_optim.h).
// Host code only: see mocca_handle.h.
#include "mocca_handle.h"

extern "C" {

int mocca_gae(mocca_handle h, const float* rew_dev, const float* value_dev, const float* masks_dev, const float* bad_masks_dev, int n_steps,
              double gamma, double lam, double reward_scale, float* returns_dev, float* adv_dev, int normalise, double adv_eps,
              float* moments_dev, void* stream) {
  ENTRY(h, "mocca_gae");
  if (!rew_dev || !value_dev || !masks_dev || !bad_masks_dev) return c.null_arg("rew_dev, value_dev, masks_dev and bad_masks_dev");
  if (normalise && (!adv_dev || !moments_dev)) return c.bad("normalise needs adv_dev and moments_dev");
  if (n_steps < 1 || n_steps > 65536) return c.bad("n_steps must be 1 .. 65536, not " + std::to_string(n_steps));
  const long long count = (long long)n_steps * h->n_envs;
  if (normalise && count < 2) return c.bad("normalise needs at least two advantages (n_steps x n_envs >= 2)");
  if (!std::isfinite(gamma) || !std::isfinite(lam) || !std::isfinite(reward_scale)) return c.bad("gamma, lam and reward_scale must be finite");
  if (!std::isfinite(adv_eps) || adv_eps < 0.0) return c.bad("adv_eps must be finite and not negative");
  DeviceGuard guard(h->device);
  const int blocks = mocca_ro::gae_blocks(h->n_envs);
  if (int rc = grow_scratch(c, h->d_gae_part, &h->gae_part_cap, 2 * (size_t)blocks)) return rc;
  mocca_ro::GaeArgs a{};
  a.rew = rew_dev; a.value = value_dev; a.masks = masks_dev; a.bad_masks = bad_masks_dev; a.returns = returns_dev; a.adv = adv_dev;
  a.partials = h->d_gae_part; a.n_envs = h->n_envs; a.n_steps = n_steps;
  a.g = (float)gamma; a.c = (float)(gamma * lam); a.s = (float)reward_scale;
  mocca_ro::launch_gae((hipStream_t)stream, a);
  if (normalise || moments_dev) {
    mocca_ro::MomentsArgs m{};
    m.partials = h->d_gae_part; m.n_partials = blocks; m.count = count; m.adv = adv_dev; m.moments = moments_dev; m.eps = (float)adv_eps;
    m.normalise = normalise != 0;
    mocca_ro::launch_moments((hipStream_t)stream, m);
  }
  return c.launched();
}

int mocca_obs_stats(mocca_handle h, const float* rows_dev, int64_t n_rows, int row_stride, int dim, double* state_dev, double eps, float* mean_dev,
                    float* inv_std_dev, void* stream) {
  ENTRY(h, "mocca_obs_stats");
  if (!rows_dev || !state_dev) return c.null_arg("rows_dev and state_dev");
  if (dim < 1 || dim > mocca_ro::OBS_MAX_DIM) return c.bad("dim must be 1 .. " + std::to_string(mocca_ro::OBS_MAX_DIM) + ", not " + std::to_string(dim));
  if (row_stride < dim) return c.small_stride("row_stride", row_stride, "dim (" + std::to_string(dim) + ")");
  if (n_rows < 1) return c.bad("n_rows must be at least 1");
  if (!std::isfinite(eps) || eps < 0.0) return c.bad("eps must be finite and not negative");
  DeviceGuard guard(h->device);
  mocca_ro::ObsArgs a{};
  a.rows = rows_dev; a.n_rows = n_rows; a.row_stride = row_stride; a.dim = dim;
  mocca_ro::obs_grid(n_rows, dim, &a.rows_per_block, &a.n_blocks);
  if (int rc = grow_scratch(c, h->d_obs_part, &h->obs_part_cap, 2 * (size_t)a.n_blocks * dim)) return rc;
  a.state = state_dev; a.partials = h->d_obs_part; a.eps = (float)eps; a.mean_out = mean_dev; a.inv_std_out = inv_std_dev;
  mocca_ro::launch_obs_stats((hipStream_t)stream, a);
  return c.launched();
}

// The rollout arrays a gradient call reads, their strides and the loss's coefficients: every entry point fills one from its arguments.  For
// distillation (PPO_DISTIL) the targets stand in the same fields: `action` carries the targets, `returns` the value targets (or NULL) and `clip`
// distill_coef; old_logp, adv and old_value are not read.  critic_obs / critic_stride: PPO_PRIV (mocca_ppo_grad_priv), the storage's critic rows.
struct PpoBatch {
  const float* obs; int obs_stride;
  const float *action, *old_logp, *adv, *returns, *old_value;
  double clip, value_coef, entropy_coef;
  int value_clip;
  const float* critic_obs = nullptr; int critic_stride = 0;
};

// mocca_ppo_grad (PPO_PLAIN), mocca_ppo_grad_sym (PPO_SYM), mocca_ppo_grad_mirror (PPO_MIRROR) and mocca_ppo_grad_dup (PPO_DUP): one batch
// record, one scratch, the same four launches; the last three share the two-column scratch layout (mocca_ppo.h).  mocca_distill_grad (PPO_DISTIL) is
// the plain call with another head stage.  check_only: the refusals alone (mocca_ppo_update asks before its first launch)
static int ppo_grad(const Call& c, mocca_ppo::PpoMode mode, const PpoBatch& b, const int64_t* idx_dev, int64_t n_rows, float* grad_dev, float* stats_dev,
                    void* stream, bool check_only = false) {
  using namespace mocca_ctrl;
  using namespace mocca_ppo;
  if (!c.h) return c.null_handle();
  const mocca_handle h = c.h;
  if (!h->student.d_pol_image || !h->student.pol_filled) return c.bad("needs a policy (mocca_set_policy, then mocca_update_policy)");
  const bool distil = mode == PPO_DISTIL;
  const bool priv = mode == PPO_PRIV;
  const bool sym = mode != PPO_PLAIN && !distil && !priv;   // twice the columns
  if (const bool has = h->student.pol.critic_in_dim != 0; has != priv) {   // (a privileged critic and a mirror attachment exclude each other)
    if (has && distil) return c.bad("the policy has a privileged critic (mocca_set_policy_priv): distilling into an asymmetric student is not provided");
    if (has) return c.bad("the policy has a privileged critic (mocca_set_policy_priv): its gradient is mocca_ppo_grad_priv, its update mocca_ppo_update_priv");
    return c.bad("needs a policy with a privileged critic (mocca_set_policy_priv); the plain policy's gradient is mocca_ppo_grad, its update mocca_ppo_update");
  }
  if (priv) {
    if (!b.critic_obs) return c.null_arg("critic_obs_dev");
    if (b.critic_stride < h->student.pol.critic_in_dim)
      return c.small_stride("critic_stride", b.critic_stride, "the policy's critic_in_dim (" + std::to_string(h->student.pol.critic_in_dim) + ")");
  } else if (const PpoMode attached = h->pol_mirror.method; distil) {
    if (attached != PPO_PLAIN)
      return c.bad(std::string("a mirror attachment is in place (") + (attached == PPO_SYM ? "mocca_set_policy_symmetry" : attached == PPO_MIRROR ? "mocca_set_policy_mirror_loss" : "mocca_set_policy_mirror_dup") +
                 "): the regression gradient is the plain policy's, detach it first");
  } else if (mode != attached) {   // the first of these that holds names the entry point to call instead
    if (attached == PPO_DUP)
      return c.bad("duplicated rows are attached: the gradient of PPO's loss over the rows and their mirror images is mocca_ppo_grad_dup (or detach them: mocca_set_policy_mirror_dup)");
    if (mode == PPO_DUP) return c.bad("needs duplicated rows attached (mocca_set_policy_mirror_dup); the plain loss's gradient is mocca_ppo_grad");
    if (attached == PPO_MIRROR)
      return c.bad("a mirror loss is attached: the gradient of PPO's loss with the mirror term is mocca_ppo_grad_mirror (or detach it: mocca_set_policy_mirror_loss)");
    if (mode == PPO_MIRROR) return c.bad("needs a mirror loss attached (mocca_set_policy_mirror_loss); the plain loss's gradient is mocca_ppo_grad");
    if (mode == PPO_PLAIN)
      return c.bad("the policy has mirror tables attached: the symmetric policy's gradient is mocca_ppo_grad_sym (or detach the tables: mocca_set_policy_symmetry)");
    return c.bad("needs a policy with mirror tables attached (mocca_set_policy_symmetry); the plain policy's gradient is mocca_ppo_grad");
  }
  if (distil && (!b.obs || !b.action || !grad_dev)) return c.null_arg("obs_dev, target_dev and grad_dev");
  if (!distil && (!b.obs || !b.action || !b.old_logp || !b.adv || !b.returns || !grad_dev))
    return c.null_arg("obs_dev, action_dev, old_logp_dev, adv_dev, returns_dev and grad_dev");
  if (b.value_clip && !b.old_value) return c.bad("value_clip needs old_value_dev");
  if (n_rows < 1 || n_rows > (sym ? PPO_MAX_ROWS_SYM : PPO_MAX_ROWS)) return c.bad(std::string("n_rows must be 1 .. ") + (sym ? "2^21" : "2^22") + ", not " + std::to_string(n_rows));
  if (b.obs_stride < h->student.pol.in_dim)
    return c.small_stride("obs_stride", b.obs_stride, "the policy's in_dim (" + std::to_string(h->student.pol.in_dim) + ")");
  if (!std::isfinite(b.clip) || b.clip < 0.0 || !std::isfinite(b.value_coef) || b.value_coef < 0.0 || !std::isfinite(b.entropy_coef) || b.entropy_coef < 0.0)
    return c.bad(distil ? "distill_coef and value_coef must be finite and not negative" : "clip, value_coef and entropy_coef must be finite and not negative");
  if (check_only) return MOCCA_OK;
  DeviceGuard guard(h->device);
  PpoArgs a{};
  const mocca_pol::PolicyArgs& p = h->student.pol;
  a.params = p.params; a.layers = p.layers; a.n_actor = p.n_actor; a.n_critic = p.n_critic;
  a.log_std_off = p.log_std_off; a.flags_off = p.flags_off; a.mean_off = p.mean_off; a.inv_std_off = p.inv_std_off;
  a.in_dim = p.in_dim; a.in_pad = p.in_pad; a.act_dim = p.act_dim; a.norm_clip = p.clip;
  std::memcpy(a.wt_off, h->student.pol_wt_off, sizeof(a.wt_off));
  a.mode = mode;
  if (distil) a.mirror_k2 = (float)(2.0 * b.clip);   // f32(2 distill_coef), the product in double
  if (sym) {
    a.in_perm = h->pol_mirror.perm; a.act_perm = h->pol_mirror.perm.get() + p.in_dim;
    a.in_sign = h->pol_mirror.sign; a.act_sign = h->pol_mirror.sign.get() + p.in_dim;
    a.mirror_k2 = (float)(2.0 * h->pol_mirror.coef);
  }
  a.obs = b.obs; a.obs_stride = b.obs_stride; a.action = b.action; a.old_logp = b.old_logp; a.adv = b.adv; a.returns = b.returns;
  a.old_value = b.old_value; a.idx = idx_dev;
  a.n_rows = (int)n_rows;
  a.b_pad = sym ? (int)((n_rows + PPO_SYM_TILE - 1) / PPO_SYM_TILE * 16) : (int)((n_rows + 15) / 16 * 16);   // the scratch's rows (mocca_ppo.h)
  a.clip = (float)b.clip; a.value_coef = (float)b.value_coef; a.entropy_coef = (float)b.entropy_coef; a.inv_b = 1.0f / (float)n_rows;
  a.n_samples = (int)n_rows;
  if (mode == PPO_DUP) { a.n_samples = 2 * (int)n_rows; a.inv_b = 1.0f / (float)a.n_samples; }   // every mean is over the 2 B samples
  a.value_clip = b.value_clip != 0;
  // the scratch (mocca_ppo.h), in floats; every piece a multiple of 4 floats, so that rows stay 16-byte aligned
  const long long bp = a.b_pad;
  const int n_layers = p.n_actor + p.n_critic;
  long long pos = 0;
  int n_tiles = PPO_ROW_COLS / 16, n_head = p.act_dim;
  a.a0_off = pos; pos += bp * p.in_pad;
  a.a0c_off = a.a0_off;
  if (priv) {   // A0c (mocca_ppo.h: Privileged critic)
    a.critic_obs = b.critic_obs; a.critic_stride = b.critic_stride; a.critic_in_dim = p.critic_in_dim; a.critic_in_pad = p.critic_in_pad;
    a.critic_mean_off = p.critic_mean_off; a.critic_inv_std_off = p.critic_inv_std_off;
    a.a0c_off = pos; pos += bp * p.critic_in_pad;
  }
  for (int i = 0; i < n_layers; ++i) {
    const int32_t* r = &h->student.pol_table[(size_t)i * CTRL_LAYER_WORDS];
    a.a_off[i] = pos; pos += bp * r[CL_OUT_PAD];
    a.dz_off[i] = pos; pos += bp * r[CL_OUT_PAD];
    n_tiles += (r[CL_OUT_PAD] / 16) * (r[CL_IN_PAD] / 16) + r[CL_OUT_PAD] / 16;
    n_head += r[CL_IN] * r[CL_OUT] + r[CL_OUT];
  }
  a.r_off = pos; pos += bp * PPO_ROW_COLS;
  ppo_chunks(a.b_pad, &a.n_chunks, &a.chunk_rows);
  a.p_floats = p.log_std_off + PPO_ROW_COLS;
  a.p_off = pos; pos += (long long)a.n_chunks * a.p_floats;
  a.n_tiles = n_tiles; a.n_head = n_head; a.n_reduce_blocks = (n_head + PPO_REDUCE_BLOCK - 1) / PPO_REDUCE_BLOCK;
  const size_t f_doubles = (size_t)(pos + 1) / 2;
  if (int rc = grow_scratch(c, h->d_ppo, &h->ppo_cap, f_doubles + (size_t)a.n_reduce_blocks)) return rc;
  a.scratch = (float*)h->d_ppo.get(); a.sq_part = h->d_ppo.get() + f_doubles;
  a.grad = grad_dev; a.stats = stats_dev;
  launch_ppo((hipStream_t)stream, a);
  return c.launched();
}

int mocca_ppo_grad(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev, const float* adv_dev,
                   const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows, double clip, double value_coef,
                   double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip};
  return ppo_grad(Call(h, "mocca_ppo_grad"), mocca_ppo::PPO_PLAIN, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_sym(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                       const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows, double clip,
                       double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip};
  return ppo_grad(Call(h, "mocca_ppo_grad_sym"), mocca_ppo::PPO_SYM, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_mirror(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                          const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows,
                          double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip};
  return ppo_grad(Call(h, "mocca_ppo_grad_mirror"), mocca_ppo::PPO_MIRROR, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_dup(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                       const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows,
                       double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip};
  return ppo_grad(Call(h, "mocca_ppo_grad_dup"), mocca_ppo::PPO_DUP, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_priv(mocca_handle h, const float* obs_dev, int obs_stride, const float* critic_obs_dev, int critic_stride, const float* action_dev,
                        const float* old_logp_dev, const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev,
                        int64_t n_rows, double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev,
                        void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip,
                   critic_obs_dev, critic_stride};
  return ppo_grad(Call(h, "mocca_ppo_grad_priv"), mocca_ppo::PPO_PRIV, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

int mocca_distill_grad(mocca_handle h, const float* obs_dev, int obs_stride, const float* target_dev, const float* value_target_dev,
                       const int64_t* idx_dev, int64_t n_rows, double distill_coef, double value_coef, float* grad_dev, float* stats_dev,
                       void* stream) {
  const PpoBatch b{obs_dev, obs_stride, target_dev, nullptr, nullptr, value_target_dev, nullptr, distill_coef, value_coef, 0.0, 0};
  return ppo_grad(Call(h, "mocca_distill_grad"), mocca_ppo::PPO_DISTIL, b, idx_dev, n_rows, grad_dev, stats_dev, stream);
}

// One step of Adam on the student's flat parameter tensor: what mocca_adam_step takes, and what the update loops repeat per minibatch.
struct AdamStep {
  float* params; size_t n_floats; int64_t n_params;
  float* moments; double* clock;
  double lr, beta1, beta2, eps, max_grad_norm;
};

// the refusals of mocca_adam_step's arguments (mocca_ppo_update shares them): -> MOCCA_OK, or MOCCA_E_ARG with the message set
static int adam_check(const Call& c, const AdamStep& s, const float* grad_dev, bool need_grad) {
  if (!c.h) return c.null_handle();
  const mocca_handle h = c.h;
  if (!h->student.d_pol_image) return c.needs("a policy", "mocca_set_policy", true);
  if (!s.params || (need_grad && !grad_dev) || !s.moments || !s.clock)
    return c.null_arg(need_grad ? "params_dev, grad_dev, moments_dev and clock_dev" : "params_dev, moments_dev and clock_dev");
  const std::string wrong = check_n_floats(h->student, s.n_floats);
  if (!wrong.empty()) return c.bad(wrong);
  if (s.n_params < 1 || s.n_params > (int64_t)h->student.pol_n_base)
    return c.bad("n_params must be 1 .. " + std::to_string(h->student.pol_n_base) + " (the floats ahead of mean / inv_std), not " + std::to_string(s.n_params));
  if (!std::isfinite(s.lr) || s.lr < 0.0 || !std::isfinite(s.eps) || s.eps < 0.0) return c.bad("lr and eps must be finite and not negative");
  if (!(s.beta1 >= 0.0 && s.beta1 < 1.0) || !(s.beta2 >= 0.0 && s.beta2 < 1.0)) return c.bad("beta1 and beta2 must lie in [0, 1)");
  if (std::isnan(s.max_grad_norm) || s.max_grad_norm < 0.0) return c.bad("max_grad_norm must not be NaN or negative (0: no clip)");
  return MOCCA_OK;
}

// f64 words of d_optim ahead of the permutation (mocca_optim.h: Scratch)
static size_t optim_head_words(mocca_handle h) { return mocca_optim::OPT_REC_WORDS + (h->student.pol_n_base + 1) / 2; }

// launches A, B and C of mocca_adam_step; the arguments have been checked, d_optim holds the record, the handle's device is current
static void adam_launch(mocca_handle h, const AdamStep& s, const float* grad_dev, float* stats_row, hipStream_t stream) {
  mocca_optim::AdamArgs a{};
  a.params = s.params; a.grad = grad_dev; a.n_params = (int)s.n_params;
  a.m = s.moments; a.v = s.moments + h->student.pol_n_base; a.clock = s.clock;
  a.rec = (mocca_optim::AdamRecord*)h->d_optim.get();
  a.lr = s.lr; a.beta1 = s.beta1; a.beta2 = s.beta2; a.eps = s.eps; a.max_grad_norm = s.max_grad_norm; a.stats = stats_row;
  mocca_optim::launch_adam(stream, a);
  repack_policy(h->student, s.params, s.n_floats, stream);
}

int mocca_adam_step(mocca_handle h, float* params_dev, size_t n_floats, const float* grad_dev, int64_t n_params, float* moments_dev,
                    double* clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream) {
  const Call c(h, "mocca_adam_step");
  const AdamStep s{params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm};
  if (int rc = adam_check(c, s, grad_dev, true)) return rc;
  DeviceGuard guard(h->device);
  if (int rc = grow_scratch(c, h->d_optim, &h->optim_cap, optim_head_words(h))) return rc;
  adam_launch(h, s, grad_dev, nullptr, (hipStream_t)stream);
  HIP_TRY(c, hipGetLastError());
  h->student.pol_filled = true;
  return MOCCA_OK;
}

// The body of mocca_ppo_update and mocca_distill_update: epochs x (n_rollout_rows / minibatch_rows) minibatches of [shuffle once per epoch,
// the gradient, launches A .. C of mocca_adam_step].  The gradient call is ppo_grad in `mode` on minibatch_rows rows of `b`; asked with
// check_only it only refuses.  A mirror mode's scratch has two rows per minibatch row, which halves the row bound.
static int update_loop(const Call& c, mocca_ppo::PpoMode mode, const PpoBatch& b, const AdamStep& s, int64_t n_rollout_rows, int64_t minibatch_rows,
                       int epochs, uint64_t seed, float* stats_dev, void* stream) {
  using namespace mocca_ppo;
  if (int rc = adam_check(c, s, nullptr, false)) return rc;
  const mocca_handle h = c.h;
  const bool sym = mode != PPO_PLAIN && mode != PPO_DISTIL && mode != PPO_PRIV;
  const long long most = sym ? PPO_MAX_ROWS_SYM : PPO_MAX_ROWS;
  if (n_rollout_rows < 1 || n_rollout_rows > most)
    return c.bad(std::string("n_rollout_rows must be 1 .. ") + (sym ? "2^21" : "2^22") + ", not " + std::to_string(n_rollout_rows));
  if (minibatch_rows < 1 || minibatch_rows > n_rollout_rows)
    return c.bad("minibatch_rows must be 1 .. n_rollout_rows (" + std::to_string(n_rollout_rows) + "), not " + std::to_string(minibatch_rows));
  if (epochs < 1) return c.bad("epochs must be at least 1, not " + std::to_string(epochs));
  float* const unset = s.params;   // stands for grad_dev in the check: the gradient buffer is the handle's
  if (int rc = ppo_grad(c, mode, b, nullptr, minibatch_rows, unset, nullptr, stream, true)) return rc;
  DeviceGuard guard(h->device);
  const size_t head = optim_head_words(h);
  if (int rc = grow_scratch(c, h->d_optim, &h->optim_cap, head + (size_t)n_rollout_rows)) return rc;
  float* const grad = (float*)(h->d_optim.get() + mocca_optim::OPT_REC_WORDS);
  int64_t* const perm = (int64_t*)(h->d_optim.get() + head);
  mocca_optim::ShuffleArgs sh{};
  sh.perm = perm; sh.n = (int)n_rollout_rows; sh.half = mocca_optim::shuffle_half(n_rollout_rows); sh.mask = (1u << sh.half) - 1u;
  sh.seed_lo = (uint32_t)seed; sh.seed_hi = (uint32_t)(seed >> 32); sh.clock = s.clock;
  const int64_t per_epoch = n_rollout_rows / minibatch_rows;   // BatchSampler(drop_last=True)
  for (int ep = 0; ep < epochs; ++ep) {
    mocca_optim::launch_shuffle((hipStream_t)stream, sh);
    for (int64_t u = 0; u < per_epoch; ++u) {
      float* const row = stats_dev ? stats_dev + 8 * ((size_t)ep * per_epoch + u) : nullptr;
      if (int rc = ppo_grad(c, mode, b, perm + u * minibatch_rows, minibatch_rows, grad, row, stream)) return rc;
      adam_launch(h, s, grad, row, (hipStream_t)stream);
    }
  }
  return c.launched();
}

int mocca_ppo_update(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                     const float* adv_dev, const float* returns_dev, const float* old_value_dev, int64_t n_rollout_rows,
                     int64_t minibatch_rows, int epochs, double clip, double value_coef, double entropy_coef, int value_clip,
                     float* params_dev, size_t n_floats, int64_t n_params, float* moments_dev, double* clock_dev, double lr,
                     double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip};
  const AdamStep s{params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm};
  // one entry point: what the handle's attachment makes it differentiate -- duplicated rows, the mirror loss, the symmetric network, or the plain
  // policy -- decides, as VecEnv.ppo_grad does
  const mocca_ppo::PpoMode mode = h ? h->pol_mirror.method : mocca_ppo::PPO_PLAIN;
  return update_loop(Call(h, "mocca_ppo_update"), mode, b, s, n_rollout_rows, minibatch_rows, epochs, seed, stats_dev, stream);
}

int mocca_ppo_update_priv(mocca_handle h, const float* obs_dev, int obs_stride, const float* critic_obs_dev, int critic_stride,
                          const float* action_dev, const float* old_logp_dev, const float* adv_dev, const float* returns_dev,
                          const float* old_value_dev, int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double clip, double value_coef,
                          double entropy_coef, int value_clip, float* params_dev, size_t n_floats, int64_t n_params, float* moments_dev,
                          double* clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed,
                          float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, clip, value_coef, entropy_coef, value_clip,
                   critic_obs_dev, critic_stride};
  const AdamStep s{params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm};
  return update_loop(Call(h, "mocca_ppo_update_priv"), mocca_ppo::PPO_PRIV, b, s, n_rollout_rows, minibatch_rows, epochs, seed, stats_dev, stream);
}

int mocca_distill_update(mocca_handle h, const float* obs_dev, int obs_stride, const float* target_dev, const float* value_target_dev,
                         int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double distill_coef, double value_coef, float* params_dev,
                         size_t n_floats, int64_t n_params, float* moments_dev, double* clock_dev, double lr, double beta1, double beta2, double eps,
                         double max_grad_norm, uint64_t seed, float* stats_dev, void* stream) {
  const PpoBatch b{obs_dev, obs_stride, target_dev, nullptr, nullptr, value_target_dev, nullptr, distill_coef, value_coef, 0.0, 0};
  const AdamStep s{params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm};
  return update_loop(Call(h, "mocca_distill_update"), mocca_ppo::PPO_DISTIL, b, s, n_rollout_rows, minibatch_rows, epochs, seed, stats_dev, stream);
}

}  // extern "C"
