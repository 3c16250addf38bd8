// mocca_api_policy.hip -- the C ABI of the networks a handle evaluates (include/mocca.h): the planner envs' base controller and its input
// statistics (mocca_controller.h), the student's and the teacher's policy slots and the student's mirror tables (mocca_policy.h), and the calls that
// run them: plan_step, act, act_step, act_plan_step, teacher_act.  Host code only: see mocca_handle.h.
#include "mocca_handle.h"

// The rules of an actor-critic layer table (mocca_controller.h: CTRL_LAYER_WORDS int32 per layer, the actor's layers first), shared by the base
// controller and the policy: -> "" and the two layer counts, or what is wrong with the first layer that breaks a rule.  `in_dim`: what a net's
// first layer takes (`first_takes` says so in words; a "%d" in it becomes the width found instead); `head`: the actor's outputs (`ends_in`);
// `n_params`: floats of the array the weight and bias offsets point into, or NO_OFFSETS where they are not read.  A layer's input is in_dim or
// the previous layer's output, so it needs no bound of its own.
constexpr size_t NO_OFFSETS = ~(size_t)0;
static std::string check_layer_table(const int32_t* layers, int n_layers_total, int in_dim, int head, size_t n_params, const std::string& first_takes,
                                     const std::string& ends_in, int count[2], int critic_in_dim = 0) {   // critic_in_dim != 0: what the CRITIC's first layer takes
  using namespace mocca_ctrl;
  if (!layers || n_layers_total < 2 || n_layers_total > 2 * CTRL_MAX_LAYERS) return "needs 1 .. 8 layers for each of the two nets";
  count[0] = count[1] = 0;
  int prev_out = 0;
  for (int i = 0; i < n_layers_total; ++i) {
    const int32_t* r = layers + (size_t)i * CTRL_LAYER_WORDS;
    const std::string at = "layer " + std::to_string(i) + ": ";
    const int net = r[CL_NET];
    if (net != 0 && net != 1) return at + "net must be 0 (actor) or 1 (critic)";
    if (i > 0 && net < (r - CTRL_LAYER_WORDS)[CL_NET]) return at + "the actor's layers come first, then the critic's";
    const bool first = count[net] == 0;
    if (++count[net] > CTRL_MAX_LAYERS) return at + "more than 8 layers in one net";
    const int in = r[CL_IN], out = r[CL_OUT];
    if (first && in != (net == 1 && critic_in_dim ? critic_in_dim : in_dim)) {
      std::string what = first_takes;
      const size_t k = what.find("%d");
      return at + (k == std::string::npos ? what : what.replace(k, 2, std::to_string(in)));
    }
    if (!first && in != prev_out) return at + "input width differs from the previous layer's output";
    if (out < 1 || out > CTRL_MAX_WIDTH) return at + "widths must be 1 .. 256";
    if (r[CL_IN_PAD] != (in + 15) / 16 * 16 || r[CL_OUT_PAD] != (out + 15) / 16 * 16) return at + "in_pad / out_pad must be the widths rounded up to a multiple of 16";
    if (r[CL_ACT] < CTRL_ACT_IDENTITY || r[CL_ACT] > CTRL_ACT_SOFTSIGN) return at + "unknown activation";
    const long long w_off = r[CL_W_OFF], b_off = r[CL_B_OFF];
    if (n_params != NO_OFFSETS && (w_off < 0 || b_off < 0 || (size_t)w_off + (size_t)in * out > n_params || (size_t)b_off + out > n_params))
      return at + "weights W[out][in] / bias b[out] must lie inside the parameter array";
    prev_out = out;
    const bool last = i + 1 == n_layers_total || (r + CTRL_LAYER_WORDS)[CL_NET] != net;
    if (last && out != (net == 0 ? head : 1)) return at + ends_in;
    if (!last && (out & 15)) return at + "hidden widths must be multiples of 16";
  }
  return count[0] < 1 || count[1] < 1 ? "needs an actor and a critic" : "";
}

// The image of a checked layer table (mocca_policy.h) in new device buffers: the table with its offsets pointing into the image, the zeroed
// image, the rows that tell the repack kernel where each piece of the source parameters goes, and the kernel's shapes and image offsets.
// `packed`: the source is W[out][in], b[out] layer after layer, then log_std (n_src: floats of that); otherwise the table's own w_off /
// b_off say where a layer's weights and bias lie in it, and log_std is zeros.  The rows tail_row .. + 2 (flags, mean, inv_std) come out as
// zeros: mocca_update_policy sets their source per call.  A packed image ends in the transposed copies of the weights of every layer but a
// net's first (mocca_ppo.h: Image), behind everything the policy kernel reads: wt_off says where, -1 for a layer without one.
struct NetImage {
  DevBuf<float> image;
  DevBuf<int32_t> layers;
  mocca_pol::PolicyArgs pa{};
  mocca_pol::RepackArgs rp{};
  size_t n_src = 0;
  int tail_row = 0;
  std::vector<int32_t> table;
  int wt_off[mocca_ppo::PPO_MAX_TABLE];
};
static hipError_t build_image(NetImage& im, const int32_t* layers_host, int n_layers_total, const int count[2], int in_dim, int act_dim, bool packed,
                              int critic_in_dim = 0) {   // != 0: a privileged critic -- two more tail rows, critic_mean and critic_inv_std (tail_row + 3, + 4)
  using namespace mocca_ctrl;
  using namespace mocca_pol;
  std::vector<int32_t>& table = im.table;
  table.assign(layers_host, layers_host + (size_t)n_layers_total * CTRL_LAYER_WORDS);
  const int in_pad = (in_dim + 15) / 16 * 16;
  int pos = 0, src = 0, nr = 0;
  auto row = [&](int floats, int src_off, int in, int out, int ipad) {
    RepackRow& q = im.rp.rows[nr++];
    q.dst = pos; q.dst_end = pos + floats; q.src = src_off; q.in = in; q.out = out; q.in_pad = ipad; q.fill = 0.0f; q.transposed = 0;
    pos += floats;
    return q.dst;
  };
  for (int i = 0; i < n_layers_total; ++i) {
    int32_t* r = &table[(size_t)i * CTRL_LAYER_WORDS];
    const int in = r[CL_IN], out = r[CL_OUT];
    r[CL_W_OFF] = row(r[CL_IN_PAD] * r[CL_OUT_PAD], packed ? src : r[CL_W_OFF], in, out, r[CL_IN_PAD]);
    src += in * out;
    r[CL_B_OFF] = row(r[CL_OUT_PAD], packed ? src : r[CL_B_OFF], 0, out, 0);
    src += out;
  }
  PolicyArgs& pa = im.pa;
  pa.log_std_off = row(POL_MAX_ACTION, packed ? src : -1, 0, act_dim, 0);
  im.n_src = (size_t)src + act_dim;
  im.tail_row = nr;
  pa.flags_off = row(POL_FLAG_WORDS, -1, 0, 1, 0);
  pa.mean_off = row(in_pad, -1, 0, in_dim, 0);
  pa.inv_std_off = row(in_pad, -1, 0, in_dim, 0);
  if (critic_in_dim) {   // a plain policy's image has neither: its offsets do not move
    pa.critic_in_dim = critic_in_dim; pa.critic_in_pad = (critic_in_dim + 15) / 16 * 16;
    pa.critic_mean_off = row(pa.critic_in_pad, -1, 0, critic_in_dim, 0);
    pa.critic_inv_std_off = row(pa.critic_in_pad, -1, 0, critic_in_dim, 0);
  }
  for (int i = 0, s = 0; i < n_layers_total; ++i) {   // W^T of a layer: in and out swap roles and padding
    const int32_t* r = &table[(size_t)i * CTRL_LAYER_WORDS];
    im.wt_off[i] = -1;
    if (packed && i != 0 && i != count[0]) {
      im.wt_off[i] = row(r[CL_IN_PAD] * r[CL_OUT_PAD], s, r[CL_OUT], r[CL_IN], r[CL_OUT_PAD]);
      im.rp.rows[nr - 1].transposed = 1;
    }
    s += r[CL_IN] * r[CL_OUT] + r[CL_OUT];
  }
  im.rp.n_rows = nr; im.rp.image_floats = pos;
  hipError_t e = im.image.alloc((size_t)pos, true);
  if (e == hipSuccess) e = im.layers.alloc(table.size(), false);
  if (e == hipSuccess) e = hipMemcpy(im.layers, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  im.rp.image = im.image;
  pa.params = im.image; pa.layers = im.layers; pa.n_actor = count[0]; pa.n_critic = count[1];
  pa.in_dim = in_dim; pa.in_pad = in_pad; pa.act_dim = act_dim;
  return e;
}

// what n_floats of a flat parameter tensor must be (mocca_update_policy, mocca_update_teacher, mocca_adam_step): -> "" or what is wrong
std::string check_n_floats(const mocca_ctx::PolicySlot& slot, size_t n_floats) {
  const size_t base = slot.pol_n_base, in_dim = (size_t)slot.pol.in_dim, critic_in = (size_t)slot.pol.critic_in_dim;
  if (n_floats == base || n_floats == base + 2 * in_dim + 2 * critic_in) return "";
  return "this policy takes " + std::to_string(base) + " floats (layers, log_std), or " + std::to_string(base + 2 * in_dim + 2 * critic_in) +
         (critic_in ? " with mean, inv_std, critic_mean and critic_inv_std, not " : " with mean and inv_std, not ") + std::to_string(n_floats);
}

// the repack launch of mocca_update_policy / mocca_update_teacher; n_floats has been checked, the handle's device is current
void repack_policy(const mocca_ctx::PolicySlot& slot, const float* params_dev, size_t n_floats, hipStream_t s) {
  const size_t base = slot.pol_n_base, in_dim = (size_t)slot.pol.in_dim;
  mocca_pol::RepackArgs rp = slot.pol_repack;
  rp.src = params_dev;
  const bool norm = n_floats != base;
  rp.rows[slot.pol_tail_row].fill = norm ? 1.0f : 0.0f;
  rp.rows[slot.pol_tail_row + 1].src = norm ? (int32_t)base : -1;
  rp.rows[slot.pol_tail_row + 2].src = norm ? (int32_t)(base + in_dim) : -1;
  if (const size_t critic_in = (size_t)slot.pol.critic_in_dim) {   // a privileged critic: its statistics follow, all four or none
    rp.rows[slot.pol_tail_row + 3].src = norm ? (int32_t)(base + 2 * in_dim) : -1;
    rp.rows[slot.pol_tail_row + 4].src = norm ? (int32_t)(base + 2 * in_dim + critic_in) : -1;
  }
  mocca_pol::launch_repack(s, rp);
}

extern "C" {

int mocca_get_base_outputs(mocca_handle h, float* action_dev, float* value_dev, void* stream) {
  ENTRY(h, "mocca_get_base_outputs");
  if (!h->d_ctrl_image) return c.needs("a base controller", "mocca_set_base_controller");
  DeviceGuard guard(h->device);
  if (action_dev) HIP_TRY(c, hipMemcpyAsync(action_dev, h->d_base_act, (size_t)h->n_envs * mocca_ctrl::CTRL_ACTION * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (value_dev) HIP_TRY(c, hipMemcpyAsync(value_dev, h->d_base_val, (size_t)h->n_envs * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_base_controller(mocca_handle h, const float* params_host, size_t n_floats, const int32_t* layers_host, int n_layers_total,
                              double action_scale) try {
  using namespace mocca_ctrl;
  ENTRY(h, "mocca_set_base_controller");
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return c.bad("only the planner task (Walker3DPlannerEnv, MikePlannerEnv) has a base controller");
  DeviceGuard guard(h->device);
  if (!params_host) {   // detach
    if (int rc = commit_ready(c)) return rc;
    h->d_ctrl_image.reset(); h->d_ctrl_layers.reset(); h->d_ctrl_norm.reset(); h->ctrl = {};
    return MOCCA_OK;
  }
  if (n_floats == 0 || n_floats > ((size_t)1 << 28)) return c.bad("the parameter array is empty or larger than any valid controller");
  if (!std::isfinite(action_scale)) return c.bad("action_scale is not finite");
  int count[2];
  const std::string wrong = check_layer_table(layers_host, n_layers_total, CTRL_IN, CTRL_ACTION, n_floats, "a net's first layer takes the 65-float input",
                                              "the actor ends in 21 outputs, the critic in 1", count);
  if (!wrong.empty()) return c.bad(wrong);
  // the image: the caller's parameters go to the device as they are and the repack kernel puts them in fragment order; it has ended when
  // `flat` and a refused call's image are freed (on success commit_ready synchronises, after a failure the line below does).  The per-env
  // buffers outlive a controller: made by the first attach, kept (with their content) by a replace and by a detach
  NetImage im;
  DevBuf<float> flat, state, act, val;
  const size_t n = (size_t)h->n_envs;
  hipError_t e = build_image(im, layers_host, n_layers_total, count, CTRL_IN, CTRL_ACTION, false);
  if (e == hipSuccess) e = flat.alloc(n_floats, false);
  if (e == hipSuccess) e = hipMemcpy(flat, params_host, n_floats * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    im.rp.src = flat;
    mocca_pol::launch_repack(nullptr, im.rp);
    e = hipGetLastError();
  }
  if (e == hipSuccess && !h->d_robot_state) e = state.alloc(n * CTRL_RS_STRIDE, true);
  if (e == hipSuccess && !h->d_base_act) e = act.alloc(n * CTRL_ACTION, true);
  if (e == hipSuccess && !h->d_base_val) e = val.alloc(n, true);
  if (e != hipSuccess) (void)hipDeviceSynchronize();
  if (int rc = commit_ready(c, e)) return rc;
  h->d_ctrl_image.swap(im.image); h->d_ctrl_layers.swap(im.layers);
  if (state) h->d_robot_state.swap(state);
  if (act) h->d_base_act.swap(act);
  if (val) h->d_base_val.swap(val);
  mocca_ctrl::ControllerArgs& ca = h->ctrl;
  ca.params = im.pa.params; ca.layers = im.pa.layers; ca.n_actor = count[0]; ca.n_critic = count[1];
  ca.robot_state = h->d_robot_state; ca.action_scale = (float)action_scale;
  ca.action = h->d_base_act; ca.value = h->d_base_val; ca.n_envs = h->n_envs;
  h->d_ctrl_norm.reset();   // the statistics belonged to the controller that was replaced
  ca.norm_mean = ca.norm_inv_std = nullptr; ca.norm_clip = 0.0f;
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_set_base_controller")); }

int mocca_set_base_controller_norm(mocca_handle h, const float* mean_host, const float* inv_std_host, double clip) {
  using namespace mocca_ctrl;
  ENTRY(h, "mocca_set_base_controller_norm");
  if (!h->d_ctrl_image) return c.needs("a base controller", "mocca_set_base_controller", true);
  if (!mean_host != !inv_std_host) return c.bad("mean_host and inv_std_host must both be given, or both be NULL (detach)");
  DeviceGuard guard(h->device);
  if (!mean_host) {   // detach
    if (int rc = commit_ready(c)) return rc;
    h->d_ctrl_norm.reset();
    h->ctrl.norm_mean = h->ctrl.norm_inv_std = nullptr; h->ctrl.norm_clip = 0.0f;
    return MOCCA_OK;
  }
  for (int k = 0; k < CTRL_IN; ++k) {
    if (!std::isfinite(mean_host[k])) return c.bad("mean[" + std::to_string(k) + "] is not finite");
    if (!std::isfinite(inv_std_host[k]) || inv_std_host[k] < 0.0f) return c.bad("inv_std[" + std::to_string(k) + "] is not finite or is negative");
  }
  if (!std::isfinite(clip) || !(clip > 0.0)) return c.bad("clip must be finite and positive");
  float host[2 * CTRL_IN];
  std::memcpy(host, mean_host, CTRL_IN * sizeof(float));
  std::memcpy(host + CTRL_IN, inv_std_host, CTRL_IN * sizeof(float));
  DevBuf<float> norm;
  hipError_t e = norm.alloc(2 * CTRL_IN, false);
  if (e == hipSuccess) e = hipMemcpy(norm, host, sizeof(host), hipMemcpyHostToDevice);
  if (int rc = commit_ready(c, e)) return rc;
  h->d_ctrl_norm.swap(norm);
  h->ctrl.norm_mean = h->d_ctrl_norm; h->ctrl.norm_inv_std = h->d_ctrl_norm.get() + CTRL_IN; h->ctrl.norm_clip = (float)clip;
  return MOCCA_OK;
}

// the base controller's launch of mocca_plan_step / mocca_act_plan_step: the plans in, d_base_act and d_base_val out; the handle's device is current
static int run_controller(const Call& c, const float* plan_dev, hipStream_t s) {
  mocca_ctrl::ControllerArgs a = c.h->ctrl;
  a.plan = plan_dev;
  mocca_ctrl::launch_controller(s, a);
  return c.launched();
}

int mocca_plan_step(mocca_handle h, const float* plan_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
                    void* stream) {
  ENTRY(h, "mocca_plan_step");
  if (!plan_dev || !obs_dev || !rew_dev || !done_dev) return c.null_arg("plan_dev, obs_dev, rew_dev and done_dev");
  if (!h->d_ctrl_image) return c.needs("a base controller", "mocca_set_base_controller");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = run_controller(c, plan_dev, s)) return rc;
  return launch_step(c, h->d_base_act, h->d_base_val, obs_dev, rew_dev, done_dev, info_dev, s);
}

// detach the policy's mirror attachment, whichever kind it is; the caller has made sure that no launch in flight reads the tables
static void drop_policy_mirror(mocca_handle h) {
  h->pol_mirror.perm.reset(); h->pol_mirror.sign.reset();
  h->pol_mirror.method = mocca_ppo::PPO_PLAIN; h->pol_mirror.coef = 0.0;
  h->student.pol.in_perm = h->student.pol.act_perm = nullptr;
  h->student.pol.in_sign = h->student.pol.act_sign = nullptr;
}

// mocca_set_policy (the student's slot: the mirror attachment goes with the old shapes) and mocca_set_teacher (the teacher's): attach,
// replace or (layers_host NULL) detach the slot's policy image.  A refused call leaves the handle as it was.
// `priv` (mocca_set_policy_priv, the student's slot): the critic's first layer takes critic_in_dim inputs and the image carries its statistics.
// Either student call drops the critic-row binding (mocca_set_critic_rows): its stride was checked against the old shapes.
static int set_policy_slot(const Call& c, bool student, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim,
                           double clip, bool priv = false, int critic_in_dim = 0) try {
  using namespace mocca_pol;
  if (!c.h) return c.null_handle();
  const mocca_handle h = c.h;
  mocca_ctx::PolicySlot& slot = student ? h->student : h->teacher;
  DeviceGuard guard(h->device);
  if (priv && h->pol_mirror.method != mocca_ppo::PPO_PLAIN)   // also for a detach: the caller says what goes first
    return c.bad(std::string("a mirror attachment is in place (") + (h->pol_mirror.method == mocca_ppo::PPO_SYM ? "mocca_set_policy_symmetry" : h->pol_mirror.method == mocca_ppo::PPO_MIRROR ? "mocca_set_policy_mirror_loss" : "mocca_set_policy_mirror_dup") +
               "): mirror tables for the critic's row are not provided, detach it first");
  if (!layers_host) {   // detach
    if (int rc = commit_ready(c)) return rc;
    slot.d_pol_image.reset(); slot.d_pol_layers.reset(); slot.pol_filled = false;
    if (student) { drop_policy_mirror(h); h->critic_rows = nullptr; h->critic_stride = 0; slot.pol.critic_in_dim = 0; }
    return MOCCA_OK;
  }
  if (in_dim < 1 || in_dim > POL_MAX_IN) return c.bad("in_dim must be 1 .. " + std::to_string(POL_MAX_IN));
  if (priv && (critic_in_dim < 1 || critic_in_dim > POL_MAX_IN)) return c.bad("critic_in_dim must be 1 .. " + std::to_string(POL_MAX_IN));
  if (act_dim < 1 || act_dim > POL_MAX_ACTION) return c.bad("act_dim must be 1 .. " + std::to_string(POL_MAX_ACTION));
  if (!std::isfinite(clip) || !(clip > 0.0)) return c.bad("clip must be finite and positive");
  int count[2];
  const std::string takes = priv ? "the actor's first layer takes in_dim = " + std::to_string(in_dim) + " inputs and the critic's critic_in_dim = " +
                                       std::to_string(critic_in_dim) + ", not %d"
                                 : "a net's first layer takes in_dim = " + std::to_string(in_dim) + " inputs, not %d";
  const std::string wrong = check_layer_table(layers_host, n_layers_total, in_dim, act_dim, NO_OFFSETS, takes,
                                              "the actor ends in act_dim = " + std::to_string(act_dim) + " outputs, the critic in 1", count,
                                              priv ? critic_in_dim : 0);
  if (!wrong.empty()) return c.bad(wrong);
  NetImage im;
  if (int rc = commit_ready(c, build_image(im, layers_host, n_layers_total, count, in_dim, act_dim, true, priv ? critic_in_dim : 0))) return rc;
  if (student) { h->critic_rows = nullptr; h->critic_stride = 0; }
  slot.d_pol_image.swap(im.image); slot.d_pol_layers.swap(im.layers);
  slot.pol = im.pa; slot.pol.clip = (float)clip;
  slot.pol_repack = im.rp; slot.pol_n_base = im.n_src; slot.pol_filled = false;
  slot.pol_tail_row = im.tail_row; slot.pol_table.swap(im.table);
  std::memcpy(slot.pol_wt_off, im.wt_off, sizeof(im.wt_off));
  if (student) drop_policy_mirror(h);   // the shapes may have changed
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(c); }

int mocca_set_policy(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim, double clip) {
  return set_policy_slot(Call(h, "mocca_set_policy"), true, layers_host, n_layers_total, in_dim, act_dim, clip);
}

int mocca_set_policy_priv(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int critic_in_dim, int act_dim, double clip) {
  return set_policy_slot(Call(h, "mocca_set_policy_priv"), true, layers_host, n_layers_total, in_dim, act_dim, clip, true, critic_in_dim);
}

int mocca_set_critic_rows(mocca_handle h, const float* rows_dev, int row_stride) {
  ENTRY(h, "mocca_set_critic_rows");
  if (!rows_dev) { h->critic_rows = nullptr; h->critic_stride = 0; return MOCCA_OK; }   // detach
  const mocca_pol::PolicyArgs& p = h->student.pol;
  if (!h->student.d_pol_image || !p.critic_in_dim)
    return c.bad("needs a policy with a privileged critic (mocca_set_policy_priv): the plain policy's critic reads mocca_act's in_dev");
  if (row_stride < p.critic_in_dim)
    return c.small_stride("row_stride", row_stride, "the policy's critic_in_dim (" + std::to_string(p.critic_in_dim) + ")");
  h->critic_rows = rows_dev; h->critic_stride = row_stride;
  return MOCCA_OK;
}

int mocca_set_teacher(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim, double clip) {
  return set_policy_slot(Call(h, "mocca_set_teacher"), false, layers_host, n_layers_total, in_dim, act_dim, clip);
}

// The rules of one mirror table (mocca_policy.h: Symmetry): -> "" or what is wrong with the first entry that breaks one.
static std::string check_mirror_table(const int32_t* perm, const float* sign, int dim, const char* perm_name, const char* sign_name) {
  for (int k = 0; k < dim; ++k) {
    const std::string at = std::string(perm_name) + "[" + std::to_string(k) + "]";
    if (perm[k] < 0 || perm[k] >= dim) return at + " = " + std::to_string(perm[k]) + " is outside 0 .. " + std::to_string(dim - 1);
    if (!(sign[k] == 1.0f || sign[k] == -1.0f)) return std::string(sign_name) + "[" + std::to_string(k) + "] must be +1 or -1";
  }
  for (int k = 0; k < dim; ++k) {
    const std::string at = std::string(perm_name) + "[" + std::to_string(k) + "]";
    if (perm[perm[k]] != k) return at + ": the permutation is not an involution (perm[perm[k]] != k)";
    if (sign[perm[k]] != sign[k]) return at + ": " + sign_name + " differs across the swapped pair (M M must be the identity)";
  }
  return "";
}

// The four mirror tables of a policy, checked and copied to the device: perm = in_perm [in_dim] then act_perm [act_dim], sign likewise.
// -> "" with *e set (the copies' status), or what is wrong with the tables (nothing allocated).
static std::string upload_mirror_tables(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                                        const float* act_sign_host, DevBuf<int32_t>& d_perm, DevBuf<float>& d_sign, hipError_t* e) {
  if (!in_sign_host || !act_perm_host || !act_sign_host) return "in_sign_host, act_perm_host and act_sign_host must not be NULL";
  const int in_dim = h->student.pol.in_dim, act_dim = h->student.pol.act_dim;
  std::string wrong = check_mirror_table(in_perm_host, in_sign_host, in_dim, "in_perm", "in_sign");
  if (wrong.empty()) wrong = check_mirror_table(act_perm_host, act_sign_host, act_dim, "act_perm", "act_sign");
  if (!wrong.empty()) return wrong;
  std::vector<int32_t> perm(in_perm_host, in_perm_host + in_dim);
  perm.insert(perm.end(), act_perm_host, act_perm_host + act_dim);
  std::vector<float> sign(in_sign_host, in_sign_host + in_dim);
  sign.insert(sign.end(), act_sign_host, act_sign_host + act_dim);
  *e = d_perm.alloc(perm.size(), false);
  if (*e == hipSuccess) *e = d_sign.alloc(sign.size(), false);
  if (*e == hipSuccess) *e = hipMemcpy(d_perm, perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (*e == hipSuccess) *e = hipMemcpy(d_sign, sign.data(), sign.size() * sizeof(float), hipMemcpyHostToDevice);
  return "";
}

// mocca_set_policy_symmetry (PPO_SYM), mocca_set_policy_mirror_loss (PPO_MIRROR) and mocca_set_policy_mirror_dup (PPO_DUP): attach `method`'s
// tables, replace them, or (in_perm_host NULL) detach them.  One kind at a time: a second kind is refused, and detaching a kind that is not the
// attached one leaves the attached one alone.  A table error or a failed upload leaves the handle as it was.
static int set_policy_mirror(const Call& c, mocca_ppo::PpoMode method, const int32_t* in_perm_host, const float* in_sign_host,
                             const int32_t* act_perm_host, const float* act_sign_host, double mirror_coef) try {
  using namespace mocca_ppo;
  if (!c.h) return c.null_handle();
  const mocca_handle h = c.h;
  DeviceGuard guard(h->device);
  if (!h->student.d_pol_image) return c.needs("a policy", "mocca_set_policy", true);
  if (in_perm_host && h->student.pol.critic_in_dim)
    return c.bad("the policy has a privileged critic (mocca_set_policy_priv): mirror tables for the critic's row are not provided, set a plain policy first (mocca_set_policy)");
  if (!in_perm_host) {   // detach
    if (int rc = commit_ready(c)) return rc;
    if (h->pol_mirror.method == method) drop_policy_mirror(h);
    return MOCCA_OK;
  }
  static const char* const refusal[4][4] = {   // [method][the attached kind]
      {},
      {nullptr, nullptr, "a mirror loss is attached (mocca_set_policy_mirror_loss): a symmetric network has no mirror loss, detach it first",
       "duplicated rows are attached (mocca_set_policy_mirror_dup): they train the plain policy, detach them first"},
      {nullptr, "the policy is mirror-symmetric (mocca_set_policy_symmetry): its mirror loss is zero by construction, detach the symmetry first", nullptr,
       "duplicated rows are attached (mocca_set_policy_mirror_dup): one symmetry method at a time, detach them first"},
      {nullptr, "the policy is mirror-symmetric (mocca_set_policy_symmetry): a row and its mirror image give it one gradient, detach the symmetry first",
       "a mirror loss is attached (mocca_set_policy_mirror_loss): one symmetry method at a time, detach it first", nullptr}};
  static_assert(PPO_PLAIN == 0 && PPO_SYM == 1 && PPO_MIRROR == 2 && PPO_DUP == 3, "refusal[][]'s rows and columns");
  if (const char* why = refusal[method][h->pol_mirror.method]) return c.bad(why);
  if (!std::isfinite(mirror_coef) || mirror_coef < 0.0) return c.bad("mirror_coef must be finite and not negative");
  DevBuf<int32_t> d_perm;
  DevBuf<float> d_sign;
  hipError_t e = hipSuccess;
  const std::string wrong = upload_mirror_tables(h, in_perm_host, in_sign_host, act_perm_host, act_sign_host, d_perm, d_sign, &e);
  if (!wrong.empty()) return c.bad(wrong);
  if (int rc = commit_ready(c, e)) return rc;
  h->pol_mirror.perm.swap(d_perm); h->pol_mirror.sign.swap(d_sign);
  h->pol_mirror.method = method; h->pol_mirror.coef = mirror_coef;
  if (method == PPO_SYM) {   // the policy kernel's symmetric instance runs from here on (launch_policy)
    const int in_dim = h->student.pol.in_dim;
    h->student.pol.in_perm = h->pol_mirror.perm; h->student.pol.act_perm = h->pol_mirror.perm.get() + in_dim;
    h->student.pol.in_sign = h->pol_mirror.sign; h->student.pol.act_sign = h->pol_mirror.sign.get() + in_dim;
  }
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(c); }

int mocca_set_policy_symmetry(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                              const float* act_sign_host) {
  return set_policy_mirror(Call(h, "mocca_set_policy_symmetry"), mocca_ppo::PPO_SYM, in_perm_host, in_sign_host, act_perm_host, act_sign_host, 0.0);
}

int mocca_set_policy_mirror_loss(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                                 const float* act_sign_host, double mirror_coef) {
  return set_policy_mirror(Call(h, "mocca_set_policy_mirror_loss"), mocca_ppo::PPO_MIRROR, in_perm_host, in_sign_host, act_perm_host, act_sign_host, mirror_coef);
}

int mocca_set_policy_mirror_dup(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                                const float* act_sign_host) {
  return set_policy_mirror(Call(h, "mocca_set_policy_mirror_dup"), mocca_ppo::PPO_DUP, in_perm_host, in_sign_host, act_perm_host, act_sign_host, 0.0);
}

// mocca_update_policy and mocca_update_teacher: new weights for the slot's image, one repack launch
static int update_policy_slot(const Call& c, const char* setter, bool student, const float* params_dev, size_t n_floats,
                              void* stream) {
  if (!c.h) return c.null_handle();
  const mocca_handle h = c.h;
  mocca_ctx::PolicySlot& slot = student ? h->student : h->teacher;
  if (!slot.d_pol_image) return c.needs("a policy", setter);
  if (!params_dev) return c.null_arg("params_dev");
  const std::string wrong = check_n_floats(slot, n_floats);
  if (!wrong.empty()) return c.bad("" + wrong);
  DeviceGuard guard(h->device);
  repack_policy(slot, params_dev, n_floats, (hipStream_t)stream);
  HIP_TRY(c, hipGetLastError());
  slot.pol_filled = true;
  return MOCCA_OK;
}

int mocca_update_policy(mocca_handle h, const float* params_dev, size_t n_floats, void* stream) {
  return update_policy_slot(Call(h, "mocca_update_policy"), "mocca_set_policy", true, params_dev, n_floats, stream);
}

int mocca_update_teacher(mocca_handle h, const float* params_dev, size_t n_floats, void* stream) {
  return update_policy_slot(Call(h, "mocca_update_teacher"), "mocca_set_teacher", false, params_dev, n_floats, stream);
}

// mocca_teacher_act: the teacher's slot through the policy kernel's plain instance, deterministic, over n_rows rows.  That path of the kernel
// reads no env record and no noise; the mean IS the deterministic action, so mean_dev stands in the kernel's action output.
int mocca_teacher_act(mocca_handle h, const float* in_dev, int in_stride, int64_t n_rows, float* mean_dev, float* value_dev, void* stream) {
  ENTRY(h, "mocca_teacher_act");
  const mocca_ctx::PolicySlot& slot = h->teacher;
  if (!slot.d_pol_image || !slot.pol_filled) return c.bad("needs a teacher (mocca_set_teacher, then mocca_update_teacher)");
  if (!in_dev || !mean_dev) return c.null_arg("in_dev and mean_dev");
  if (in_stride < slot.pol.in_dim)
    return c.small_stride("in_stride", in_stride, "the teacher's in_dim (" + std::to_string(slot.pol.in_dim) + ")");
  if (n_rows < 1 || n_rows > mocca_ppo::PPO_MAX_ROWS) return c.bad("n_rows must be 1 .. 2^22, not " + std::to_string(n_rows));
  DeviceGuard guard(h->device);
  mocca_pol::PolicyArgs a = slot.pol;   // (a teacher has no mirror tables: the plain instance)
  a.in = in_dev; a.in_stride = in_stride; a.eps = nullptr; a.deterministic = 1;
  a.action = mean_dev; a.logp = nullptr; a.value = value_dev; a.mean = nullptr; a.n_envs = (int)n_rows;
  mocca_pol::launch_policy((hipStream_t)stream, a);
  return c.launched();
}

// the policy kernel's launch of mocca_act / mocca_act_step; the handle's device is current
static int launch_act(const Call& c, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev,
                      float* logp_dev, float* value_dev, float* mean_dev, hipStream_t s) {
  const mocca_handle h = c.h;
  if (!h->student.d_pol_image || !h->student.pol_filled) return c.needs("a policy", "mocca_set_policy, then mocca_update_policy");
  if (!in_dev || !action_dev) return c.null_arg("in_dev and action_dev");
  if (in_stride < h->student.pol.in_dim) return c.small_stride("in_stride", in_stride, "the policy's in_dim (" + std::to_string(h->student.pol.in_dim) + ")");
  if ((long long)h->env_offset + h->n_envs > (1ll << 28) || h->env_offset < 0)
    return c.bad("the noise is keyed by global env ids below 2^28 (MOCCA_PARAM_ENV_OFFSET + n_envs)");
  if (h->student.pol.critic_in_dim && value_dev && !h->critic_rows)
    return c.bad("the policy's critic reads rows of its own: bind them (mocca_set_critic_rows), or pass value_dev NULL");
  mocca_pol::PolicyArgs a = h->student.pol;
  a.critic_in = h->critic_rows; a.critic_stride = h->critic_stride;
  a.in = in_dev; a.in_stride = in_stride; a.eps = eps_dev; a.deterministic = deterministic != 0;
  a.task = h->d_task; a.task_words = MOCCA_TASK_WORDS; a.tw_t = MOCCA_TW_T; a.tw_episode = MOCCA_TW_EPISODE;
  a.env_offset = h->env_offset; a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
  a.action = action_dev; a.logp = logp_dev; a.value = value_dev; a.mean = mean_dev; a.n_envs = h->n_envs;
  mocca_pol::launch_policy(s, a);
  return c.launched();
}

int mocca_act(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev, float* logp_dev,
              float* value_dev, float* mean_dev, void* stream) {
  ENTRY(h, "mocca_act");
  DeviceGuard guard(h->device);
  return launch_act(c, in_dev, in_stride, eps_dev, deterministic, action_dev, logp_dev, value_dev, mean_dev, (hipStream_t)stream);
}

int mocca_act_step(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev, float* logp_dev,
                   float* value_dev, float* mean_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  ENTRY(h, "mocca_act_step");
  if (!obs_dev || !rew_dev || !done_dev) return c.null_arg("obs_dev, rew_dev and done_dev");
  if (h->student.d_pol_image && h->student.pol.act_dim != mocca_act_dim(h))
    return c.bad("the policy's act_dim (" + std::to_string(h->student.pol.act_dim) + ") is not the env's (" + std::to_string(mocca_act_dim(h)) + ")");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_act(c, in_dev, in_stride, eps_dev, deterministic, action_dev, logp_dev, value_dev, mean_dev, s)) return rc;
  return launch_step(c, action_dev, nullptr, obs_dev, rew_dev, done_dev, info_dev, s);
}

int mocca_act_plan_step(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* plan_dev, float* logp_dev,
                        float* value_dev, float* mean_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  ENTRY(h, "mocca_act_plan_step");
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return c.bad("only the planner task takes plans");
  if (!obs_dev || !rew_dev || !done_dev) return c.null_arg("obs_dev, rew_dev and done_dev");
  if (!h->d_ctrl_image) return c.needs("a base controller", "mocca_set_base_controller");
  if (h->student.d_pol_image && h->student.pol.act_dim != mocca_ctrl::CTRL_PLAN)
    return c.bad("the policy's act_dim (" + std::to_string(h->student.pol.act_dim) + ") is not the plan's (" + std::to_string(mocca_ctrl::CTRL_PLAN) + ")");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_act(c, in_dev, in_stride, eps_dev, deterministic, plan_dev, logp_dev, value_dev, mean_dev, s)) return rc;
  if (int rc = run_controller(c, plan_dev, s)) return rc;
  return launch_step(c, h->d_base_act, h->d_base_val, obs_dev, rew_dev, done_dev, info_dev, s);
}

}  // extern "C"
