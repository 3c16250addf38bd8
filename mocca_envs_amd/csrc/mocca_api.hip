// mocca_api.hip -- kernels' entry points and the C ABI of libmocca_hip.so (include/mocca.h).
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see mocca_envs_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "mocca.h"
#include "mocca_kernels.h"
#include "mocca_optim.h"
#include "mocca_policy.h"
#include "mocca_ppo.h"
#include "mocca_render.h"
#include "mocca_rollout.h"
#include "mocca_scan.h"
#include "mocca_depth.h"
#include "mocca_terrain.h"
#include "mocca_randomise.h"
#include "mocca_history.h"

using namespace mocca;

// the compact instance of the step kernel (mocca_r32.hip)
extern "C" size_t mocca_r32_args_sizeof(void);
extern "C" int mocca_r32_max_rows(void);
extern "C" int mocca_r32_max_contacts(void);
extern "C" void mocca_r32_launch_step(int topo, int task_id, int n, hipStream_t s, const void* args);
extern "C" void mocca_r32_kernel_info(int topo, int task_id, hipFuncAttributes* fa, int* nb, hipError_t* e);
// the 64-row / 20-contact accuracy instance (mocca_r64.hip)
extern "C" size_t mocca_r64_args_sizeof(void);
extern "C" int mocca_r64_max_rows(void);
extern "C" int mocca_r64_max_contacts(void);
extern "C" void mocca_r64_launch_step(int topo, int task_id, int n, hipStream_t s, const void* args);
extern "C" void mocca_r64_kernel_info(int topo, int task_id, hipFuncAttributes* fa, int* nb, hipError_t* e);

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
__global__ void copy_param_kernel(float* dst, const float* src, bool broadcast, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[broadcast ? 0 : i];
}
__global__ void set_task_word_kernel(uint32_t* task, int word, const float* vals, float scalar, int use_scalar, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) task[(size_t)i * MOCCA_TASK_WORDS + word] = __float_as_uint(use_scalar ? scalar : vals[i]);
}

// Launch order of the step kernel (MOCCA_PARAM_ORDER_EVERY): a counting sort of the envs by the constraint-row count their last step ended
// with (task word 23, 0 .. 63), most rows first.  One workgroup; the order inside a bucket is whatever the atomics make it -- it only
// decides when an env's wave starts.  ~6 us for 8192 envs, every K-th step.
__global__ __launch_bounds__(1024) void order_by_rows_kernel(const uint32_t* task, int32_t* order, int n) {
  __shared__ int hist[64], start[64];
  const int t = threadIdx.x;
  if (t < 64) hist[t] = 0;
  __syncthreads();
  for (int e = t; e < n; e += 1024) {
    const uint32_t r = task[(size_t)e * MOCCA_TASK_WORDS + MOCCA_TW_LAST_ROWS];
    atomicAdd(&hist[63 - (r > 63u ? 63u : r)], 1);   // bucket 0 = heaviest
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < 64; ++k) { start[k] = acc; acc += hist[k]; }
  }
  __syncthreads();
  for (int e = t; e < n; e += 1024) {
    const uint32_t r = task[(size_t)e * MOCCA_TASK_WORDS + MOCCA_TW_LAST_ROWS];
    order[atomicAdd(&start[63 - (r > 63u ? 63u : r)], 1)] = e;
  }
}

// Owner of one device allocation: move-only, freed by its destructor.  Whatever the handle owns on the device is one of these, so destroying
// the handle frees it; a setter builds its new buffers in locals and swaps them into the handle after its last fallible step (commit_ready),
// and the locals' destructors free whichever side lost: the new buffers of a refused call, the old ones of a successful one.
template <class T>
class DevBuf {
  T* p_ = nullptr;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }   // (the source's destructor frees what this one held)
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); }
  // `count` elements in place of what it held, zero-filled on request; empty when that fails
  hipError_t alloc(size_t count, bool zero) {
    reset();
    hipError_t e = hipMalloc(&p_, count * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return e; }
    if (zero && (e = hipMemset(p_, 0, count * sizeof(T))) != hipSuccess) reset();
    return e;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
};

struct mocca_ctx {
  MoccaModel model;
  int task_id = 0, n_envs = 0, device = 0, obs_dim = 0;
  DevBuf<MoccaModel> d_model;
  int topo = 0;  // TOPO_*
  DevBuf<float> d_dyn;
  DevBuf<uint32_t> d_task;
  DevBuf<float> d_terrain;
  int auto_reset = 0, eval_mode = 0, random_pose = 1, curriculum = 0, host_retarget = 0, env_offset = 0, random_reward = 0;
  float gain = 1.0f;
  bool compact = false;        // the blob fits the compact step-kernel instance (compact_ok); MOCCA_PARAM_KERNEL_VARIANT = 1 overrides
  bool wide = false;           // the blob's caps exceed 48 rows / 12 contacts: the 64-row accuracy instance (mocca_r64.hip)
  int force_full = 0;          // MOCCA_PARAM_KERNEL_VARIANT, bits 0..1: 1 forces the 48-row instance, 2 the 64-row one
  bool delassus_valu = false;  // MOCCA_PARAM_KERNEL_VARIANT, bit 2: the step kernel builds the Delassus matrix on the VALU for every row count
  int persist_warm = 0;        // MOCCA_PARAM_PERSIST_IMPULSES
  int pace = -18;              // MOCCA_PARAM_PACE_TICKS: self-calibrating pace priorities, 18/16 of the previous launch's mean wave time (profiles/archive/r04_pace_*.jsonl)
  DevBuf<unsigned long long> d_pace_acc;     // self-calibration samples of the pace, one packed word (StepArgs.pace_acc), owned by the handle
  // Monitor / TimeLimitMask inside the launch (mocca_set_episode_stats)
  DevBuf<float> d_ep_ret;          // [N] running episode returns, owned by the handle
  float *ep_masks = nullptr, *ep_bad = nullptr, *ep_totals = nullptr;   // caller-owned
  char* ep_rec = nullptr;          // caller-owned record ring: n_slots slots of [N] x 16 bytes, ep_stride bytes apart
  int ep_slots = 0;
  size_t ep_stride = 0;
  uint32_t ep_serial = 1;          // stamped into the records of the next mocca_step (0 never: a zeroed ring holds no record)
  int order_every = 0;         // MOCCA_PARAM_ORDER_EVERY: re-sort the launch order every K steps (0: envs run in index order)
  int order_age = 0;           // steps since the last sort
  DevBuf<int32_t> d_order;     // [N] the permutation, owned by the handle
  bool gain_pending = false;   // a scalar MOCCA_PARAM_APPLIED_GAIN not yet written into the task records (flush_pending)
  float* final_obs = nullptr;  // caller-owned (mocca_set_terminal_obs_buffer)
  DevBuf<float> d_pvec[3];     // per-env curriculum / eval_mode / applied_gain (mocca_set_param_v), lazily allocated
  bool pvec_on[3] = {false, false, false};
  const float* tape = nullptr;  // caller-owned (mocca_set_draw_tape)
  int tape_n = 0;
  int32_t* dbg = nullptr;       // caller-owned (mocca_set_debug_buffer)
  int prio = MOCCA_PRIO_T1 + 64 * MOCCA_PRIO_T2 + 4096 * MOCCA_PRIO_T3;   // MOCCA_PARAM_ISSUE_PRIORITY
  uint64_t seed = 0;
  DevBuf<float> d_traj;         // Cassie mocap / phase envs: the motion table (mocca_set_trajectory), owned by the handle
  int traj_n = 0;
  double traj_tmax = 0.0, traj_cstep = 0.0;
  // planner envs: the terrain bank (mocca_set_heightfield_bank; mocca_set_heightfield attaches a bank of one), all owned by the handle
  DevBuf<float> d_hf;           // [hf_n_fields][hf_planes][rows][cols]: a field's heights, then its max-pooled copies (windows 2 .. hf_planes)
  int hf_rows = 0, hf_cols = 0, hf_n_fields = 0, hf_planes = 1;
  float hf_scale = 0.0f;
  DevBuf<float> d_hf_range;     // [hf_n_fields][2] range of each field's heights (mocca_render clips its rays to it)
  DevBuf<float> d_hf_part;      // [hf_n_fields][blocks][2] scratch of mocca_generate_heightfields' range reduction
  DevBuf<int32_t> d_hf_field;   // [N] the field each env stands on (mocca_set_env_fields)
  int hf_redraw = 0;            // every reset draws the env's field anew
  DevBuf<float> d_scenes;       // mocca_render: world-space primitives of each view, owned by the handle, grown on demand
  int scenes_cap = 0;           // views it holds
  DevBuf<float> d_scan_pts;     // mocca_set_height_scan: the pattern [scan_n][2] in the heading frame, owned by the handle
  int scan_n = 0;
  float scan_above = 0.0f, scan_drop = 0.0f;
  bool depth_on = false;        // mocca_set_depth_camera: the camera, passed to the kernel by value (out, obs and the records apart)
  mocca_depth::DepthArgs depth{};
  // planner envs: the base controller (mocca_set_base_controller), all owned by the handle
  DevBuf<float> d_ctrl_image;        // the kernel's image (mocca_controller.h; the tail of mocca_policy.h's image is there and not read)
  DevBuf<int32_t> d_ctrl_layers;
  mocca_ctrl::ControllerArgs ctrl{}; // everything of mocca_plan_step's launch but the plans
  DevBuf<float> d_robot_state;       // [N][ROBOT_STATE_STRIDE] the controller's next input (StepArgs.robot_state)
  DevBuf<float> d_base_act;          // [N][21] the actor's output of the last mocca_plan_step
  DevBuf<float> d_base_val;          // [N] the critic's
  DevBuf<float> d_ctrl_norm;         // mocca_set_base_controller_norm: mean [65] then inv_std [65]; ctrl.norm_mean / norm_inv_std point into it
  // a policy image and what describes it, owned by the handle.  Two slots: `student`, the trainer's policy (mocca_set_policy: mocca_act, the
  // gradient and the optimiser calls), and `teacher`, a frozen second policy that only mocca_teacher_act evaluates (mocca_set_teacher)
  struct PolicySlot {
    DevBuf<float> d_pol_image;         // the kernel's image (mocca_policy.h)
    DevBuf<int32_t> d_pol_layers;
    mocca_pol::PolicyArgs pol{};       // shapes and image offsets; the per-call pointers are filled by mocca_act / mocca_teacher_act
    mocca_pol::RepackArgs pol_repack{};   // rows of the repack kernel; src offsets in the caller's flat parameters
    size_t pol_n_base = 0;             // floats of mocca_update_policy's params_dev without the normalisation arrays
    bool pol_filled = false;           // mocca_update_policy / mocca_update_teacher has run since the slot was set
    int pol_tail_row = 0;              // pol_repack's row of the flags; the rows of mean and inv_std follow it
    std::vector<int32_t> pol_table;    // host copy of d_pol_layers (offsets into the image)
    int pol_wt_off[mocca_ppo::PPO_MAX_TABLE] = {};   // the layers' transposed copies in the image (mocca_ppo.h), -1: none
  } student, teacher;
  // the student's ONE mirror attachment (set_policy_mirror): the setters refuse a second kind, so the tables are held once
  struct {
    mocca_ppo::PpoMode method = mocca_ppo::PPO_PLAIN;   // PPO_PLAIN: nothing attached.  PPO_SYM (mocca_set_policy_symmetry): pol.in_perm and its
                                     // kin point into the tables; PPO_MIRROR (.._mirror_loss) and PPO_DUP (.._mirror_dup): mocca_ppo_grad_mirror /
                                     // _dup ALONE read them, pol stays plain
    DevBuf<int32_t> perm;            // in_perm [in_dim] then act_perm [act_dim]
    DevBuf<float> sign;              // in_sign [in_dim] then act_sign [act_dim]
    double coef = 0.0;               // PPO_MIRROR: mirror_coef
  } pol_mirror;
  // the student's privileged critic (mocca_set_policy_priv: student.pol.critic_in_dim != 0): the rows its workgroups of mocca_act read
  const float* critic_rows = nullptr;   // caller-owned [n_envs][critic_stride] (mocca_set_critic_rows)
  int critic_stride = 0;
  // scratch of mocca_gae / mocca_obs_stats (mocca_rollout.h), owned by the handle, grown on demand
  DevBuf<double> d_gae_part;         // [blocks][2]
  size_t gae_part_cap = 0;           // doubles
  DevBuf<double> d_obs_part;         // [blocks][dim][2]
  size_t obs_part_cap = 0;
  DevBuf<double> d_ppo;              // scratch of mocca_ppo_grad (mocca_ppo.h), grown on demand
  size_t ppo_cap = 0;
  DevBuf<double> d_optim;            // scratch of mocca_adam_step / mocca_ppo_update (mocca_optim.h): the record, the gradient, the permutation
  size_t optim_cap = 0;
  // domain randomisation (mocca_randomise.h), all owned by the handle
  bool rand_on = false;              // mocca_set_randomisation: launch_step runs the perturb kernel and the step kernel reads d_rand_eff
  mocca_rand::RandConfig rand_cfg{};
  DevBuf<float> d_rand_eff;          // [N][act_dim] the effective action of the last step
  DevBuf<float> d_rand_ring;         // [N][delay_max + 1][act_dim] the stored actions of the last delay_max + 1 steps; NOT part of a snapshot
  DevBuf<float> d_noise_scale;       // [obs_dim] mocca_set_sensor_noise
  // the observation-action history (mocca_history.h), all owned by the handle; hist_cfg.steps == 0: none attached
  mocca_hist::HistConfig hist_cfg{};
  DevBuf<int32_t> d_hist_cols;       // [n_cols] the observation columns of a frame
  DevBuf<float> d_hist_ring;         // [N][steps * stride + 1][n_cols + act_dim] the frames; NOT part of a snapshot
  DevBuf<uint32_t> d_hist_tags;      // [N][steps * stride + 1][2] (episode, step) of the frame a slot holds
  std::string err;
};
static_assert(ROBOT_STATE_STRIDE == mocca_ctrl::CTRL_RS_STRIDE, "the step kernels and the controller kernel share the robot_state buffer");

static thread_local std::string g_err;

#define HIP_TRY(h, expr)                                                         \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) {                                                      \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return MOCCA_E_HIP;                                                        \
    }                                                                            \
  } while (0)

// The ABI boundary of the calls that build host images (std::vector, std::string): a failed host allocation is a code and a message.
static int out_of_host_memory(mocca_handle h, const char* who) {
  (h ? h->err : g_err) = std::string(who) + ": out of host memory";
  return MOCCA_E_ARG;
}

// Attach / replace / detach of what a handle owns (mocca_set_*, mocca_render's scenes) is one sequence: validate; build the new buffers in local
// DevBufs and upload (`e`: how that went); commit_ready; swap the locals into the handle and set its scalar fields.  commit_ready is the last
// step that can fail, so a refused call leaves the handle exactly as it was; after it no launch in flight still reads the old buffers.
static int commit_ready(mocca_handle h, const char* who, hipError_t e = hipSuccess) {
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) return MOCCA_OK;
  h->err = std::string(who) + ": " + hipGetErrorString(e);
  return MOCCA_E_HIP;
}

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

// does the blob give mass or inertia to a link the compiled topology T treats as massless?
template <class T>
static bool massive_intermediates(const MoccaModel& m) {
  for (int b = 1; b < T::NB; ++b)
    if (T::massless(b)) {
      bool zero = m.mass[b] == 0.0f;
      for (int i = 0; i < 6; ++i) zero = zero && m.inertia[b][i] == 0.0f;
      if (!zero) return true;
    }
  return false;
}
template <class T>
static int check_topology_t(const MoccaModel& m, const char* name, std::string& err) {
  if (m.n_bodies != T::NB || m.n_joints != T::NJ || m.n_geoms > T::NG || m.n_slots > T::NSLOT || m.n_closures != T::NCLOS) {
    err = std::string("model blob sizes differ from the compiled topology (") + name + ")";
    return MOCCA_E_TOPOLOGY;
  }
  for (int b = 0; b < T::NB; ++b)
    if (m.parent[b] != T::parent(b) || m.anc_mask[b] != T::anc_mask(b)) {
      err = std::string("model blob tree differs from the compiled topology (") + name + ")";
      return MOCCA_E_TOPOLOGY;
    }
  if (massive_intermediates<T>(m)) {   // the ABA inward pass of T does not read the link inertia of a level that holds only such links
    err = std::string("model blob gives mass to a link the compiled topology treats as massless (") + name + ")";   // (check_topology picks the
    return MOCCA_E_TOPOLOGY;                                                                                      // ...Massive instance first)
  }
  if (m.n_pairs > 0 && 6 * T::NG > GP_FLOATS) {
    err = std::string("this topology's geom points overlap the contact records: blobs with self-collision pairs are not supported (") + name + ")";
    return MOCCA_E_ARG;
  }
  if (m.max_rows > mocca_r64_max_rows() || m.max_contacts > mocca_r64_max_contacts() || m.max_rows < 1 + 3 * T::NCLOS + (T::NCLOS > 0 && m.planar ? 3 : 0) ||
      m.n_pairs > MOCCA_MAX_PAIRS || m.n_feet != T::NFEET || m.n_ctrl > MOCCA_MAX_CTRL || m.n_ordered > MOCCA_MAX_CTRL) {
    err = "model blob caps exceed the kernel's (max_rows <= 64 and >= 1 + the closure / planar rows, max_contacts <= 20 -- beyond 48 / 12 the 64-row instance runs --, n_feet as compiled)";
    return MOCCA_E_ARG;
  }
  return MOCCA_OK;
}
static int check_topology(const MoccaModel& m, int task_id, int* topo, std::string& err) {
  // A blob that gives mass or inertia to the intermediate links of multi-hinge joints (PyBullet's importer may: pybullet_dump.py) runs on
  // the instance of the same tree that reads every link's inertia in the ABA inward pass.
  if (task_id == MOCCA_TASK_CASSIE) {
    if (m.n_bodies == TopoCassie::NB && massive_intermediates<TopoCassie>(m)) {
      *topo = TOPO_CASSIE_MASSIVE; return check_topology_t<TopoCassieMassive>(m, "TopoCassieMassive", err);
    }
    *topo = TOPO_CASSIE; return check_topology_t<TopoCassie>(m, "TopoCassie", err);
  }
  if (task_id == MOCCA_TASK_WALKER3D_CUSTOM && m.n_bodies == TopoWalker2D::NB) {
    *topo = TOPO_WALKER2D; return check_topology_t<TopoWalker2D>(m, "TopoWalker2D", err);
  }
  if (task_id == MOCCA_TASK_WALKER3D_CUSTOM && m.n_bodies == TopoCrab2D::NB) {
    *topo = TOPO_CRAB2D; return check_topology_t<TopoCrab2D>(m, "TopoCrab2D", err);
  }
  if (task_id == MOCCA_TASK_WALKER3D_PLANNER && m.n_bodies != TopoWalker3D::NB) {
    err = "the planner task runs on the Walker3D tree (Walker3DPlannerEnv, MikePlannerEnv)";
    return MOCCA_E_TOPOLOGY;
  }
  if ((task_id == MOCCA_TASK_WALKER3D_CUSTOM || task_id == MOCCA_TASK_WALKER3D_STEPPER) && m.n_bodies == TopoLaikago::NB) {
    *topo = TOPO_LAIKAGO; return check_topology_t<TopoLaikago>(m, "TopoLaikago", err);   // LaikagoCustomEnv / LaikagoStepperEnv
  }
  if (m.n_bodies == TopoWalker3D::NB && massive_intermediates<TopoWalker3D>(m)) {
    *topo = TOPO_WALKER3D_MASSIVE; return check_topology_t<TopoWalker3DMassive>(m, "TopoWalker3DMassive", err);
  }
  *topo = TOPO_WALKER3D;
  return check_topology_t<TopoWalker3D>(m, "TopoWalker3D", err);
}

// A blob whose caps fit 32 rows / 10 contacts on a tree without loop closures runs the compact instance of the step kernel (less LDS per
// env: more resident waves).  Same arithmetic, same order: which instance runs is not observable in the results.
static bool compact_ok(const MoccaModel& m, int topo) {
  return topo != TOPO_CASSIE && topo != TOPO_CASSIE_MASSIVE && m.n_closures == 0 && m.max_rows <= mocca_r32_max_rows() &&
         m.max_contacts <= mocca_r32_max_contacts() && mocca_r32_args_sizeof() == sizeof(StepArgs);
}
// ... and one whose caps exceed the 48-row instance's (48 rows / 12 contacts) runs the 64-row accuracy instance
// ... or that asks for Bullet's alternating sweep direction of the non-contact rows (compiled into that instance only: mocca_device.h ALT_SWEEPS)
static bool wide_needed(const MoccaModel& m) { return m.max_rows > MAXR || m.max_contacts > MAXC || m.sweep_alternate != 0; }
enum { INST_FULL = 0, INST_COMPACT = 1, INST_WIDE = 2 };
template <class T, int TASK> struct LaunchStep {
  static void run(int n, hipStream_t s, StepArgs a) { hipLaunchKernelGGL((mocca_step_kernel<T, TASK>), dim3(n), dim3(64), 0, s, a); }
};
template <class T, int TASK> struct LaunchReset {
  static void run(int n, hipStream_t s, StepArgs a) { hipLaunchKernelGGL((mocca_reset_kernel<T, TASK>), dim3(n), dim3(64), 0, s, a); }
};
template <class T, int TASK> struct LaunchObserve {
  static void run(int n, hipStream_t s, StepArgs a) { hipLaunchKernelGGL((mocca_observe_kernel<T, TASK>), dim3(n), dim3(64), 0, s, a); }
};
template <class T, int TASK> struct KernelInfo {
  static void run(hipFuncAttributes* fa, int* nb, hipError_t* e) {
    *e = hipFuncGetAttributes(fa, (const void*)mocca_step_kernel<T, TASK>);
    if (*e == hipSuccess) *e = hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, mocca_step_kernel<T, TASK>, 64, 0);
  }
};

// The handle's buffers live on h->device: launches and copies are issued with that device current, whatever the
// caller's current device is (restored on return).  hipGetDevice / hipSetDevice are thread-local bookkeeping.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) err = hipSetDevice(dev); else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// which instance of the step kernel a handle's mocca_step launches (reset / observe / task-step kernels exist once)
static int step_instance(const mocca_ctx* h) {
  if (h->wide || h->force_full == 2) return INST_WIDE;
  if (h->compact && !h->force_full) return INST_COMPACT;
  return INST_FULL;
}

// copy_param_kernel / set_task_word_kernel: one thread per env, 256 to a workgroup
template <class... P>
static void launch_per_env(void (*kernel)(P...), mocca_handle h, hipStream_t s, std::common_type_t<P>... args) {
  hipLaunchKernelGGL(kernel, dim3((h->n_envs + 255) / 256), dim3(256), 0, s, args...);
}

extern "C" {

int mocca_abi_version(void) { return MOCCA_ABI_VERSION; }
size_t mocca_model_sizeof(void) { return sizeof(MoccaModel); }

const char* mocca_last_error(mocca_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

int mocca_create(const void* model_blob, size_t nbytes, int task_id, int n_envs, int device, mocca_handle* out) try {
  if (!out) return MOCCA_E_ARG;
  *out = nullptr;
  if (!model_blob || nbytes != sizeof(MoccaModel)) { g_err = "model blob has the wrong size"; return MOCCA_E_ARG; }
  if (n_envs <= 0) { g_err = "n_envs must be positive"; return MOCCA_E_ARG; }
  if (task_id != MOCCA_TASK_WALKER3D_CUSTOM && task_id != MOCCA_TASK_WALKER3D_STEPPER && task_id != MOCCA_TASK_CASSIE &&
      task_id != MOCCA_TASK_WALKER3D_PLANNER) {
    g_err = "unknown task id"; return MOCCA_E_ARG;
  }
  std::unique_ptr<mocca_ctx> h(new mocca_ctx());   // (every return below that is not the last one frees it, and with it what it owns on the device)
  std::memcpy(&h->model, model_blob, sizeof(MoccaModel));
  if (h->model.magic != MOCCA_MODEL_MAGIC || h->model.version != MOCCA_MODEL_VERSION) { g_err = "bad model blob magic/version"; return MOCCA_E_ARG; }
  int rc = check_topology(h->model, task_id, &h->topo, g_err);
  if (rc != MOCCA_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) { g_err = "no such HIP device"; return MOCCA_E_NODEVICE; }
  h->task_id = task_id; h->n_envs = n_envs; h->device = device;
  h->compact = compact_ok(h->model, h->topo);
  h->wide = wide_needed(h->model);
  if (h->wide && mocca_r64_args_sizeof() != sizeof(StepArgs)) { g_err = "the 64-row kernel instance was built from another StepArgs"; return MOCCA_E_ARG; }
  // pace priorities make the waves of a SIMD finish together -- right when all of a batch is resident (or whole generations are); the compact
  // instance exists for batches beyond one generation, whose partial last generation wants its slots refilled one by one: measured 1.5 - 2.5 %
  // slower with the pace than with the row-count priorities (8192 / 16384 envs), so its default is off
  if (h->compact) h->pace = 0;
  h->obs_dim = task_id == MOCCA_TASK_CASSIE
                   ? (h->model.cassie_mode == MOCCA_CASSIE_PLAIN ? 6 + 2 * h->model.n_ordered + 2 : 12 + 2 * h->model.n_ordered + 2)  // env_cassie.py:344-346 / :633
                   : 6 + 2 * h->model.n_joints + h->model.n_feet + (task_id == MOCCA_TASK_WALKER3D_STEPPER ? 5 * (h->model.lookbehind + 2) : 2);
  if (task_id == MOCCA_TASK_CASSIE && (h->model.cassie_mode < MOCCA_CASSIE_PLAIN || h->model.cassie_mode > MOCCA_CASSIE_PHASE_MIRROR ||
                                       (h->model.cassie_mode != MOCCA_CASSIE_PLAIN && h->model.n_ordered != 14))) {
    g_err = "Cassie blob: unknown cassie_mode (the mocap / phase envs need the 14 ordered joints)"; return MOCCA_E_ARG;
  }
  if (task_id == MOCCA_TASK_WALKER3D_STEPPER &&
      (h->model.n_planks < 1 || h->model.n_planks > MOCCA_MAX_PLANKS || h->model.lookbehind < 1 || h->model.lookbehind > 2)) {
    g_err = "Stepper blob: n_planks must be 1..4 and lookbehind 1 or 2"; return MOCCA_E_ARG;
  }
  auto fail = [&](const char* what, hipError_t e) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return MOCCA_E_HIP;
  };
  hipError_t e;
  DeviceGuard guard(device);  // the caller's current device is restored on return
  if ((e = guard.err) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = h->d_model.alloc(1, false)) != hipSuccess) return fail("hipMalloc(model)", e);
  if ((e = hipMemcpy(h->d_model, &h->model, sizeof(MoccaModel), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy(model)", e);
  const size_t n = (size_t)n_envs;
  if ((e = h->d_dyn.alloc(n * DYN_STRIDE, false)) != hipSuccess) return fail("hipMalloc(state)", e);
  if ((e = h->d_task.alloc(n * MOCCA_TASK_WORDS, false)) != hipSuccess) return fail("hipMalloc(task)", e);
  if ((e = h->d_terrain.alloc(n * TERRAIN_STRIDE, true)) != hipSuccess) return fail("hipMalloc(terrain)", e);
  if ((e = h->d_pace_acc.alloc(1, true)) != hipSuccess) return fail("hipMalloc(pace samples)", e);
  // task records: episode = -1 so the first reset is episode 0; applied_gain = 1
  {
    std::vector<uint32_t> tmp(n * MOCCA_TASK_WORDS);
    const float one = 1.0f;
    uint32_t one_bits; std::memcpy(&one_bits, &one, 4);
    for (size_t i = 0; i < n; ++i) {
      tmp[i * MOCCA_TASK_WORDS + MOCCA_TW_EPISODE] = (uint32_t)-1;
      tmp[i * MOCCA_TASK_WORDS + MOCCA_TW_APPLIED_GAIN] = one_bits;
    }
    if ((e = hipMemcpy(h->d_task, tmp.data(), tmp.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy(task)", e);
  }
  // identity quaternion so an un-reset env is still a valid state
  {
    std::vector<float> tmp(n * DYN_STRIDE);
    for (size_t i = 0; i < n; ++i) tmp[i * DYN_STRIDE + 6] = 1.0f;
    if ((e = hipMemcpy(h->d_dyn, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy(state)", e);
  }
  *out = h.release();
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(nullptr, "mocca_create"); }

int mocca_destroy(mocca_handle h) {
  delete h;   // its DevBufs free the device memory
  return MOCCA_OK;
}

int mocca_n_envs(mocca_handle h) { return h ? h->n_envs : MOCCA_E_ARG; }
int mocca_obs_dim(mocca_handle h) { return h ? h->obs_dim : MOCCA_E_ARG; }
int mocca_act_dim(mocca_handle h) {
  if (!h) return MOCCA_E_ARG;
  return h->task_id == MOCCA_TASK_CASSIE ? h->model.n_ctrl - 2 : h->model.n_joints;
}
int mocca_plan_dim(mocca_handle h) {
  if (!h) return MOCCA_E_ARG;
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) { h->err = "mocca_plan_dim: only the planner task takes plans"; return MOCCA_E_ARG; }
  return mocca_ctrl::CTRL_PLAN;
}
int mocca_state_dim(mocca_handle h) { return h ? MOCCA_STATE_DIM(h->model.n_joints, h->model.n_slots) : MOCCA_E_ARG; }

static StepArgs make_args(mocca_handle h) {
  StepArgs a{};
  a.model = h->d_model; a.dyn = h->d_dyn; a.task = h->d_task; a.terrain = h->d_terrain;
  a.n_envs = h->n_envs; a.obs_dim = h->obs_dim;
  a.auto_reset = h->auto_reset; a.eval_mode = h->eval_mode; a.random_pose = h->random_pose; a.curriculum = h->curriculum;
  a.host_retarget = h->host_retarget; a.env_offset = h->env_offset; a.random_reward = h->random_reward;
  a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
  a.curriculum_v = h->pvec_on[0] ? h->d_pvec[0].get() : nullptr;
  a.eval_mode_v = h->pvec_on[1] ? h->d_pvec[1].get() : nullptr;
  a.gain_v = h->pvec_on[2] ? h->d_pvec[2].get() : nullptr;
  a.gain = h->gain;
  a.dbg = h->dbg;
  a.prio = h->prio | (h->delassus_valu ? PRIO_DELASSUS_VALU : 0);   // (the thresholds take 18 bits)
  a.traj = h->d_traj; a.traj_n = h->traj_n; a.traj_tmax = h->traj_tmax; a.traj_cstep = h->traj_cstep;
  a.final_obs = h->final_obs;
  a.persist_warm = h->persist_warm;
  a.pace = h->pace;
  a.pace_acc = h->d_pace_acc;
  a.ep_ret = h->d_ep_ret; a.ep_masks = h->ep_masks; a.ep_bad = h->ep_bad; a.ep_totals = h->ep_totals;   // (ep_rec / ep_serial: mocca_step only)
  a.hf = h->d_hf; a.hf_rows = h->hf_rows; a.hf_cols = h->hf_cols; a.hf_scale = h->hf_scale;
  if (h->hf_n_fields > 1) {   // (a bank of one is the shared grid: the kernels take the path they always took)
    a.hf_field = h->d_hf_field; a.hf_stride = h->hf_planes * h->hf_rows * h->hf_cols; a.hf_n_fields = h->hf_n_fields; a.hf_redraw = h->hf_redraw;
  }
  a.robot_state = h->d_ctrl_image ? h->d_robot_state.get() : nullptr;   // (base_value: mocca_plan_step only)
  return a;
}
// A scalar MOCCA_PARAM_APPLIED_GAIN is written into the task records (word MOCCA_TW_APPLIED_GAIN, what apply_action reads) by the NEXT call that takes
// a stream, on that stream: ordered against the caller's in-flight steps, which also write the word (store_task).
static int flush_pending(mocca_handle h, hipStream_t s) {
  if (!h->gain_pending) return MOCCA_OK;
  launch_per_env(set_task_word_kernel, h, s, h->d_task, MOCCA_TW_APPLIED_GAIN, nullptr, h->gain, 1, h->n_envs);
  HIP_TRY(h, hipGetLastError());
  h->gain_pending = false;
  return MOCCA_OK;
}
// the planner envs stand on the height field (`who`: the calling function and a colon, or nothing; `when`: the end of the sentence)
static int need_heightfield(mocca_handle h, const char* who, const char* when) {
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER || h->d_hf) return MOCCA_OK;
  h->err = std::string(who) + "the planner task needs mocca_set_heightfield " + when;
  return MOCCA_E_ARG;
}
// ... and this is what the ray caster and the height scan read of it; the other tasks have no grid
static mocca_rdr::HeightFieldBank heightfield_record(mocca_handle h) {
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return mocca_rdr::HeightFieldBank{nullptr, 0, 0, 0.0f, nullptr, nullptr, 0};
  return mocca_rdr::HeightFieldBank{h->d_hf, h->hf_rows, h->hf_cols, h->hf_scale, h->d_hf_range, h->hf_n_fields > 1 ? h->d_hf_field.get() : nullptr,
                                    (size_t)h->hf_planes * h->hf_rows * h->hf_cols};
}
// what reset / step / observe cannot run without: the mocap / phase envs read their targets, reset poses and reward references from the
// motion table, the planner envs their ground from the height field
static int need_attachments(mocca_handle h) {
  if (h->task_id == MOCCA_TASK_CASSIE && h->model.cassie_mode != MOCCA_CASSIE_PLAIN && !h->d_traj) {
    h->err = "this Cassie blob (cassie_mode != 0) needs mocca_set_trajectory before reset / step / observe";
    return MOCCA_E_ARG;
  }
  return need_heightfield(h, "", "before reset / step / observe");
}

int mocca_reset(mocca_handle h, const uint8_t* mask_dev, uint64_t seed, float* obs_dev, void* stream) {
  if (!h || !obs_dev) return MOCCA_E_ARG;
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  h->seed = seed;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.mask = mask_dev; a.obs = obs_dev;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_pending(h, s)) return rc;
  if (h->tape) {  // recorded draws instead of Philox (mocca_set_draw_tape)
    a.tape = h->tape; a.tape_n = h->tape_n;
    launch_taped_reset(h->topo, h->task_id, h->n_envs, s, a);
  } else {
    dispatch<LaunchReset>(h->topo, h->task_id, h->n_envs, s, a);
  }
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

// what the randomisation kernels key their draws by (mocca_randomise.h)
static mocca_rand::RandKeys rand_keys(mocca_handle h) {
  return mocca_rand::RandKeys{h->d_task, MOCCA_TASK_WORDS, MOCCA_TW_T, MOCCA_TW_EPISODE, h->env_offset, h->n_envs, (uint32_t)h->seed,
                              (uint32_t)(h->seed >> 32)};
}

// the step-kernel launch of mocca_step / mocca_plan_step (base_value: the controller's value estimates, or null); the handle's device is current
static int launch_step(mocca_handle h, const float* act_dev, const float* base_value, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                       int32_t* info_dev, hipStream_t s) {
  StepArgs a = make_args(h);
  a.act = act_dev; a.obs = obs_dev; a.rew = rew_dev; a.done = done_dev; a.info = info_dev;
  a.base_value = base_value;
  if (int rc = flush_pending(h, s)) return rc;
  if (h->rand_on) {   // strength, latency and pushes act on what the step kernel reads: one small launch in front of it, nothing without an attachment
    mocca_rand::PerturbArgs p{rand_keys(h), h->rand_cfg, act_dev, h->d_rand_eff, h->d_rand_ring, h->d_dyn, DYN_STRIDE, mocca_act_dim(h)};
    mocca_rand::launch_perturb(s, p);
    HIP_TRY(h, hipGetLastError());
    a.act = h->d_rand_eff;
  }
  // mocca_step never allocates and never synchronises, and the pace calibrates itself on the device: the launch can be captured in a
  // hipGraph.  Two optional features keep HOST state per launch that a capture bakes into the kernel arguments: the episode-record ring
  // (slot and serial below: a replayed launch keeps writing one slot under one serial -- read ep_masks / ep_totals instead) and the
  // re-sort schedule of MOCCA_PARAM_ORDER_EVERY > 0.
  if (h->d_ep_ret && h->ep_rec) {
    a.ep_rec = h->ep_rec + (size_t)(h->ep_serial % (uint32_t)h->ep_slots) * h->ep_stride;
    a.ep_serial = h->ep_serial;
    if (++h->ep_serial == 0u) h->ep_serial = 1u;
  }
  if (h->order_every > 0 && h->d_order) {   // heaviest envs first: the permutation is rebuilt on the caller's stream, ahead of the step that reads it
    if (h->order_age >= h->order_every) {
      hipLaunchKernelGGL(order_by_rows_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)h->d_task, h->d_order, h->n_envs);
      HIP_TRY(h, hipGetLastError());
      h->order_age = 0;
    }
    ++h->order_age;
    a.order = h->d_order;
  }
  switch (step_instance(h)) {
    case INST_COMPACT: mocca_r32_launch_step(h->topo, h->task_id, h->n_envs, s, &a); break;
    case INST_WIDE: mocca_r64_launch_step(h->topo, h->task_id, h->n_envs, s, &a); break;
    default: dispatch<LaunchStep>(h->topo, h->task_id, h->n_envs, s, a);
  }
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_step(mocca_handle h, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
               void* stream) {
  if (!h || !act_dev || !obs_dev || !rew_dev || !done_dev) return MOCCA_E_ARG;
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  return launch_step(h, act_dev, nullptr, obs_dev, rew_dev, done_dev, info_dev, (hipStream_t)stream);
}

int mocca_plan_step(mocca_handle h, const float* plan_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
                    void* stream) {
  if (!h || !plan_dev || !obs_dev || !rew_dev || !done_dev) return MOCCA_E_ARG;
  if (!h->d_ctrl_image) { h->err = "mocca_plan_step needs a base controller (mocca_set_base_controller)"; return MOCCA_E_ARG; }
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  mocca_ctrl::ControllerArgs c = h->ctrl;
  c.plan = plan_dev;
  mocca_ctrl::launch_controller(s, c);
  HIP_TRY(h, hipGetLastError());
  return launch_step(h, h->d_base_act, h->d_base_val, obs_dev, rew_dev, done_dev, info_dev, s);
}

// ---- domain randomisation (mocca_randomise.h) ----
int mocca_set_randomisation(mocca_handle h, const mocca_randomisation* cfg) {
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  if (!cfg) {   // detach: the next step reads the caller's actions again
    if (int rc = commit_ready(h, "mocca_set_randomisation")) return rc;
    h->rand_on = false; h->d_rand_eff.reset(); h->d_rand_ring.reset();
    return MOCCA_OK;
  }
  auto refuse = [&](const std::string& what) { h->err = "mocca_set_randomisation: " + what; return MOCCA_E_ARG; };
  const float lo = (float)cfg->strength_lo, hi = (float)cfg->strength_hi, pm = (float)cfg->push_max;
  if (!(lo > 0.0f) || !(hi <= 1.0f) || !(lo <= hi)) return refuse("the strength range must satisfy 0 < strength_lo <= strength_hi <= 1");
  if (h->task_id == MOCCA_TASK_CASSIE && (lo != 1.0f || hi != 1.0f))
    return refuse("MOCCA_TASK_CASSIE takes the strength range [1, 1] alone: its action is a PD target, not a torque");
  if (cfg->delay_min < 0 || cfg->delay_max < cfg->delay_min || cfg->delay_max > MOCCA_RAND_MAX_DELAY)
    return refuse("the delays must satisfy 0 <= delay_min <= delay_max <= " + std::to_string(MOCCA_RAND_MAX_DELAY));
  if (!std::isfinite(pm) || pm < 0.0f) return refuse("push_max must be finite and not negative");
  if (cfg->push_interval < 0 || cfg->push_interval > mocca_rand::RAND_MAX_INTERVAL)
    return refuse("push_interval must be 0 (no pushes) .. " + std::to_string(mocca_rand::RAND_MAX_INTERVAL));
  const int ad = mocca_act_dim(h);
  const size_t n_eff = (size_t)h->n_envs * ad, n_ring = n_eff * (cfg->delay_max + 1);
  if (n_eff >= ((size_t)1 << 31) || (long long)h->env_offset + h->n_envs > (1ll << 32) || h->env_offset < 0)
    return refuse("n_envs x act_dim must stay below 2^31 and the global env ids below 2^32");
  DevBuf<float> eff, ring;
  hipError_t e = eff.alloc(n_eff, true);
  if (e == hipSuccess) e = ring.alloc(n_ring, true);
  if (int rc = commit_ready(h, "mocca_set_randomisation", e)) return rc;
  h->d_rand_eff.swap(eff); h->d_rand_ring.swap(ring);
  const int planar = h->topo == TOPO_WALKER2D || h->topo == TOPO_CRAB2D || h->model.planar != 0;
  h->rand_cfg = mocca_rand::RandConfig{lo, hi, cfg->delay_min, cfg->delay_max, cfg->push_interval, pm, planar};
  h->rand_on = true;
  return MOCCA_OK;
}

int mocca_get_effective_action(mocca_handle h, float* out_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->rand_on) { h->err = "mocca_get_effective_action needs a randomisation (mocca_set_randomisation)"; return MOCCA_E_ARG; }
  if (!out_dev) { h->err = "mocca_get_effective_action: out_dev is NULL"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  HIP_TRY(h, hipMemcpyAsync(out_dev, h->d_rand_eff, (size_t)h->n_envs * mocca_act_dim(h) * sizeof(float), hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_sensor_noise(mocca_handle h, const float* scale_host, int dim) {
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  if (!scale_host) {
    if (int rc = commit_ready(h, "mocca_set_sensor_noise")) return rc;
    h->d_noise_scale.reset();
    return MOCCA_OK;
  }
  if (dim != h->obs_dim) { h->err = "mocca_set_sensor_noise: dim must be obs_dim (" + std::to_string(h->obs_dim) + ")"; return MOCCA_E_ARG; }
  for (int k = 0; k < dim; ++k)
    if (!std::isfinite(scale_host[k]) || scale_host[k] < 0.0f) {
      h->err = "mocca_set_sensor_noise: scale " + std::to_string(k) + " must be finite and not negative"; return MOCCA_E_ARG;
    }
  if ((size_t)h->n_envs * dim >= ((size_t)1 << 31)) { h->err = "mocca_set_sensor_noise: n_envs x dim must stay below 2^31"; return MOCCA_E_ARG; }
  DevBuf<float> sc;
  hipError_t e = sc.alloc(dim, false);
  if (e == hipSuccess) e = hipMemcpy(sc, scale_host, (size_t)dim * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(h, "mocca_set_sensor_noise", e)) return rc;
  h->d_noise_scale.swap(sc);
  return MOCCA_OK;
}

int mocca_sensor_noise(mocca_handle h, const float* rows_dev, int in_stride, float* out_dev, int out_stride, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->d_noise_scale) { h->err = "mocca_sensor_noise needs the scales (mocca_set_sensor_noise)"; return MOCCA_E_ARG; }
  if (!rows_dev || !out_dev) { h->err = "mocca_sensor_noise: rows_dev or out_dev is NULL"; return MOCCA_E_ARG; }
  if (in_stride < h->obs_dim || out_stride < h->obs_dim) {
    h->err = "mocca_sensor_noise: in_stride and out_stride must be at least obs_dim (" + std::to_string(h->obs_dim) + ")"; return MOCCA_E_ARG;
  }
  DeviceGuard guard(h->device);
  mocca_rand::NoiseArgs a{rand_keys(h), h->d_noise_scale, rows_dev, out_dev, in_stride, out_stride, h->obs_dim};
  mocca_rand::launch_noise((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_randomisation_record(mocca_handle h, float* out_dev, int row_stride, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->rand_on) { h->err = "mocca_randomisation_record needs a randomisation (mocca_set_randomisation)"; return MOCCA_E_ARG; }
  if (!out_dev) { h->err = "mocca_randomisation_record: out_dev is NULL"; return MOCCA_E_ARG; }
  if (row_stride < MOCCA_RAND_WORDS) {
    h->err = "mocca_randomisation_record: row_stride must be at least MOCCA_RAND_WORDS (" + std::to_string(MOCCA_RAND_WORDS) + ")"; return MOCCA_E_ARG;
  }
  DeviceGuard guard(h->device);
  mocca_rand::RecordArgs a{rand_keys(h), h->rand_cfg, out_dev, row_stride};
  mocca_rand::launch_record((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

// ---- the observation-action history (mocca_history.h) ----
int mocca_set_history(mocca_handle h, const int32_t* cols_host, int n_cols, int act_dim, int steps, int stride) {
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  if (steps == 0) {   // detach
    if (int rc = commit_ready(h, "mocca_set_history")) return rc;
    h->hist_cfg = mocca_hist::HistConfig{}; h->d_hist_cols.reset(); h->d_hist_ring.reset(); h->d_hist_tags.reset();
    return MOCCA_OK;
  }
  auto refuse = [&](const std::string& what) { h->err = "mocca_set_history: " + what; return MOCCA_E_ARG; };
  if (steps < 1 || steps > MOCCA_HIST_MAX_STEPS) return refuse("steps must be 1 .. " + std::to_string(MOCCA_HIST_MAX_STEPS) + " (0 detaches)");
  if (stride < 1 || stride > MOCCA_HIST_MAX_STRIDE) return refuse("stride must be 1 .. " + std::to_string(MOCCA_HIST_MAX_STRIDE));
  if (act_dim < 0 || act_dim > mocca_hist::HIST_MAX_ACT) return refuse("act_dim must be 0 .. " + std::to_string(mocca_hist::HIST_MAX_ACT));
  if (n_cols < 0 || n_cols > h->obs_dim || (n_cols > 0 && !cols_host))
    return refuse("n_cols must be 0 .. obs_dim (" + std::to_string(h->obs_dim) + "), with that many columns");
  if (n_cols + act_dim == 0) return refuse("a frame needs at least one observation column or one action entry");
  std::vector<char> seen((size_t)h->obs_dim, 0);
  for (int k = 0; k < n_cols; ++k) {
    const int c = cols_host[k];
    if (c < 0 || c >= h->obs_dim) return refuse("column " + std::to_string(c) + " is outside 0 .. " + std::to_string(h->obs_dim - 1));
    if (seen[c]) return refuse("column " + std::to_string(c) + " is repeated");
    seen[c] = 1;
  }
  const mocca_hist::HistConfig cfg{steps, stride, n_cols, act_dim};
  if (mocca_hist::hist_dim(cfg) > MOCCA_HIST_MAX_DIM)
    return refuse("the block has steps x (n_cols + act_dim) = " + std::to_string(mocca_hist::hist_dim(cfg)) + " floats, at most " +
                  std::to_string(MOCCA_HIST_MAX_DIM));
  const size_t n_slots = (size_t)h->n_envs * mocca_hist::hist_slots(cfg);
  if ((size_t)h->n_envs * mocca_hist::hist_dim(cfg) >= ((size_t)1 << 31)) return refuse("n_envs x the block width must stay below 2^31");
  DevBuf<int32_t> cols;
  DevBuf<float> ring;
  DevBuf<uint32_t> tags;
  hipError_t e = cols.alloc((size_t)(n_cols > 0 ? n_cols : 1), true);
  if (e == hipSuccess && n_cols > 0) e = hipMemcpy(cols, cols_host, (size_t)n_cols * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ring.alloc(n_slots * mocca_hist::hist_width(cfg), true);
  if (e == hipSuccess) e = tags.alloc(n_slots * 2, false);
  if (e == hipSuccess) e = hipMemset(tags, 0xFF, n_slots * 2 * sizeof(uint32_t));   // every tag word HIST_NO_T: a frame no episode holds
  if (int rc = commit_ready(h, "mocca_set_history", e)) return rc;
  h->d_hist_cols.swap(cols); h->d_hist_ring.swap(ring); h->d_hist_tags.swap(tags);
  h->hist_cfg = cfg;
  return MOCCA_OK;
}

int mocca_history_dim(mocca_handle h) {
  if (!h) return MOCCA_E_ARG;
  if (h->hist_cfg.steps == 0) { h->err = "mocca_history_dim needs a history (mocca_set_history)"; return MOCCA_E_ARG; }
  return mocca_hist::hist_dim(h->hist_cfg);
}

int mocca_history(mocca_handle h, const float* rows_dev, int row_stride, const float* act_dev, int act_stride, float* out_dev, int out_stride,
                  void* stream) {
  if (!h) return MOCCA_E_ARG;
  const mocca_hist::HistConfig& cfg = h->hist_cfg;
  if (cfg.steps == 0) { h->err = "mocca_history needs a history (mocca_set_history)"; return MOCCA_E_ARG; }
  if (!rows_dev || !out_dev) { h->err = "mocca_history: rows_dev or out_dev is NULL"; return MOCCA_E_ARG; }
  if (row_stride < h->obs_dim) { h->err = "mocca_history: row_stride must be at least obs_dim (" + std::to_string(h->obs_dim) + ")"; return MOCCA_E_ARG; }
  if (out_stride < mocca_hist::hist_dim(cfg)) {
    h->err = "mocca_history: out_stride must be at least the block width (" + std::to_string(mocca_hist::hist_dim(cfg)) + ")"; return MOCCA_E_ARG;
  }
  if (act_dev && act_stride < cfg.act_dim) {
    h->err = "mocca_history: act_stride must be at least the history's act_dim (" + std::to_string(cfg.act_dim) + ")"; return MOCCA_E_ARG;
  }
  DeviceGuard guard(h->device);
  mocca_hist::HistArgs a{cfg, h->d_task, MOCCA_TASK_WORDS, MOCCA_TW_T, MOCCA_TW_EPISODE, h->n_envs, h->d_hist_cols, h->d_hist_ring, h->d_hist_tags,
                         rows_dev, act_dev, out_dev, row_stride, act_stride, out_stride};
  mocca_hist::launch_history((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_get_base_outputs(mocca_handle h, float* action_dev, float* value_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->d_ctrl_image) { h->err = "mocca_get_base_outputs needs a base controller (mocca_set_base_controller)"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  if (action_dev) HIP_TRY(h, hipMemcpyAsync(action_dev, h->d_base_act, (size_t)h->n_envs * mocca_ctrl::CTRL_ACTION * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (value_dev) HIP_TRY(h, hipMemcpyAsync(value_dev, h->d_base_val, (size_t)h->n_envs * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_base_controller(mocca_handle h, const float* params_host, size_t n_floats, const int32_t* layers_host, int n_layers_total,
                              double action_scale) try {
  using namespace mocca_ctrl;
  if (!h) return MOCCA_E_ARG;
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) { h->err = "mocca_set_base_controller: only the planner task (Walker3DPlannerEnv, MikePlannerEnv) has a base controller"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  if (!params_host) {   // detach
    if (int rc = commit_ready(h, "mocca_set_base_controller")) return rc;
    h->d_ctrl_image.reset(); h->d_ctrl_layers.reset(); h->d_ctrl_norm.reset(); h->ctrl = {};
    return MOCCA_OK;
  }
  auto bad = [&](const std::string& what) { h->err = "mocca_set_base_controller: " + what; return MOCCA_E_ARG; };
  if (n_floats == 0 || n_floats > ((size_t)1 << 28)) return bad("the parameter array is empty or larger than any valid controller");
  if (!std::isfinite(action_scale)) return bad("action_scale is not finite");
  int count[2];
  const std::string wrong = check_layer_table(layers_host, n_layers_total, CTRL_IN, CTRL_ACTION, n_floats, "a net's first layer takes the 65-float input",
                                              "the actor ends in 21 outputs, the critic in 1", count);
  if (!wrong.empty()) return bad(wrong);
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
  if (e == hipSuccess && !h->d_robot_state) e = state.alloc(n * ROBOT_STATE_STRIDE, true);
  if (e == hipSuccess && !h->d_base_act) e = act.alloc(n * CTRL_ACTION, true);
  if (e == hipSuccess && !h->d_base_val) e = val.alloc(n, true);
  if (e != hipSuccess) (void)hipDeviceSynchronize();
  if (int rc = commit_ready(h, "mocca_set_base_controller", e)) return rc;
  h->d_ctrl_image.swap(im.image); h->d_ctrl_layers.swap(im.layers);
  if (state) h->d_robot_state.swap(state);
  if (act) h->d_base_act.swap(act);
  if (val) h->d_base_val.swap(val);
  mocca_ctrl::ControllerArgs& c = h->ctrl;
  c.params = im.pa.params; c.layers = im.pa.layers; c.n_actor = count[0]; c.n_critic = count[1];
  c.robot_state = h->d_robot_state; c.action_scale = (float)action_scale;
  c.action = h->d_base_act; c.value = h->d_base_val; c.n_envs = h->n_envs;
  h->d_ctrl_norm.reset();   // the statistics belonged to the controller that was replaced
  c.norm_mean = c.norm_inv_std = nullptr; c.norm_clip = 0.0f;
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_set_base_controller"); }

int mocca_set_base_controller_norm(mocca_handle h, const float* mean_host, const float* inv_std_host, double clip) {
  using namespace mocca_ctrl;
  if (!h) { g_err = "mocca_set_base_controller_norm: NULL handle"; return MOCCA_E_ARG; }
  auto bad = [&](const std::string& what) { h->err = "mocca_set_base_controller_norm: " + what; return MOCCA_E_ARG; };
  if (!h->d_ctrl_image) return bad("needs a base controller (mocca_set_base_controller)");
  if (!mean_host != !inv_std_host) return bad("mean_host and inv_std_host must both be given, or both be NULL (detach)");
  DeviceGuard guard(h->device);
  if (!mean_host) {   // detach
    if (int rc = commit_ready(h, "mocca_set_base_controller_norm")) return rc;
    h->d_ctrl_norm.reset();
    h->ctrl.norm_mean = h->ctrl.norm_inv_std = nullptr; h->ctrl.norm_clip = 0.0f;
    return MOCCA_OK;
  }
  for (int k = 0; k < CTRL_IN; ++k) {
    if (!std::isfinite(mean_host[k])) return bad("mean[" + std::to_string(k) + "] is not finite");
    if (!std::isfinite(inv_std_host[k]) || inv_std_host[k] < 0.0f) return bad("inv_std[" + std::to_string(k) + "] is not finite or is negative");
  }
  if (!std::isfinite(clip) || !(clip > 0.0)) return bad("clip must be finite and positive");
  float host[2 * CTRL_IN];
  std::memcpy(host, mean_host, CTRL_IN * sizeof(float));
  std::memcpy(host + CTRL_IN, inv_std_host, CTRL_IN * sizeof(float));
  DevBuf<float> norm;
  hipError_t e = norm.alloc(2 * CTRL_IN, false);
  if (e == hipSuccess) e = hipMemcpy(norm, host, sizeof(host), hipMemcpyHostToDevice);
  if (int rc = commit_ready(h, "mocca_set_base_controller_norm", e)) return rc;
  h->d_ctrl_norm.swap(norm);
  h->ctrl.norm_mean = h->d_ctrl_norm; h->ctrl.norm_inv_std = h->d_ctrl_norm.get() + CTRL_IN; h->ctrl.norm_clip = (float)clip;
  return MOCCA_OK;
}

int mocca_task_step(mocca_handle h, const float* act_dev, const int32_t* touch_dev, const int32_t* target_dev, const int32_t* body_dev,
                    float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  if (!h || !act_dev || !obs_dev || !rew_dev || !done_dev) return MOCCA_E_ARG;
  if (!touch_dev && h->task_id != MOCCA_TASK_CASSIE) { h->err = "mocca_task_step needs the foot contact flags"; return MOCCA_E_ARG; }
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.act = act_dev; a.obs = obs_dev; a.rew = rew_dev; a.done = done_dev; a.info = info_dev;
  a.inj_touch = touch_dev; a.inj_target = target_dev; a.inj_body = body_dev;
  a.tape = h->tape; a.tape_n = h->tape_n;
  a.dbg = nullptr;
  if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
  launch_task_step(h->topo, h->task_id, h->n_envs, (hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_set_draw_tape(mocca_handle h, const float* tape_dev, int n_per_env) {
  if (!h || (tape_dev && n_per_env <= 0)) return MOCCA_E_ARG;
  h->tape = tape_dev; h->tape_n = tape_dev ? n_per_env : 0;
  return MOCCA_OK;
}

int mocca_set_debug_buffer(mocca_handle h, int32_t* dbg_dev) {
  if (!h) return MOCCA_E_ARG;
  h->dbg = dbg_dev;
  return MOCCA_OK;
}

int mocca_set_terminal_obs_buffer(mocca_handle h, float* final_obs_dev) {
  if (!h) return MOCCA_E_ARG;
  h->final_obs = final_obs_dev;
  return MOCCA_OK;
}

int mocca_set_episode_stats(mocca_handle h, float* masks_dev, float* bad_masks_dev, float* totals_dev, void* records, int n_slots,
                            size_t slot_stride_bytes) {
  if (!h) return MOCCA_E_ARG;
  const bool on = masks_dev || bad_masks_dev || totals_dev || records;
  if (records && (n_slots < 1 || slot_stride_bytes < (size_t)h->n_envs * sizeof(mocca_episode_rec) || ((uintptr_t)records & 15u) || (slot_stride_bytes & 15u))) {
    h->err = "episode records: n_slots >= 1 slots of n_envs 16-byte records, 16-byte aligned, slot_stride_bytes >= 16 n_envs"; return MOCCA_E_ARG;
  }
  DeviceGuard guard(h->device);
  if (on && !h->d_ep_ret) {
    HIP_TRY(h, h->d_ep_ret.alloc((size_t)h->n_envs, true));
  } else if (!on && h->d_ep_ret) {
    HIP_TRY(h, hipDeviceSynchronize());   // a launch in flight may still add to it
    h->d_ep_ret.reset();
  }
  h->ep_masks = masks_dev; h->ep_bad = bad_masks_dev; h->ep_totals = totals_dev;
  h->ep_rec = (char*)records; h->ep_slots = records ? n_slots : 0; h->ep_stride = records ? slot_stride_bytes : 0;
  return MOCCA_OK;
}
uint32_t mocca_episode_serial(mocca_handle h) { return h ? h->ep_serial : 0u; }

int mocca_set_seed(mocca_handle h, uint64_t seed) {
  if (!h) return MOCCA_E_ARG;
  h->seed = seed;
  return MOCCA_OK;
}

int mocca_is_diagnostic_build(void) {
#if defined(MOCCA_SKIP_COLLIDE) || defined(MOCCA_SKIP_ABA) || defined(MOCCA_SKIP_SOLVE) || defined(MOCCA_DUMMY_VALU) || defined(MOCCA_STAMPS) || \
    defined(MOCCA_NO_TWO_PATHS) || defined(MOCCA_ABL_PAIRLOAD) || defined(MOCCA_ABL_NOPASS2) || defined(MOCCA_ABL_NOHITS) || MOCCA_LDS_PAD > 0
  return 1;
#else
  return 0;
#endif
}

int mocca_set_trajectory(mocca_handle h, const float* table_host, int n_frames, double max_time, double control_step) {
  if (!h) return MOCCA_E_ARG;
  if (!table_host || n_frames <= 0 || !(max_time > 0.0) || !(control_step > 0.0)) { h->err = "mocca_set_trajectory: empty table or non-positive times"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  const size_t floats = (size_t)n_frames * MOCCA_TRAJ_STRIDE;
  DevBuf<float> traj;
  hipError_t e = traj.alloc(floats, false);
  if (e == hipSuccess) e = hipMemcpy(traj, table_host, floats * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(h, "mocca_set_trajectory", e)) return rc;
  h->d_traj.swap(traj);
  h->traj_n = n_frames; h->traj_tmax = max_time; h->traj_cstep = control_step;
  return MOCCA_OK;
}

// Attach a terrain bank (mocca_set_heightfield: a bank of one; `who`: the entry point's name).  heights_host == nullptr: a bank of zeros.
static int attach_bank(mocca_handle h, const std::string& who, const float* heights_host, int n_fields, int rows, int cols, double scale) {
  if (rows < 2 || cols < 2 || !(scale > 0.0)) { h->err = who + ": needs at least 2 x 2 heights and a positive scale"; return MOCCA_E_ARG; }
  // Search window of every terrain contact slot: a sphere of reach rho = radius + margin around a centre that is at most half a cell from
  // its nearest grid point touches only cells within W = ceil(rho scale + 1/2) of that point (1e-6: a reach of exactly half a cell is W = 1).
  // W - 1 travels in bits 30..31 of the slot record; a grid so fine that a sphere spans more than 4 cells each way is refused.
  int wmax = 1;
  uint32_t wbits[MOCCA_MAX_SLOTS];
  for (int sl = 0; sl < h->model.n_slots; ++sl) {
    uint32_t ids; std::memcpy(&ids, &h->model.slot_tab[sl][2], 4);
    const double reach = (double)h->model.slot_tab[sl][0] + (double)((ids >> 17) & 0xFFu) / 8192.0;
    int w = (int)std::ceil(reach * scale + 0.5 - 1e-6);
    if (w < 1) w = 1;
    if (w > 4 && ((ids >> 25) & 1u)) { h->err = who + ": the grid is too fine for this robot (a contact sphere would span more than 4 cells each way)"; return MOCCA_E_ARG; }
    if (w > 4) w = 4;
    wbits[sl] = (ids & 0x3FFFFFFFu) | ((uint32_t)(w - 1) << 30);
    if (((ids >> 25) & 1u) && w > wmax) wmax = w;
  }
  const size_t cells = (size_t)rows * cols, stride = cells * wmax;
  if (stride > ((size_t)1 << 26) || stride * n_fields > ((size_t)1 << 30)) { h->err = who + ": the bank is larger than 2^30 heights (pooled copies included)"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  // every field: the heights, followed by one max-pooled copy per window 2 .. wmax (copy k: the highest point within k + 1 cells of each grid
  // point): what a wide sphere's search is pruned by with one load.  Beside the bank, each field's range.
  std::vector<float> host, range((size_t)n_fields * 2, 0.0f);
  if (heights_host) {
    host.resize(stride * n_fields);
    for (int f = 0; f < n_fields; ++f) {
      const float* in = heights_host + cells * f;
      float* field = host.data() + stride * f;
      std::memcpy(field, in, cells * sizeof(float));
      for (int w = 2; w <= wmax; ++w) {
        float* out = field + cells * (w - 1);
        for (int j = 0; j < rows; ++j)
          for (int i = 0; i < cols; ++i) {
            float m = -1e30f;
            for (int jj = (j - w < 0 ? 0 : j - w); jj <= (j + w > rows - 1 ? rows - 1 : j + w); ++jj)
              for (int ii = (i - w < 0 ? 0 : i - w); ii <= (i + w > cols - 1 ? cols - 1 : i + w); ++ii)
                m = in[(size_t)jj * cols + ii] > m ? in[(size_t)jj * cols + ii] : m;
            out[(size_t)j * cols + i] = m;
          }
      }
      float zmin = in[0], zmax = in[0];
      for (size_t k = 1; k < cells; ++k) {
        zmin = in[k] < zmin ? in[k] : zmin;
        zmax = in[k] > zmax ? in[k] : zmax;
      }
      range[2 * (size_t)f] = zmin; range[2 * (size_t)f + 1] = zmax;
    }
  }
  // the window bits go into a COPY of the model; the handle's host image takes them only once the device has them
  auto next = std::make_unique<MoccaModel>(h->model);
  for (int sl = 0; sl < next->n_slots; ++sl) std::memcpy(&next->slot_tab[sl][2], &wbits[sl], 4);
  DevBuf<float> hf, rng, part;
  DevBuf<int32_t> field;
  hipError_t e = hf.alloc(stride * n_fields, !heights_host);
  if (e == hipSuccess && heights_host) e = hipMemcpy(hf, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = rng.alloc(range.size(), false);
  if (e == hipSuccess) e = hipMemcpy(rng, range.data(), range.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = part.alloc((size_t)n_fields * mocca_terrain::terrain_blocks(rows, cols) * 2, true);
  if (e == hipSuccess) e = field.alloc((size_t)h->n_envs, true);
  if (int rc = commit_ready(h, who.c_str(), e)) return rc;   // no launch in flight still reads the old bank or the old slot records
  // the device model is rewritten in place: the last step that can fail, and one that fails leaves host and device records as they were
  if ((e = hipMemcpy(h->d_model, next.get(), sizeof(MoccaModel), hipMemcpyHostToDevice)) != hipSuccess) {
    h->err = std::string("hipMemcpy(model): ") + hipGetErrorString(e); return MOCCA_E_HIP;
  }
  h->model = *next;
  h->d_hf.swap(hf); h->d_hf_range.swap(rng); h->d_hf_part.swap(part); h->d_hf_field.swap(field);
  h->hf_rows = rows; h->hf_cols = cols; h->hf_scale = (float)scale;
  h->hf_n_fields = n_fields; h->hf_planes = wmax; h->hf_redraw = 0;
  return MOCCA_OK;
}

int mocca_set_heightfield(mocca_handle h, const float* heights_host, int rows, int cols, double scale) try {
  if (!h) return MOCCA_E_ARG;
  if (!heights_host) { h->err = "mocca_set_heightfield: needs at least 2 x 2 heights and a positive scale"; return MOCCA_E_ARG; }
  return attach_bank(h, "mocca_set_heightfield", heights_host, 1, rows, cols, scale);
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_set_heightfield"); }

int mocca_set_heightfield_bank(mocca_handle h, const float* heights_host, int n_fields, int rows, int cols, double scale) try {
  if (!h) return MOCCA_E_ARG;
  const std::string who = "mocca_set_heightfield_bank";
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) { h->err = who + ": only the planner task (Walker3DPlannerEnv, MikePlannerEnv) stands on height fields"; return MOCCA_E_ARG; }
  if (!heights_host && n_fields == 0) {   // detach
    DeviceGuard guard(h->device);
    if (int rc = commit_ready(h, who.c_str())) return rc;
    h->d_hf.reset(); h->d_hf_range.reset(); h->d_hf_part.reset(); h->d_hf_field.reset();
    h->hf_rows = h->hf_cols = h->hf_n_fields = h->hf_redraw = 0; h->hf_planes = 1; h->hf_scale = 0.0f;
    return MOCCA_OK;
  }
  if (n_fields < 1 || n_fields > MOCCA_HF_MAX_FIELDS) { h->err = who + ": n_fields must be 1 .. " + std::to_string(MOCCA_HF_MAX_FIELDS); return MOCCA_E_ARG; }
  return attach_bank(h, who, heights_host, n_fields, rows, cols, scale);
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_set_heightfield_bank"); }

// what the bank calls below share: a planner handle with a bank, and fields first .. first + count - 1 inside it
static int need_bank(mocca_handle h, const std::string& who, int first, int count) {
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER || !h->d_hf) { h->err = who + ": no terrain bank (mocca_set_heightfield_bank)"; return MOCCA_E_ARG; }
  if (first < 0 || count < 1 || first > h->hf_n_fields - count) {
    h->err = who + ": fields " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) + " are not inside the bank of " + std::to_string(h->hf_n_fields);
    return MOCCA_E_ARG;
  }
  return MOCCA_OK;
}

int mocca_generate_heightfields(mocca_handle h, int first, int count, uint64_t seed, int n_peaks, double gain, void* stream) try {
  if (!h) return MOCCA_E_ARG;
  const std::string who = "mocca_generate_heightfields";
  if (int rc = need_bank(h, who, first, count)) return rc;
  if ((h->hf_rows & 7) || (h->hf_cols & 7)) { h->err = who + ": rows and cols must be multiples of 8 (the noise lattices of 4 and 8 cells divide them)"; return MOCCA_E_ARG; }
  if (n_peaks < 1 || n_peaks > MOCCA_HF_MAX_PEAKS) { h->err = who + ": n_peaks must be 1 .. " + std::to_string(MOCCA_HF_MAX_PEAKS); return MOCCA_E_ARG; }
  if (!std::isfinite(gain) || !(gain > 0.0)) { h->err = who + ": gain must be finite and > 0"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  mocca_terrain::TerrainArgs a{};
  a.bank = h->d_hf; a.range = h->d_hf_range; a.part = h->d_hf_part;
  a.rows = h->hf_rows; a.cols = h->hf_cols; a.planes = h->hf_planes; a.stride = (size_t)h->hf_planes * h->hf_rows * h->hf_cols;
  a.scale = h->hf_scale; a.gain = (float)gain;
  a.first = first; a.count = count; a.n_peaks = n_peaks;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  mocca_terrain::launch_generate((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_generate_heightfields"); }

int mocca_set_env_fields(mocca_handle h, const int32_t* field_dev, int redraw_at_reset, void* stream) try {
  if (!h) return MOCCA_E_ARG;
  const std::string who = "mocca_set_env_fields";
  if (int rc = need_bank(h, who, 0, 1)) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)h->n_envs * sizeof(int32_t);
  if (field_dev) {
    std::vector<int32_t> ids((size_t)h->n_envs);
    HIP_TRY(h, hipMemcpyAsync(ids.data(), field_dev, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int e = 0; e < h->n_envs; ++e)
      if (ids[e] < 0 || ids[e] >= h->hf_n_fields) {
        h->err = who + ": field " + std::to_string(ids[e]) + " (env " + std::to_string(e) + ") is outside 0 .. " + std::to_string(h->hf_n_fields - 1);
        return MOCCA_E_ARG;
      }
    HIP_TRY(h, hipMemcpyAsync(h->d_hf_field, field_dev, bytes, hipMemcpyDeviceToDevice, s));
  } else {
    HIP_TRY(h, hipMemsetAsync(h->d_hf_field, 0, bytes, s));
  }
  h->hf_redraw = redraw_at_reset != 0;
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_set_env_fields"); }

int mocca_get_env_fields(mocca_handle h, int32_t* field_dev, void* stream) try {
  if (!h) return MOCCA_E_ARG;
  if (!field_dev) { h->err = "mocca_get_env_fields: field_dev must not be NULL"; return MOCCA_E_ARG; }
  if (int rc = need_bank(h, "mocca_get_env_fields", 0, 1)) return rc;
  DeviceGuard guard(h->device);
  HIP_TRY(h, hipMemcpyAsync(field_dev, h->d_hf_field, (size_t)h->n_envs * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_get_env_fields"); }

int mocca_get_heightfields(mocca_handle h, int first, int count, float* out_dev, void* stream) try {
  if (!h) return MOCCA_E_ARG;
  if (!out_dev) { h->err = "mocca_get_heightfields: out_dev must not be NULL"; return MOCCA_E_ARG; }
  if (int rc = need_bank(h, "mocca_get_heightfields", first, count)) return rc;
  DeviceGuard guard(h->device);
  const size_t cells = (size_t)h->hf_rows * h->hf_cols, w = cells * sizeof(float);   // the heights of each field, without its pooled copies
  const float* src = h->d_hf.get() + cells * h->hf_planes * first;
  if (h->hf_planes == 1) HIP_TRY(h, hipMemcpyAsync(out_dev, src, w * count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  else
    for (int f = 0; f < count; ++f)
      HIP_TRY(h, hipMemcpyAsync(out_dev + cells * f, src + cells * h->hf_planes * f, w, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_get_heightfields"); }

int mocca_observe(mocca_handle h, float* obs_dev, void* stream) {
  if (!h || !obs_dev) return MOCCA_E_ARG;
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.obs = obs_dev;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_pending(h, s)) return rc;
  dispatch<LaunchObserve>(h->topo, h->task_id, h->n_envs, s, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_get_state(mocca_handle h, float* state_dev, void* stream) {
  if (!h || !state_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  const size_t w = (size_t)mocca_state_dim(h) * sizeof(float);
  HIP_TRY(h, hipMemcpy2DAsync(state_dev, w, h->d_dyn, DYN_STRIDE * sizeof(float), w, h->n_envs, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_state(mocca_handle h, const float* state_dev, void* stream) {
  if (!h || !state_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  const size_t w = (size_t)mocca_state_dim(h) * sizeof(float);
  HIP_TRY(h, hipMemcpy2DAsync(h->d_dyn, DYN_STRIDE * sizeof(float), state_dev, w, w, h->n_envs, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_get_task(mocca_handle h, uint32_t* task_dev, void* stream) {
  if (!h || !task_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
  HIP_TRY(h, hipMemcpyAsync(task_dev, h->d_task, (size_t)h->n_envs * MOCCA_TASK_WORDS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_task(mocca_handle h, const uint32_t* task_dev, void* stream) {
  if (!h || !task_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  // a restored snapshot wins over an earlier scalar applied_gain: every env's MOCCA_TW_APPLIED_GAIN is the snapshot's; the handle's own copy (what a
  // Custom env's reset writes, robot.applied_gain persists across resets) keeps the value of the last mocca_set_param
  h->gain_pending = false;
  HIP_TRY(h, hipMemcpyAsync(h->d_task, task_dev, (size_t)h->n_envs * MOCCA_TASK_WORDS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_get_terrain(mocca_handle h, float* terrain_dev, void* stream) {
  if (!h || !terrain_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  HIP_TRY(h, hipMemcpyAsync(terrain_dev, h->d_terrain, (size_t)h->n_envs * TERRAIN_STRIDE * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_terrain(mocca_handle h, const float* terrain_dev, void* stream) {
  if (!h || !terrain_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  HIP_TRY(h, hipMemcpyAsync(h->d_terrain, terrain_dev, (size_t)h->n_envs * TERRAIN_STRIDE * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_param(mocca_handle h, int param_id, double value) {
  if (!h) return MOCCA_E_ARG;
  switch (param_id) {
    case MOCCA_PARAM_AUTO_RESET: h->auto_reset = value != 0; break;
    case MOCCA_PARAM_EVAL_MODE: h->eval_mode = value != 0; h->pvec_on[1] = false; break;
    case MOCCA_PARAM_CURRICULUM: h->curriculum = (int)value < 0 ? 0 : ((int)value > 9 ? 9 : (int)value); h->pvec_on[0] = false; break;
    case MOCCA_PARAM_APPLIED_GAIN:  // acts on the next apply_action: the task records carry the value the kernel uses; this call has no
      h->gain = (float)value; h->pvec_on[2] = false; h->gain_pending = true;   // stream, so the write is enqueued by the next call that has
      break;                                                                    // one (flush_pending), ordered on the caller's stream
    case MOCCA_PARAM_RANDOM_POSE: h->random_pose = value != 0; break;
    case MOCCA_PARAM_HOST_RETARGET: h->host_retarget = value != 0; break;
    case MOCCA_PARAM_SEED: h->seed = (uint64_t)value; break;
    case MOCCA_PARAM_ENV_OFFSET: h->env_offset = (int)value; break;
    case MOCCA_PARAM_ISSUE_PRIORITY:
      if (value < 0 || value >= 262144) { h->err = "MOCCA_PARAM_ISSUE_PRIORITY is t1 + 64 t2 + 4096 t3 with each threshold in 0..63"; return MOCCA_E_ARG; }
      h->prio = (int)value;
      break;
    case MOCCA_PARAM_RANDOM_REWARD:
      if (value != 0 && value != 1 && value != 2) { h->err = "MOCCA_PARAM_RANDOM_REWARD is 0, 1 or 2"; return MOCCA_E_ARG; }
      h->random_reward = (int)value; break;
    case MOCCA_PARAM_PERSIST_IMPULSES: h->persist_warm = value != 0; break;
    case MOCCA_PARAM_PACE_TICKS:
      if (value < -64 || value > 1e9) { h->err = "MOCCA_PARAM_PACE_TICKS is a tick count > 0, 0 (off) or -k (self-calibrating, k / 16 of the mean wave time, k <= 64)"; return MOCCA_E_ARG; }
      h->pace = (int)value; break;
    case MOCCA_PARAM_ORDER_EVERY:
      if (value < 0 || value > 1e6) { h->err = "MOCCA_PARAM_ORDER_EVERY is a step count >= 0"; return MOCCA_E_ARG; }
      h->order_every = (int)value; h->order_age = h->order_every;
      if (h->order_every > 0 && !h->d_order) {   // (allocated here, not in mocca_step)
        DeviceGuard guard(h->device);
        HIP_TRY(h, h->d_order.alloc((size_t)h->n_envs, false));
      }
      break;
    case MOCCA_PARAM_KERNEL_VARIANT: {
      if (value != (double)(int)value || value < 0 || value > 7 || ((int)value & 3) == 3) { h->err = "MOCCA_PARAM_KERNEL_VARIANT is 0 (automatic), 1 (force the 48-row instance) or 2 (force the 64-row instance), plus 4 to build the Delassus matrix on the VALU"; return MOCCA_E_ARG; }
      const int inst = (int)value & 3;
      if (inst == 1 && h->wide) { h->err = "MOCCA_PARAM_KERNEL_VARIANT = 1: this blob needs the 64-row instance (caps beyond 48 rows / 12 contacts, or sweep_alternate)"; return MOCCA_E_ARG; }
      h->force_full = inst; h->delassus_valu = ((int)value & 4) != 0; break;
    }
    default: h->err = "unknown parameter id"; return MOCCA_E_ARG;
  }
  return MOCCA_OK;
}

int mocca_set_param_v(mocca_handle h, int param_id, const float* values_dev, int broadcast, void* stream) {
  if (!h || !values_dev) return MOCCA_E_ARG;
  const int slot = param_id == MOCCA_PARAM_CURRICULUM ? 0 : param_id == MOCCA_PARAM_EVAL_MODE ? 1 : param_id == MOCCA_PARAM_APPLIED_GAIN ? 2 : -1;
  if (slot < 0) { h->err = "this parameter has no per-env form"; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  if (!h->d_pvec[slot]) HIP_TRY(h, h->d_pvec[slot].alloc((size_t)h->n_envs, false));
  hipStream_t s = (hipStream_t)stream;
  launch_per_env(copy_param_kernel, h, s, h->d_pvec[slot], values_dev, broadcast != 0, h->n_envs);
  HIP_TRY(h, hipGetLastError());
  if (slot == 2) {  // applied_gain acts at once (robots.py:33)
    // the per-env values supersede a scalar mocca_set_param(APPLIED_GAIN) that was not flushed yet: left pending, the next call with a
    // stream would overwrite every env's word with the stale scalar (call order must win, as it did when the scalar write was synchronous)
    h->gain_pending = false;
    launch_per_env(set_task_word_kernel, h, s, h->d_task, MOCCA_TW_APPLIED_GAIN, h->d_pvec[slot], 0.0f, 0, h->n_envs);
    HIP_TRY(h, hipGetLastError());
  }
  h->pvec_on[slot] = true;
  return MOCCA_OK;
}

static mocca_rdr::SceneArgs scene_args(mocca_handle h) {
  mocca_rdr::SceneArgs a{};
  a.model = h->d_model; a.dyn = h->d_dyn; a.task = h->d_task; a.terrain = h->d_terrain;
  a.dyn_stride = DYN_STRIDE; a.terrain_stride = TERRAIN_STRIDE; a.task_id = h->task_id;
  return a;
}

int mocca_get_link_frames(mocca_handle h, float* frames_dev, void* stream) {
  if (!h || !frames_dev) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  mocca_rdr::launch_link_frames((hipStream_t)stream, scene_args(h), h->n_envs, frames_dev);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_render(mocca_handle h, const int32_t* env_ids_dev, int n_views, const float* cameras_dev, int width, int height, uint8_t* rgb_dev,
                 float* depth_dev, int32_t* id_dev, void* stream) try {
  if (!h) return MOCCA_E_ARG;
  if (!env_ids_dev || !cameras_dev) { h->err = "mocca_render: env_ids_dev and cameras_dev must not be NULL"; return MOCCA_E_ARG; }
  if (n_views < 1 || n_views > 65535) { h->err = "mocca_render: n_views must be 1 .. 65535"; return MOCCA_E_ARG; }
  if (width < 1 || height < 1 || width > MOCCA_RENDER_MAX_SIZE || height > MOCCA_RENDER_MAX_SIZE) {
    h->err = "mocca_render: width and height must be 1 .. " + std::to_string(MOCCA_RENDER_MAX_SIZE); return MOCCA_E_ARG;
  }
  if (need_heightfield(h, "mocca_render: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> ids((size_t)n_views);
  HIP_TRY(h, hipMemcpyAsync(ids.data(), env_ids_dev, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  for (int v = 0; v < n_views; ++v)
    if (ids[v] < 0 || ids[v] >= h->n_envs) {
      h->err = "mocca_render: env index " + std::to_string(ids[v]) + " (view " + std::to_string(v) + ") is outside 0 .. " + std::to_string(h->n_envs - 1);
      return MOCCA_E_ARG;
    }
  if (n_views > h->scenes_cap) {   // grow: an earlier render in flight may still read the old scenes
    DevBuf<float> scenes;
    if (int rc = commit_ready(h, "mocca_render", scenes.alloc((size_t)n_views * mocca_rdr::SCENE_WORDS, false))) return rc;
    h->d_scenes.swap(scenes);
    h->scenes_cap = n_views;
  }
  if (int rc = flush_pending(h, s)) return rc;
  mocca_rdr::launch_scene(s, scene_args(h), env_ids_dev, h->n_envs, n_views, h->d_scenes);
  HIP_TRY(h, hipGetLastError());
  mocca_rdr::launch_raycast(s, h->d_scenes, cameras_dev, n_views, width, height, h->task_id, h->model.plank_shape, h->model.plank_half,
                            heightfield_record(h), env_ids_dev, rgb_dev, depth_dev, id_dev);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, "mocca_render"); }

int mocca_set_height_scan(mocca_handle h, const float* points_host, int n_points, double z_above, double max_drop) {
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  if (!points_host) {   // detach
    if (int rc = commit_ready(h, "mocca_set_height_scan")) return rc;
    h->d_scan_pts.reset(); h->scan_n = 0;
    return MOCCA_OK;
  }
  auto bad = [&](const std::string& what) { h->err = "mocca_set_height_scan: " + what; return MOCCA_E_ARG; };
  if (n_points < 1 || n_points > MOCCA_SCAN_MAX_POINTS) return bad("n_points must be 1 .. " + std::to_string(MOCCA_SCAN_MAX_POINTS));
  if (!std::isfinite(z_above) || !std::isfinite(max_drop) || z_above < 0.0 || !(max_drop > 0.0)) return bad("needs a finite z_above >= 0 and max_drop > 0");
  for (int k = 0; k < 2 * n_points; ++k)
    if (!std::isfinite(points_host[k])) return bad("point " + std::to_string(k / 2) + " is not finite");
  DevBuf<float> pts;
  hipError_t e = pts.alloc((size_t)n_points * 2, false);
  if (e == hipSuccess) e = hipMemcpy(pts, points_host, (size_t)n_points * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(h, "mocca_set_height_scan", e)) return rc;
  h->d_scan_pts.swap(pts);
  h->scan_n = n_points; h->scan_above = (float)z_above; h->scan_drop = (float)max_drop;
  return MOCCA_OK;
}

int mocca_scan_dim(mocca_handle h) { return h ? h->scan_n : MOCCA_E_ARG; }

int mocca_height_scan(mocca_handle h, float* out_dev, int row_stride, const float* obs_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->d_scan_pts) { h->err = "mocca_height_scan: no scan pattern (mocca_set_height_scan)"; return MOCCA_E_ARG; }
  if (!out_dev) { h->err = "mocca_height_scan: out_dev must not be NULL"; return MOCCA_E_ARG; }
  const int width = h->scan_n + (obs_dev ? h->obs_dim : 0);
  if (row_stride < width) {
    h->err = "mocca_height_scan: row_stride " + std::to_string(row_stride) + " is smaller than the row (" + std::to_string(width) + " floats)";
    return MOCCA_E_ARG;
  }
  if (need_heightfield(h, "mocca_height_scan: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  mocca_scan::ScanArgs a{};
  a.scene = scene_args(h);
  a.hf = heightfield_record(h);
  a.points = h->d_scan_pts; a.n_points = h->scan_n; a.z_above = h->scan_above; a.max_drop = h->scan_drop;
  a.out = out_dev; a.row_stride = row_stride; a.obs = obs_dev; a.obs_dim = obs_dev ? h->obs_dim : 0;
  mocca_scan::launch_height_scan((hipStream_t)stream, a, h->n_envs);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_set_depth_camera(mocca_handle h, int body, const float* mount_host, int width, int height, double fov_y, double near, double far, int flags) {
  if (!h) return MOCCA_E_ARG;
  if (!mount_host) {   // detach
    h->depth_on = false;
    return MOCCA_OK;
  }
  auto bad = [&](const std::string& what) { h->err = "mocca_set_depth_camera: " + what; return MOCCA_E_ARG; };
  if (body < 0 || body >= h->model.n_bodies) return bad("body " + std::to_string(body) + " is outside 0 .. " + std::to_string(h->model.n_bodies - 1));
  if (width < 1 || width > 64 || height < 1 || height > 64 || width * height > MOCCA_DEPTH_MAX_PIXELS)
    return bad("width and height must be 1 .. 64 and their product at most " + std::to_string(MOCCA_DEPTH_MAX_PIXELS));
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(mount_host[k])) return bad("mount entry " + std::to_string(k) + " is not finite");
  if (!(fov_y > 0.0 && fov_y < 3.14159265358979323846)) return bad("fov_y must lie in (0, pi) radians");
  if (!std::isfinite(near) || !std::isfinite(far) || !(near > 0.0) || !(far > near)) return bad("needs finite 0 < near < far");
  if (flags & ~(MOCCA_DEPTH_STABILISED | MOCCA_DEPTH_SEE_ROBOT)) return bad("unknown flag bits " + std::to_string(flags & ~(MOCCA_DEPTH_STABILISED | MOCCA_DEPTH_SEE_ROBOT)));
  mocca_depth::DepthArgs a{};
  a.body = body; a.width = width; a.height = height; a.flags = flags;
  for (int k = 0; k < 3; ++k) a.offset[k] = mount_host[k];
  mocca_rdr::euler_to_mat(mount_host[3], mount_host[4], mount_host[5], a.axes);
  a.tan_half_fov = (float)std::tan(0.5 * fov_y); a.near = (float)near; a.far = (float)far;
  if (!std::isfinite(a.tan_half_fov) || !(a.near > 0.0f) || !(a.far > a.near)) return bad("fov_y, near and far must stay distinct and finite in float32");
  h->depth = a; h->depth_on = true;
  return MOCCA_OK;
}

int mocca_depth_dim(mocca_handle h) { return h ? (h->depth_on ? h->depth.width * h->depth.height : 0) : MOCCA_E_ARG; }

int mocca_depth_camera(mocca_handle h, float* out_dev, int row_stride, const float* obs_dev, float* cameras_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!h->depth_on) { h->err = "mocca_depth_camera: no camera (mocca_set_depth_camera)"; return MOCCA_E_ARG; }
  if (!out_dev) { h->err = "mocca_depth_camera: out_dev must not be NULL"; return MOCCA_E_ARG; }
  const int width = h->depth.width * h->depth.height + (obs_dev ? h->obs_dim : 0);
  if (row_stride < width) {
    h->err = "mocca_depth_camera: row_stride " + std::to_string(row_stride) + " is smaller than the row (" + std::to_string(width) + " floats)";
    return MOCCA_E_ARG;
  }
  if (need_heightfield(h, "mocca_depth_camera: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  mocca_depth::DepthArgs a = h->depth;
  a.scene = scene_args(h);
  a.hf = heightfield_record(h);
  a.out = out_dev; a.row_stride = row_stride; a.obs = obs_dev; a.obs_dim = obs_dev ? h->obs_dim : 0; a.cameras = cameras_dev;
  mocca_depth::launch_depth_camera((hipStream_t)stream, a, h->n_envs);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
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
static int set_policy_slot(mocca_handle h, const char* name, bool student, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim,
                           double clip, bool priv = false, int critic_in_dim = 0) try {
  using namespace mocca_pol;
  if (!h) return MOCCA_E_ARG;
  mocca_ctx::PolicySlot& slot = student ? h->student : h->teacher;
  DeviceGuard guard(h->device);
  auto bad = [&](const std::string& what) { h->err = std::string(name) + ": " + what; return MOCCA_E_ARG; };
  if (priv && h->pol_mirror.method != mocca_ppo::PPO_PLAIN)   // also for a detach: the caller says what goes first
    return bad(std::string("a mirror attachment is in place (") + (h->pol_mirror.method == mocca_ppo::PPO_SYM ? "mocca_set_policy_symmetry" : h->pol_mirror.method == mocca_ppo::PPO_MIRROR ? "mocca_set_policy_mirror_loss" : "mocca_set_policy_mirror_dup") +
               "): mirror tables for the critic's row are not provided, detach it first");
  if (!layers_host) {   // detach
    if (int rc = commit_ready(h, name)) return rc;
    slot.d_pol_image.reset(); slot.d_pol_layers.reset(); slot.pol_filled = false;
    if (student) { drop_policy_mirror(h); h->critic_rows = nullptr; h->critic_stride = 0; slot.pol.critic_in_dim = 0; }
    return MOCCA_OK;
  }
  if (in_dim < 1 || in_dim > POL_MAX_IN) return bad("in_dim must be 1 .. " + std::to_string(POL_MAX_IN));
  if (priv && (critic_in_dim < 1 || critic_in_dim > POL_MAX_IN)) return bad("critic_in_dim must be 1 .. " + std::to_string(POL_MAX_IN));
  if (act_dim < 1 || act_dim > POL_MAX_ACTION) return bad("act_dim must be 1 .. " + std::to_string(POL_MAX_ACTION));
  if (!std::isfinite(clip) || !(clip > 0.0)) return bad("clip must be finite and positive");
  int count[2];
  const std::string takes = priv ? "the actor's first layer takes in_dim = " + std::to_string(in_dim) + " inputs and the critic's critic_in_dim = " +
                                       std::to_string(critic_in_dim) + ", not %d"
                                 : "a net's first layer takes in_dim = " + std::to_string(in_dim) + " inputs, not %d";
  const std::string wrong = check_layer_table(layers_host, n_layers_total, in_dim, act_dim, NO_OFFSETS, takes,
                                              "the actor ends in act_dim = " + std::to_string(act_dim) + " outputs, the critic in 1", count,
                                              priv ? critic_in_dim : 0);
  if (!wrong.empty()) return bad(wrong);
  NetImage im;
  if (int rc = commit_ready(h, name, build_image(im, layers_host, n_layers_total, count, in_dim, act_dim, true, priv ? critic_in_dim : 0))) return rc;
  if (student) { h->critic_rows = nullptr; h->critic_stride = 0; }
  slot.d_pol_image.swap(im.image); slot.d_pol_layers.swap(im.layers);
  slot.pol = im.pa; slot.pol.clip = (float)clip;
  slot.pol_repack = im.rp; slot.pol_n_base = im.n_src; slot.pol_filled = false;
  slot.pol_tail_row = im.tail_row; slot.pol_table.swap(im.table);
  std::memcpy(slot.pol_wt_off, im.wt_off, sizeof(im.wt_off));
  if (student) drop_policy_mirror(h);   // the shapes may have changed
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, name); }

int mocca_set_policy(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim, double clip) {
  return set_policy_slot(h, "mocca_set_policy", true, layers_host, n_layers_total, in_dim, act_dim, clip);
}

int mocca_set_policy_priv(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int critic_in_dim, int act_dim, double clip) {
  return set_policy_slot(h, "mocca_set_policy_priv", true, layers_host, n_layers_total, in_dim, act_dim, clip, true, critic_in_dim);
}

int mocca_set_critic_rows(mocca_handle h, const float* rows_dev, int row_stride) {
  if (!h) return MOCCA_E_ARG;
  auto bad = [&](const std::string& what) { h->err = "mocca_set_critic_rows: " + what; return MOCCA_E_ARG; };
  if (!rows_dev) { h->critic_rows = nullptr; h->critic_stride = 0; return MOCCA_OK; }   // detach
  const mocca_pol::PolicyArgs& p = h->student.pol;
  if (!h->student.d_pol_image || !p.critic_in_dim)
    return bad("needs a policy with a privileged critic (mocca_set_policy_priv): the plain policy's critic reads mocca_act's in_dev");
  if (row_stride < p.critic_in_dim)
    return bad("row_stride " + std::to_string(row_stride) + " is smaller than the policy's critic_in_dim (" + std::to_string(p.critic_in_dim) + ")");
  h->critic_rows = rows_dev; h->critic_stride = row_stride;
  return MOCCA_OK;
}

int mocca_set_teacher(mocca_handle h, const int32_t* layers_host, int n_layers_total, int in_dim, int act_dim, double clip) {
  return set_policy_slot(h, "mocca_set_teacher", false, layers_host, n_layers_total, in_dim, act_dim, clip);
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
static int set_policy_mirror(mocca_handle h, const char* name, mocca_ppo::PpoMode method, const int32_t* in_perm_host, const float* in_sign_host,
                             const int32_t* act_perm_host, const float* act_sign_host, double mirror_coef) try {
  using namespace mocca_ppo;
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  auto bad = [&](const std::string& what) { h->err = std::string(name) + ": " + what; return MOCCA_E_ARG; };
  if (!h->student.d_pol_image) return bad("needs a policy (mocca_set_policy)");
  if (in_perm_host && h->student.pol.critic_in_dim)
    return bad("the policy has a privileged critic (mocca_set_policy_priv): mirror tables for the critic's row are not provided, set a plain policy first (mocca_set_policy)");
  if (!in_perm_host) {   // detach
    if (int rc = commit_ready(h, name)) return rc;
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
  if (const char* why = refusal[method][h->pol_mirror.method]) return bad(why);
  if (!std::isfinite(mirror_coef) || mirror_coef < 0.0) return bad("mirror_coef must be finite and not negative");
  DevBuf<int32_t> d_perm;
  DevBuf<float> d_sign;
  hipError_t e = hipSuccess;
  const std::string wrong = upload_mirror_tables(h, in_perm_host, in_sign_host, act_perm_host, act_sign_host, d_perm, d_sign, &e);
  if (!wrong.empty()) return bad(wrong);
  if (int rc = commit_ready(h, name, e)) return rc;
  h->pol_mirror.perm.swap(d_perm); h->pol_mirror.sign.swap(d_sign);
  h->pol_mirror.method = method; h->pol_mirror.coef = mirror_coef;
  if (method == PPO_SYM) {   // the policy kernel's symmetric instance runs from here on (launch_policy)
    const int in_dim = h->student.pol.in_dim;
    h->student.pol.in_perm = h->pol_mirror.perm; h->student.pol.act_perm = h->pol_mirror.perm.get() + in_dim;
    h->student.pol.in_sign = h->pol_mirror.sign; h->student.pol.act_sign = h->pol_mirror.sign.get() + in_dim;
  }
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(h, name); }

int mocca_set_policy_symmetry(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                              const float* act_sign_host) {
  return set_policy_mirror(h, "mocca_set_policy_symmetry", mocca_ppo::PPO_SYM, in_perm_host, in_sign_host, act_perm_host, act_sign_host, 0.0);
}

int mocca_set_policy_mirror_loss(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                                 const float* act_sign_host, double mirror_coef) {
  return set_policy_mirror(h, "mocca_set_policy_mirror_loss", mocca_ppo::PPO_MIRROR, in_perm_host, in_sign_host, act_perm_host, act_sign_host, mirror_coef);
}

int mocca_set_policy_mirror_dup(mocca_handle h, const int32_t* in_perm_host, const float* in_sign_host, const int32_t* act_perm_host,
                                const float* act_sign_host) {
  return set_policy_mirror(h, "mocca_set_policy_mirror_dup", mocca_ppo::PPO_DUP, in_perm_host, in_sign_host, act_perm_host, act_sign_host, 0.0);
}

// what n_floats of a flat parameter tensor must be (mocca_update_policy, mocca_update_teacher, mocca_adam_step): -> "" or what is wrong
static std::string check_n_floats(const mocca_ctx::PolicySlot& slot, size_t n_floats) {
  const size_t base = slot.pol_n_base, in_dim = (size_t)slot.pol.in_dim, critic_in = (size_t)slot.pol.critic_in_dim;
  if (n_floats == base || n_floats == base + 2 * in_dim + 2 * critic_in) return "";
  return "this policy takes " + std::to_string(base) + " floats (layers, log_std), or " + std::to_string(base + 2 * in_dim + 2 * critic_in) +
         (critic_in ? " with mean, inv_std, critic_mean and critic_inv_std, not " : " with mean and inv_std, not ") + std::to_string(n_floats);
}

// the repack launch of mocca_update_policy / mocca_update_teacher; n_floats has been checked, the handle's device is current
static void repack_policy(const mocca_ctx::PolicySlot& slot, const float* params_dev, size_t n_floats, hipStream_t s) {
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

// mocca_update_policy and mocca_update_teacher: new weights for the slot's image, one repack launch
static int update_policy_slot(mocca_handle h, const char* name, const char* setter, bool student, const float* params_dev, size_t n_floats,
                              void* stream) {
  if (!h) return MOCCA_E_ARG;
  mocca_ctx::PolicySlot& slot = student ? h->student : h->teacher;
  if (!slot.d_pol_image) { h->err = std::string(name) + " needs a policy (" + setter + ")"; return MOCCA_E_ARG; }
  if (!params_dev) { h->err = std::string(name) + ": params_dev must not be NULL"; return MOCCA_E_ARG; }
  const std::string wrong = check_n_floats(slot, n_floats);
  if (!wrong.empty()) { h->err = std::string(name) + ": " + wrong; return MOCCA_E_ARG; }
  DeviceGuard guard(h->device);
  repack_policy(slot, params_dev, n_floats, (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  slot.pol_filled = true;
  return MOCCA_OK;
}

int mocca_update_policy(mocca_handle h, const float* params_dev, size_t n_floats, void* stream) {
  return update_policy_slot(h, "mocca_update_policy", "mocca_set_policy", true, params_dev, n_floats, stream);
}

int mocca_update_teacher(mocca_handle h, const float* params_dev, size_t n_floats, void* stream) {
  return update_policy_slot(h, "mocca_update_teacher", "mocca_set_teacher", false, params_dev, n_floats, stream);
}

// mocca_teacher_act: the teacher's slot through the policy kernel's plain instance, deterministic, over n_rows rows.  That path of the kernel
// reads no env record and no noise; the mean IS the deterministic action, so mean_dev stands in the kernel's action output.
int mocca_teacher_act(mocca_handle h, const float* in_dev, int in_stride, int64_t n_rows, float* mean_dev, float* value_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  auto bad = [&](const std::string& what) { h->err = "mocca_teacher_act: " + what; return MOCCA_E_ARG; };
  const mocca_ctx::PolicySlot& slot = h->teacher;
  if (!slot.d_pol_image || !slot.pol_filled) return bad("needs a teacher (mocca_set_teacher, then mocca_update_teacher)");
  if (!in_dev || !mean_dev) return bad("in_dev and mean_dev must not be NULL");
  if (in_stride < slot.pol.in_dim)
    return bad("in_stride " + std::to_string(in_stride) + " is smaller than the teacher's in_dim (" + std::to_string(slot.pol.in_dim) + ")");
  if (n_rows < 1 || n_rows > mocca_ppo::PPO_MAX_ROWS) return bad("n_rows must be 1 .. 2^22, not " + std::to_string(n_rows));
  DeviceGuard guard(h->device);
  mocca_pol::PolicyArgs a = slot.pol;   // (a teacher has no mirror tables: the plain instance)
  a.in = in_dev; a.in_stride = in_stride; a.eps = nullptr; a.deterministic = 1;
  a.action = mean_dev; a.logp = nullptr; a.value = value_dev; a.mean = nullptr; a.n_envs = (int)n_rows;
  mocca_pol::launch_policy((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

// the policy kernel's launch of mocca_act / mocca_act_step; the handle's device is current
static int launch_act(mocca_handle h, const char* who, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev,
                      float* logp_dev, float* value_dev, float* mean_dev, hipStream_t s) {
  if (!h->student.d_pol_image || !h->student.pol_filled) {
    h->err = std::string(who) + " needs a policy (mocca_set_policy, then mocca_update_policy)"; return MOCCA_E_ARG;
  }
  if (!in_dev || !action_dev) { h->err = std::string(who) + ": in_dev and action_dev must not be NULL"; return MOCCA_E_ARG; }
  if (in_stride < h->student.pol.in_dim) {
    h->err = std::string(who) + ": in_stride " + std::to_string(in_stride) + " is smaller than the policy's in_dim (" + std::to_string(h->student.pol.in_dim) + ")";
    return MOCCA_E_ARG;
  }
  if ((long long)h->env_offset + h->n_envs > (1ll << 28) || h->env_offset < 0) {
    h->err = std::string(who) + ": the noise is keyed by global env ids below 2^28 (MOCCA_PARAM_ENV_OFFSET + n_envs)"; return MOCCA_E_ARG;
  }
  if (h->student.pol.critic_in_dim && value_dev && !h->critic_rows) {
    h->err = std::string(who) + ": the policy's critic reads rows of its own: bind them (mocca_set_critic_rows), or pass value_dev NULL"; return MOCCA_E_ARG;
  }
  mocca_pol::PolicyArgs a = h->student.pol;
  a.critic_in = h->critic_rows; a.critic_stride = h->critic_stride;
  a.in = in_dev; a.in_stride = in_stride; a.eps = eps_dev; a.deterministic = deterministic != 0;
  a.task = h->d_task; a.task_words = MOCCA_TASK_WORDS; a.tw_t = MOCCA_TW_T; a.tw_episode = MOCCA_TW_EPISODE;
  a.env_offset = h->env_offset; a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
  a.action = action_dev; a.logp = logp_dev; a.value = value_dev; a.mean = mean_dev; a.n_envs = h->n_envs;
  mocca_pol::launch_policy(s, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_act(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev, float* logp_dev,
              float* value_dev, float* mean_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  return launch_act(h, "mocca_act", in_dev, in_stride, eps_dev, deterministic, action_dev, logp_dev, value_dev, mean_dev, (hipStream_t)stream);
}

int mocca_act_step(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* action_dev, float* logp_dev,
                   float* value_dev, float* mean_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (!obs_dev || !rew_dev || !done_dev) { h->err = "mocca_act_step: obs_dev, rew_dev and done_dev must not be NULL"; return MOCCA_E_ARG; }
  if (h->student.d_pol_image && h->student.pol.act_dim != mocca_act_dim(h)) {
    h->err = "mocca_act_step: the policy's act_dim (" + std::to_string(h->student.pol.act_dim) + ") is not the env's (" + std::to_string(mocca_act_dim(h)) + ")";
    return MOCCA_E_ARG;
  }
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_act(h, "mocca_act_step", in_dev, in_stride, eps_dev, deterministic, action_dev, logp_dev, value_dev, mean_dev, s)) return rc;
  return launch_step(h, action_dev, nullptr, obs_dev, rew_dev, done_dev, info_dev, s);
}

int mocca_act_plan_step(mocca_handle h, const float* in_dev, int in_stride, const float* eps_dev, int deterministic, float* plan_dev, float* logp_dev,
                        float* value_dev, float* mean_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  if (!h) return MOCCA_E_ARG;
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) { h->err = "mocca_act_plan_step: only the planner task takes plans"; return MOCCA_E_ARG; }
  if (!obs_dev || !rew_dev || !done_dev) { h->err = "mocca_act_plan_step: obs_dev, rew_dev and done_dev must not be NULL"; return MOCCA_E_ARG; }
  if (!h->d_ctrl_image) { h->err = "mocca_act_plan_step needs a base controller (mocca_set_base_controller)"; return MOCCA_E_ARG; }
  if (h->student.d_pol_image && h->student.pol.act_dim != mocca_ctrl::CTRL_PLAN) {
    h->err = "mocca_act_plan_step: the policy's act_dim (" + std::to_string(h->student.pol.act_dim) + ") is not the plan's (" + std::to_string(mocca_ctrl::CTRL_PLAN) + ")";
    return MOCCA_E_ARG;
  }
  if (need_attachments(h) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_act(h, "mocca_act_plan_step", in_dev, in_stride, eps_dev, deterministic, plan_dev, logp_dev, value_dev, mean_dev, s)) return rc;
  mocca_ctrl::ControllerArgs c = h->ctrl;
  c.plan = plan_dev;
  mocca_ctrl::launch_controller(s, c);
  HIP_TRY(h, hipGetLastError());
  return launch_step(h, h->d_base_act, h->d_base_val, obs_dev, rew_dev, done_dev, info_dev, s);
}

// scratch of the rollout kernels: allocated on the first call and on one that needs more; only such a call synchronises
static int grow_scratch(mocca_handle h, const char* who, DevBuf<double>& buf, size_t* cap, size_t need) {
  if (need <= *cap) return MOCCA_OK;
  DevBuf<double> next;
  hipError_t e = buf ? hipDeviceSynchronize() : hipSuccess;   // a launch in flight may still use the old one
  if (e == hipSuccess) e = next.alloc(need, false);
  if (e != hipSuccess) { h->err = std::string(who) + ": scratch: " + hipGetErrorString(e); return MOCCA_E_HIP; }
  buf.swap(next);
  *cap = need;
  return MOCCA_OK;
}

int mocca_gae(mocca_handle h, const float* rew_dev, const float* value_dev, const float* masks_dev, const float* bad_masks_dev, int n_steps,
              double gamma, double lam, double reward_scale, float* returns_dev, float* adv_dev, int normalise, double adv_eps,
              float* moments_dev, void* stream) {
  if (!h) { g_err = "mocca_gae: NULL handle"; return MOCCA_E_ARG; }
  auto bad = [&](const std::string& what) { h->err = "mocca_gae: " + what; return MOCCA_E_ARG; };
  if (!rew_dev || !value_dev || !masks_dev || !bad_masks_dev) return bad("rew_dev, value_dev, masks_dev and bad_masks_dev must not be NULL");
  if (normalise && (!adv_dev || !moments_dev)) return bad("normalise needs adv_dev and moments_dev");
  if (n_steps < 1 || n_steps > 65536) return bad("n_steps must be 1 .. 65536, not " + std::to_string(n_steps));
  const long long count = (long long)n_steps * h->n_envs;
  if (normalise && count < 2) return bad("normalise needs at least two advantages (n_steps x n_envs >= 2)");
  if (!std::isfinite(gamma) || !std::isfinite(lam) || !std::isfinite(reward_scale)) return bad("gamma, lam and reward_scale must be finite");
  if (!std::isfinite(adv_eps) || adv_eps < 0.0) return bad("adv_eps must be finite and not negative");
  DeviceGuard guard(h->device);
  const int blocks = mocca_ro::gae_blocks(h->n_envs);
  if (int rc = grow_scratch(h, "mocca_gae", h->d_gae_part, &h->gae_part_cap, 2 * (size_t)blocks)) return rc;
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
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_obs_stats(mocca_handle h, const float* rows_dev, int64_t n_rows, int row_stride, int dim, double* state_dev, double eps, float* mean_dev,
                    float* inv_std_dev, void* stream) {
  if (!h) { g_err = "mocca_obs_stats: NULL handle"; return MOCCA_E_ARG; }
  auto bad = [&](const std::string& what) { h->err = "mocca_obs_stats: " + what; return MOCCA_E_ARG; };
  if (!rows_dev || !state_dev) return bad("rows_dev and state_dev must not be NULL");
  if (dim < 1 || dim > mocca_ro::OBS_MAX_DIM) return bad("dim must be 1 .. " + std::to_string(mocca_ro::OBS_MAX_DIM) + ", not " + std::to_string(dim));
  if (row_stride < dim) return bad("row_stride " + std::to_string(row_stride) + " is smaller than dim (" + std::to_string(dim) + ")");
  if (n_rows < 1) return bad("n_rows must be at least 1");
  if (!std::isfinite(eps) || eps < 0.0) return bad("eps must be finite and not negative");
  DeviceGuard guard(h->device);
  mocca_ro::ObsArgs a{};
  a.rows = rows_dev; a.n_rows = n_rows; a.row_stride = row_stride; a.dim = dim;
  mocca_ro::obs_grid(n_rows, dim, &a.rows_per_block, &a.n_blocks);
  if (int rc = grow_scratch(h, "mocca_obs_stats", h->d_obs_part, &h->obs_part_cap, 2 * (size_t)a.n_blocks * dim)) return rc;
  a.state = state_dev; a.partials = h->d_obs_part; a.eps = (float)eps; a.mean_out = mean_dev; a.inv_std_out = inv_std_dev;
  mocca_ro::launch_obs_stats((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

// what the handle's attachment makes mocca_ppo_update differentiate: duplicated rows, the mirror loss, the symmetric network, or the plain policy
static mocca_ppo::PpoMode ppo_mode(mocca_handle h) { return h->pol_mirror.method; }

// mocca_ppo_grad (PPO_PLAIN), mocca_ppo_grad_sym (PPO_SYM), mocca_ppo_grad_mirror (PPO_MIRROR) and mocca_ppo_grad_dup (PPO_DUP): one argument
// list, one scratch, the same four launches; the last three share the two-column scratch layout (mocca_ppo.h).  mocca_distill_grad (PPO_DISTIL) is
// the plain call with another head stage: action_dev carries the targets, returns_dev the value targets (or NULL) and `clip` distill_coef;
// old_logp_dev, adv_dev and old_value_dev are not read.
static int ppo_grad(mocca_handle h, const char* name, mocca_ppo::PpoMode mode, const float* obs_dev, int obs_stride, const float* action_dev,
                    const float* old_logp_dev, const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev,
                    int64_t n_rows, double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev,
                    void* stream, bool check_only = false,   // check_only: the refusals alone (mocca_ppo_update asks before its first launch)
                    const float* critic_obs_dev = nullptr, int critic_stride = 0) {   // PPO_PRIV (mocca_ppo_grad_priv): the storage's critic rows
  using namespace mocca_ctrl;
  using namespace mocca_ppo;
  if (!h) { g_err = std::string(name) + ": NULL handle"; return MOCCA_E_ARG; }
  auto bad = [&](const std::string& what) { h->err = std::string(name) + ": " + what; return MOCCA_E_ARG; };
  if (!h->student.d_pol_image || !h->student.pol_filled) return bad("needs a policy (mocca_set_policy, then mocca_update_policy)");
  const bool distil = mode == PPO_DISTIL;
  const bool priv = mode == PPO_PRIV;
  const bool sym = mode != PPO_PLAIN && !distil && !priv;   // twice the columns
  if (const bool has = h->student.pol.critic_in_dim != 0; has != priv) {   // (a privileged critic and a mirror attachment exclude each other)
    if (has && distil) return bad("the policy has a privileged critic (mocca_set_policy_priv): distilling into an asymmetric student is not provided");
    if (has) return bad("the policy has a privileged critic (mocca_set_policy_priv): its gradient is mocca_ppo_grad_priv, its update mocca_ppo_update_priv");
    return bad("needs a policy with a privileged critic (mocca_set_policy_priv); the plain policy's gradient is mocca_ppo_grad, its update mocca_ppo_update");
  }
  if (priv) {
    if (!critic_obs_dev) return bad("critic_obs_dev must not be NULL");
    if (critic_stride < h->student.pol.critic_in_dim)
      return bad("critic_stride " + std::to_string(critic_stride) + " is smaller than the policy's critic_in_dim (" + std::to_string(h->student.pol.critic_in_dim) + ")");
  } else if (const PpoMode attached = ppo_mode(h); distil) {
    if (attached != PPO_PLAIN)
      return bad(std::string("a mirror attachment is in place (") + (attached == PPO_SYM ? "mocca_set_policy_symmetry" : attached == PPO_MIRROR ? "mocca_set_policy_mirror_loss" : "mocca_set_policy_mirror_dup") +
                 "): the regression gradient is the plain policy's, detach it first");
  } else if (mode != attached) {   // the first of these that holds names the entry point to call instead
    if (attached == PPO_DUP)
      return bad("duplicated rows are attached: the gradient of PPO's loss over the rows and their mirror images is mocca_ppo_grad_dup (or detach them: mocca_set_policy_mirror_dup)");
    if (mode == PPO_DUP) return bad("needs duplicated rows attached (mocca_set_policy_mirror_dup); the plain loss's gradient is mocca_ppo_grad");
    if (attached == PPO_MIRROR)
      return bad("a mirror loss is attached: the gradient of PPO's loss with the mirror term is mocca_ppo_grad_mirror (or detach it: mocca_set_policy_mirror_loss)");
    if (mode == PPO_MIRROR) return bad("needs a mirror loss attached (mocca_set_policy_mirror_loss); the plain loss's gradient is mocca_ppo_grad");
    if (mode == PPO_PLAIN)
      return bad("the policy has mirror tables attached: the symmetric policy's gradient is mocca_ppo_grad_sym (or detach the tables: mocca_set_policy_symmetry)");
    return bad("needs a policy with mirror tables attached (mocca_set_policy_symmetry); the plain policy's gradient is mocca_ppo_grad");
  }
  if (distil && (!obs_dev || !action_dev || !grad_dev)) return bad("obs_dev, target_dev and grad_dev must not be NULL");
  if (!distil && (!obs_dev || !action_dev || !old_logp_dev || !adv_dev || !returns_dev || !grad_dev))
    return bad("obs_dev, action_dev, old_logp_dev, adv_dev, returns_dev and grad_dev must not be NULL");
  if (value_clip && !old_value_dev) return bad("value_clip needs old_value_dev");
  if (n_rows < 1 || n_rows > (sym ? PPO_MAX_ROWS_SYM : PPO_MAX_ROWS)) return bad(std::string("n_rows must be 1 .. ") + (sym ? "2^21" : "2^22") + ", not " + std::to_string(n_rows));
  if (obs_stride < h->student.pol.in_dim)
    return bad("obs_stride " + std::to_string(obs_stride) + " is smaller than the policy's in_dim (" + std::to_string(h->student.pol.in_dim) + ")");
  if (!std::isfinite(clip) || clip < 0.0 || !std::isfinite(value_coef) || value_coef < 0.0 || !std::isfinite(entropy_coef) || entropy_coef < 0.0)
    return bad(distil ? "distill_coef and value_coef must be finite and not negative" : "clip, value_coef and entropy_coef must be finite and not negative");
  if (check_only) return MOCCA_OK;
  DeviceGuard guard(h->device);
  PpoArgs a{};
  const mocca_pol::PolicyArgs& p = h->student.pol;
  a.params = p.params; a.layers = p.layers; a.n_actor = p.n_actor; a.n_critic = p.n_critic;
  a.log_std_off = p.log_std_off; a.flags_off = p.flags_off; a.mean_off = p.mean_off; a.inv_std_off = p.inv_std_off;
  a.in_dim = p.in_dim; a.in_pad = p.in_pad; a.act_dim = p.act_dim; a.norm_clip = p.clip;
  std::memcpy(a.wt_off, h->student.pol_wt_off, sizeof(a.wt_off));
  a.mode = mode;
  if (distil) a.mirror_k2 = (float)(2.0 * clip);   // f32(2 distill_coef), the product in double
  if (sym) {
    a.in_perm = h->pol_mirror.perm; a.act_perm = h->pol_mirror.perm.get() + p.in_dim;
    a.in_sign = h->pol_mirror.sign; a.act_sign = h->pol_mirror.sign.get() + p.in_dim;
    a.mirror_k2 = (float)(2.0 * h->pol_mirror.coef);
  }
  a.obs = obs_dev; a.obs_stride = obs_stride; a.action = action_dev; a.old_logp = old_logp_dev; a.adv = adv_dev; a.returns = returns_dev;
  a.old_value = old_value_dev; a.idx = idx_dev;
  a.n_rows = (int)n_rows;
  a.b_pad = sym ? (int)((n_rows + PPO_SYM_TILE - 1) / PPO_SYM_TILE * 16) : (int)((n_rows + 15) / 16 * 16);   // the scratch's rows (mocca_ppo.h)
  a.clip = (float)clip; a.value_coef = (float)value_coef; a.entropy_coef = (float)entropy_coef; a.inv_b = 1.0f / (float)n_rows;
  a.n_samples = (int)n_rows;
  if (mode == PPO_DUP) { a.n_samples = 2 * (int)n_rows; a.inv_b = 1.0f / (float)a.n_samples; }   // every mean is over the 2 B samples
  a.value_clip = value_clip != 0;
  // the scratch (mocca_ppo.h), in floats; every piece a multiple of 4 floats, so that rows stay 16-byte aligned
  const long long bp = a.b_pad;
  const int n_layers = p.n_actor + p.n_critic;
  long long pos = 0;
  int n_tiles = PPO_ROW_COLS / 16, n_head = p.act_dim;
  a.a0_off = pos; pos += bp * p.in_pad;
  a.a0c_off = a.a0_off;
  if (priv) {   // A0c (mocca_ppo.h: Privileged critic)
    a.critic_obs = critic_obs_dev; a.critic_stride = critic_stride; a.critic_in_dim = p.critic_in_dim; a.critic_in_pad = p.critic_in_pad;
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
  if (int rc = grow_scratch(h, name, h->d_ppo, &h->ppo_cap, f_doubles + (size_t)a.n_reduce_blocks)) return rc;
  a.scratch = (float*)h->d_ppo.get(); a.sq_part = h->d_ppo.get() + f_doubles;
  a.grad = grad_dev; a.stats = stats_dev;
  launch_ppo((hipStream_t)stream, a);
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_ppo_grad(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev, const float* adv_dev,
                   const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows, double clip, double value_coef,
                   double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  return ppo_grad(h, "mocca_ppo_grad", mocca_ppo::PPO_PLAIN, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, idx_dev, n_rows, clip,
                  value_coef, entropy_coef, value_clip, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_sym(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                       const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows, double clip,
                       double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  return ppo_grad(h, "mocca_ppo_grad_sym", mocca_ppo::PPO_SYM, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, idx_dev, n_rows,
                  clip, value_coef, entropy_coef, value_clip, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_mirror(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                          const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows,
                          double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  return ppo_grad(h, "mocca_ppo_grad_mirror", mocca_ppo::PPO_MIRROR, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev,
                  idx_dev, n_rows, clip, value_coef, entropy_coef, value_clip, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_dup(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                       const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev, int64_t n_rows,
                       double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev, void* stream) {
  return ppo_grad(h, "mocca_ppo_grad_dup", mocca_ppo::PPO_DUP, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev,
                  idx_dev, n_rows, clip, value_coef, entropy_coef, value_clip, grad_dev, stats_dev, stream);
}

int mocca_ppo_grad_priv(mocca_handle h, const float* obs_dev, int obs_stride, const float* critic_obs_dev, int critic_stride, const float* action_dev,
                        const float* old_logp_dev, const float* adv_dev, const float* returns_dev, const float* old_value_dev, const int64_t* idx_dev,
                        int64_t n_rows, double clip, double value_coef, double entropy_coef, int value_clip, float* grad_dev, float* stats_dev,
                        void* stream) {
  return ppo_grad(h, "mocca_ppo_grad_priv", mocca_ppo::PPO_PRIV, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev,
                  idx_dev, n_rows, clip, value_coef, entropy_coef, value_clip, grad_dev, stats_dev, stream, false, critic_obs_dev, critic_stride);
}

// the refusals of mocca_adam_step's arguments (mocca_ppo_update shares them): -> MOCCA_OK, or MOCCA_E_ARG with the message set
static int adam_check(mocca_handle h, const char* name, const float* params_dev, size_t n_floats, const float* grad_dev, bool need_grad,
                      int64_t n_params, const float* moments_dev, const double* clock_dev, double lr, double beta1, double beta2, double eps,
                      double max_grad_norm) {
  if (!h) { g_err = std::string(name) + ": NULL handle"; return MOCCA_E_ARG; }
  auto bad = [&](const std::string& what) { h->err = std::string(name) + ": " + what; return MOCCA_E_ARG; };
  if (!h->student.d_pol_image) return bad("needs a policy (mocca_set_policy)");
  if (!params_dev || (need_grad && !grad_dev) || !moments_dev || !clock_dev)
    return bad(std::string("params_dev, ") + (need_grad ? "grad_dev, " : "") + "moments_dev and clock_dev must not be NULL");
  const std::string wrong = check_n_floats(h->student, n_floats);
  if (!wrong.empty()) return bad(wrong);
  if (n_params < 1 || n_params > (int64_t)h->student.pol_n_base)
    return bad("n_params must be 1 .. " + std::to_string(h->student.pol_n_base) + " (the floats ahead of mean / inv_std), not " + std::to_string(n_params));
  if (!std::isfinite(lr) || lr < 0.0 || !std::isfinite(eps) || eps < 0.0) return bad("lr and eps must be finite and not negative");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return bad("beta1 and beta2 must lie in [0, 1)");
  if (std::isnan(max_grad_norm) || max_grad_norm < 0.0) return bad("max_grad_norm must not be NaN or negative (0: no clip)");
  return MOCCA_OK;
}

// f64 words of d_optim ahead of the permutation (mocca_optim.h: Scratch)
static size_t optim_head_words(mocca_handle h) { return mocca_optim::OPT_REC_WORDS + (h->student.pol_n_base + 1) / 2; }

// launches A, B and C of mocca_adam_step; the arguments have been checked, d_optim holds the record, the handle's device is current
static void adam_launch(mocca_handle h, float* params_dev, size_t n_floats, const float* grad_dev, int64_t n_params, float* moments_dev,
                        double* clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, float* stats_row, hipStream_t s) {
  mocca_optim::AdamArgs a{};
  a.params = params_dev; a.grad = grad_dev; a.n_params = (int)n_params;
  a.m = moments_dev; a.v = moments_dev + h->student.pol_n_base; a.clock = clock_dev;
  a.rec = (mocca_optim::AdamRecord*)h->d_optim.get();
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_grad_norm = max_grad_norm; a.stats = stats_row;
  mocca_optim::launch_adam(s, a);
  repack_policy(h->student, params_dev, n_floats, s);
}

int mocca_adam_step(mocca_handle h, float* params_dev, size_t n_floats, const float* grad_dev, int64_t n_params, float* moments_dev,
                    double* clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream) {
  if (int rc = adam_check(h, "mocca_adam_step", params_dev, n_floats, grad_dev, true, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps,
                          max_grad_norm)) return rc;
  DeviceGuard guard(h->device);
  if (int rc = grow_scratch(h, "mocca_adam_step", h->d_optim, &h->optim_cap, optim_head_words(h))) return rc;
  adam_launch(h, params_dev, n_floats, grad_dev, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm, nullptr, (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  h->student.pol_filled = true;
  return MOCCA_OK;
}

int mocca_distill_grad(mocca_handle h, const float* obs_dev, int obs_stride, const float* target_dev, const float* value_target_dev,
                       const int64_t* idx_dev, int64_t n_rows, double distill_coef, double value_coef, float* grad_dev, float* stats_dev,
                       void* stream) {
  return ppo_grad(h, "mocca_distill_grad", mocca_ppo::PPO_DISTIL, obs_dev, obs_stride, target_dev, nullptr, nullptr, value_target_dev, nullptr, idx_dev,
                  n_rows, distill_coef, value_coef, 0.0, 0, grad_dev, stats_dev, stream);
}

// The body of mocca_ppo_update and mocca_distill_update: epochs x (n_rollout_rows / minibatch_rows) minibatches of [shuffle once per epoch,
// the gradient, launches A .. C of mocca_adam_step].  `grad_of(idx, grad, stats_row, check_only)` is the gradient call on minibatch_rows rows;
// asked with check_only it only refuses.  `sym`: the gradient call's scratch has two rows per minibatch row, which halves the row bound.
using UpdateGrad = std::function<int(const int64_t* idx, float* grad, float* stats_row, bool check_only)>;
static int update_loop(mocca_handle h, const char* name, bool sym, int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, float* params_dev,
                       size_t n_floats, int64_t n_params, float* moments_dev, double* clock_dev, double lr, double beta1, double beta2, double eps,
                       double max_grad_norm, uint64_t seed, float* stats_dev, void* stream, const UpdateGrad& grad_of) {
  auto bad = [&](const std::string& what) { h->err = std::string(name) + ": " + what; return MOCCA_E_ARG; };
  const long long most = sym ? mocca_ppo::PPO_MAX_ROWS_SYM : mocca_ppo::PPO_MAX_ROWS;
  if (n_rollout_rows < 1 || n_rollout_rows > most)
    return bad(std::string("n_rollout_rows must be 1 .. ") + (sym ? "2^21" : "2^22") + ", not " + std::to_string(n_rollout_rows));
  if (minibatch_rows < 1 || minibatch_rows > n_rollout_rows)
    return bad("minibatch_rows must be 1 .. n_rollout_rows (" + std::to_string(n_rollout_rows) + "), not " + std::to_string(minibatch_rows));
  if (epochs < 1) return bad("epochs must be at least 1, not " + std::to_string(epochs));
  float* const unset = params_dev;   // stands for grad_dev in the check: the gradient buffer is the handle's
  if (int rc = grad_of(nullptr, unset, nullptr, true)) return rc;
  DeviceGuard guard(h->device);
  const size_t head = optim_head_words(h);
  if (int rc = grow_scratch(h, name, h->d_optim, &h->optim_cap, head + (size_t)n_rollout_rows)) return rc;
  float* const grad = (float*)(h->d_optim.get() + mocca_optim::OPT_REC_WORDS);
  int64_t* const perm = (int64_t*)(h->d_optim.get() + head);
  mocca_optim::ShuffleArgs sh{};
  sh.perm = perm; sh.n = (int)n_rollout_rows; sh.half = mocca_optim::shuffle_half(n_rollout_rows); sh.mask = (1u << sh.half) - 1u;
  sh.seed_lo = (uint32_t)seed; sh.seed_hi = (uint32_t)(seed >> 32); sh.clock = clock_dev;
  const int64_t per_epoch = n_rollout_rows / minibatch_rows;   // BatchSampler(drop_last=True)
  for (int ep = 0; ep < epochs; ++ep) {
    mocca_optim::launch_shuffle((hipStream_t)stream, sh);
    for (int64_t u = 0; u < per_epoch; ++u) {
      float* const row = stats_dev ? stats_dev + 8 * ((size_t)ep * per_epoch + u) : nullptr;
      if (int rc = grad_of(perm + u * minibatch_rows, grad, row, false)) return rc;
      adam_launch(h, params_dev, n_floats, grad, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm, row, (hipStream_t)stream);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return MOCCA_OK;
}

int mocca_ppo_update(mocca_handle h, const float* obs_dev, int obs_stride, const float* action_dev, const float* old_logp_dev,
                     const float* adv_dev, const float* returns_dev, const float* old_value_dev, int64_t n_rollout_rows,
                     int64_t minibatch_rows, int epochs, double clip, double value_coef, double entropy_coef, int value_clip,
                     float* params_dev, size_t n_floats, int64_t n_params, float* moments_dev, double* clock_dev, double lr,
                     double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed, float* stats_dev, void* stream) {
  const char* name = "mocca_ppo_update";
  if (int rc = adam_check(h, name, params_dev, n_floats, nullptr, false, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm))
    return rc;
  const mocca_ppo::PpoMode mode = ppo_mode(h);   // one entry point: the handle's attachments decide, as VecEnv.ppo_grad does
  return update_loop(h, name, mode != mocca_ppo::PPO_PLAIN, n_rollout_rows, minibatch_rows, epochs, params_dev, n_floats, n_params, moments_dev,
                     clock_dev, lr, beta1, beta2, eps, max_grad_norm, seed, stats_dev, stream,
                     [&](const int64_t* idx, float* grad, float* stats_row, bool check_only) {
                       return ppo_grad(h, name, mode, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev, idx,
                                       minibatch_rows, clip, value_coef, entropy_coef, value_clip, grad, stats_row, stream, check_only);
                     });
}

int mocca_ppo_update_priv(mocca_handle h, const float* obs_dev, int obs_stride, const float* critic_obs_dev, int critic_stride,
                          const float* action_dev, const float* old_logp_dev, const float* adv_dev, const float* returns_dev,
                          const float* old_value_dev, int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double clip, double value_coef,
                          double entropy_coef, int value_clip, float* params_dev, size_t n_floats, int64_t n_params, float* moments_dev,
                          double* clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed,
                          float* stats_dev, void* stream) {
  const char* name = "mocca_ppo_update_priv";
  if (int rc = adam_check(h, name, params_dev, n_floats, nullptr, false, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm))
    return rc;
  return update_loop(h, name, false, n_rollout_rows, minibatch_rows, epochs, params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1,
                     beta2, eps, max_grad_norm, seed, stats_dev, stream,
                     [&](const int64_t* idx, float* grad, float* stats_row, bool check_only) {
                       return ppo_grad(h, name, mocca_ppo::PPO_PRIV, obs_dev, obs_stride, action_dev, old_logp_dev, adv_dev, returns_dev, old_value_dev,
                                       idx, minibatch_rows, clip, value_coef, entropy_coef, value_clip, grad, stats_row, stream, check_only,
                                       critic_obs_dev, critic_stride);
                     });
}

int mocca_distill_update(mocca_handle h, const float* obs_dev, int obs_stride, const float* target_dev, const float* value_target_dev,
                         int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double distill_coef, double value_coef, float* params_dev,
                         size_t n_floats, int64_t n_params, float* moments_dev, double* clock_dev, double lr, double beta1, double beta2, double eps,
                         double max_grad_norm, uint64_t seed, float* stats_dev, void* stream) {
  const char* name = "mocca_distill_update";
  if (int rc = adam_check(h, name, params_dev, n_floats, nullptr, false, n_params, moments_dev, clock_dev, lr, beta1, beta2, eps, max_grad_norm))
    return rc;
  return update_loop(h, name, false, n_rollout_rows, minibatch_rows, epochs, params_dev, n_floats, n_params, moments_dev, clock_dev, lr, beta1,
                     beta2, eps, max_grad_norm, seed, stats_dev, stream,
                     [&](const int64_t* idx, float* grad, float* stats_row, bool check_only) {
                       return ppo_grad(h, name, mocca_ppo::PPO_DISTIL, obs_dev, obs_stride, target_dev, nullptr, nullptr, value_target_dev, nullptr,
                                       idx, minibatch_rows, distill_coef, value_coef, 0.0, 0, grad, stats_row, stream, check_only);
                     });
}

#ifdef MOCCA_STAMPS
// diagnostic builds only: the raw s_memtime marks (STAMP_SLOTS per wave) of the most recent launch
int mocca_debug_stamps(unsigned long long* out, int n_waves) {
  if (n_waves > mocca::STAMP_WAVES) n_waves = mocca::STAMP_WAVES;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mocca::g_stamps), (size_t)n_waves * mocca::STAMP_SLOTS * 8) != hipSuccess) return MOCCA_E_HIP;
  return MOCCA_OK;
}
#endif

int mocca_kernel_info(mocca_handle h, int* vgprs, int* sgprs, int* lds_bytes, int* scratch_bytes, int* max_blocks_per_cu) {
  if (!h) return MOCCA_E_ARG;
  hipFuncAttributes fa;
  int nb = 0;
  hipError_t e = hipSuccess;
  switch (step_instance(h)) {
    case INST_COMPACT: mocca_r32_kernel_info(h->topo, h->task_id, &fa, &nb, &e); break;
    case INST_WIDE: mocca_r64_kernel_info(h->topo, h->task_id, &fa, &nb, &e); break;
    default: dispatch<KernelInfo>(h->topo, h->task_id, &fa, &nb, &e);
  }
  HIP_TRY(h, e);
  if (vgprs) *vgprs = fa.numRegs;
  if (sgprs) *sgprs = -1;   // hipFuncAttributes has no scalar-register field: -1 = not reported (the count is in the code object's metadata: build.py -v prints it)
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (max_blocks_per_cu) *max_blocks_per_cu = nb;
  return MOCCA_OK;
}

}  // extern "C"
