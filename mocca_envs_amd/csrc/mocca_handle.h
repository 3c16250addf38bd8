// mocca_handle.h -- private to the C ABI's host units (mocca_api.hip and mocca_api_*.hip), never installed: the handle, the owner of its device
// buffers, the context every entry point refuses through, and the few host functions that cross units.  No kernel and no step-kernel header.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "mocca.h"
#include "mocca_model.h"
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
#include "mocca_curriculum.h"

#pragma GCC visibility push(hidden)   // what follows is shared by the library's units, not exported from it

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

struct mocca_ctx {
  MoccaModel model;
  int task_id = 0, n_envs = 0, device = 0, obs_dim = 0;
  DevBuf<MoccaModel> d_model;
  int topo = 0;  // TOPO_*
  bool planar = false;   // a 2-D tree, or a blob that says so: pushes stay in the plane (mocca_set_randomisation)
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
  int prio = 0;                 // MOCCA_PARAM_ISSUE_PRIORITY; mocca_create sets the step kernel's default thresholds
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
  // the per-env adaptive curriculum (mocca_curriculum.h); its levels are d_pvec[0], the words the step kernel reads
  bool cur_on = false;               // mocca_set_curriculum: with auto_reset, launch_step runs the rule's kernel behind the step kernel
  mocca_cur::CurConfig cur_cfg{};
  DevBuf<int32_t> d_cur_streak;      // [N] owned by the handle; NOT part of a snapshot
  DevBuf<int32_t> d_cur_hold;        // [N]
  DevBuf<int32_t> d_cur_info;        // [N] the step's info words where the caller passes info_dev == NULL
  float* cur_totals = nullptr;       // caller-owned [10][4], or null
  std::string err;
};
extern thread_local std::string g_err;   // the message of a call that has no handle to keep it in (mocca_api.hip)

// The context of one C ABI call, built first in every entry point from the handle and the entry's name: the ONE way a call is refused.  The
// message goes to the handle, or to the thread's g_err when there is none; mocca_last_error returns it (include/mocca.h).
struct Call {
  mocca_handle h;
  const char* name;
  Call(mocca_handle h, const char* name) : h(h), name(name) {}
  // MOCCA_E_ARG with `whole` as the message (the few sentences that do not begin with the entry's name)
  int say(const std::string& whole) const { (h ? h->err : g_err) = whole; return MOCCA_E_ARG; }
  int bad(const std::string& what) const { return say(std::string(name) + ": " + what); }
  int null_handle() const { return bad("NULL handle"); }
  // the sentences that recur; `how`, `colon` and `than` keep each entry's own wording
  int null_arg(const char* args, const char* how = " must not be NULL") const { return bad(std::string(args) + how); }
  int small_stride(const char* stride, long long value, const std::string& than) const {
    return bad(std::string(stride) + " " + std::to_string(value) + " is smaller than " + than);
  }
  int needs(const char* what, const char* setter, bool colon = false) const {
    return say(std::string(name) + (colon ? ": needs " : " needs ") + what + " (" + setter + ")");
  }
  int hip(const std::string& what, hipError_t e) const { (h ? h->err : g_err) = what + ": " + hipGetErrorString(e); return MOCCA_E_HIP; }
  // the end of an entry point that launched: MOCCA_OK, or what the launches left in hipGetLastError()
  int launched() const {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MOCCA_OK : hip("hipGetLastError()", e);
  }
};

// the first line of an entry point that takes the handle: its context `c`, and the refusal of a NULL handle
#define ENTRY(h, entry_name)     \
  const Call c(h, entry_name);   \
  if (!(h)) return c.null_handle()

#define HIP_TRY(c, expr)                                                        \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) return (c).hip(#expr, e_);                             \
  } while (0)

// The ABI boundary of the calls that build host images (std::vector, std::string): a failed host allocation is a code and a message.
inline int out_of_host_memory(const Call& c) { return c.bad("out of host memory"); }

// Attach / replace / detach of what a handle owns (mocca_set_*, mocca_render's scenes) is one sequence: validate; build the new buffers in local
// DevBufs and upload (`e`: how that went); commit_ready; swap the locals into the handle and set its scalar fields.  commit_ready is the last
// step that can fail, so a refused call leaves the handle exactly as it was; after it no launch in flight still reads the old buffers.
inline int commit_ready(const Call& c, hipError_t e = hipSuccess) {
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) return MOCCA_OK;
  return c.hip(c.name, e);
}

// scratch of the rollout kernels: allocated on the first call and on one that needs more; only such a call synchronises
inline int grow_scratch(const Call& c, DevBuf<double>& buf, size_t* cap, size_t need) {
  if (need <= *cap) return MOCCA_OK;
  DevBuf<double> next;
  hipError_t e = buf ? hipDeviceSynchronize() : hipSuccess;   // a launch in flight may still use the old one
  if (e == hipSuccess) e = next.alloc(need, false);
  if (e != hipSuccess) return c.hip(std::string(c.name) + ": scratch", e);
  buf.swap(next);
  *cap = need;
  return MOCCA_OK;
}

// ---- what crosses units ----
// mocca_api.hip: the step kernel's launch and what the sensors read of the handle
int launch_step(const Call& c, const float* act_dev, const float* base_value, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
                hipStream_t s);
int flush_pending(const Call& c, hipStream_t s);
int need_attachments(const Call& c);
int need_heightfield(const Call& c, const char* who, const char* when);
mocca_rdr::HeightFieldBank heightfield_record(mocca_handle h);
mocca_rand::RandKeys rand_keys(mocca_handle h);
mocca_rdr::SceneArgs scene_args(mocca_handle h);
// mocca_api_curriculum.hip: the arguments of the rule's launch on a step's done bytes and info words
mocca_cur::CurArgs curriculum_args(mocca_handle h, const uint8_t* done_dev, const int32_t* info_dev);
// mocca_api_policy.hip: the student's flat parameter tensor, as the optimiser calls of mocca_api_trainer.hip see it
std::string check_n_floats(const mocca_ctx::PolicySlot& slot, size_t n_floats);
void repack_policy(const mocca_ctx::PolicySlot& slot, const float* params_dev, size_t n_floats, hipStream_t s);

#pragma GCC visibility pop
