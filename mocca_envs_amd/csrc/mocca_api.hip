// mocca_api.hip -- kernels' entry points and the part of the C ABI of libmocca_hip.so (include/mocca.h) that the step kernel's launch depends on.
// The host-only features are units of their own: mocca_api_terrain.hip, mocca_api_sensors.hip, mocca_api_policy.hip, mocca_api_trainer.hip,
// mocca_api_curriculum.hip.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see mocca_envs_amd/build.py).
#include <cstdio>

#include "mocca_handle.h"
#include "mocca_kernels.h"

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

static_assert(ROBOT_STATE_STRIDE == mocca_ctrl::CTRL_RS_STRIDE, "the step kernels and the controller kernel share the robot_state buffer");

thread_local std::string g_err;

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
int flush_pending(const Call& c, hipStream_t s) {
  const mocca_handle h = c.h;
  if (!h->gain_pending) return MOCCA_OK;
  launch_per_env(set_task_word_kernel, h, s, h->d_task, MOCCA_TW_APPLIED_GAIN, nullptr, h->gain, 1, h->n_envs);
  HIP_TRY(c, hipGetLastError());
  h->gain_pending = false;
  return MOCCA_OK;
}
// the planner envs stand on the height field (`who`: the calling function and a colon, or nothing; `when`: the end of the sentence)
int need_heightfield(const Call& c, const char* who, const char* when) {
  if (c.h->task_id != MOCCA_TASK_WALKER3D_PLANNER || c.h->d_hf) return MOCCA_OK;
  return c.say(std::string(who) + "the planner task needs mocca_set_heightfield " + when);
}
// ... and this is what the ray caster and the height scan read of it; the other tasks have no grid
mocca_rdr::HeightFieldBank heightfield_record(mocca_handle h) {
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return mocca_rdr::HeightFieldBank{nullptr, 0, 0, 0.0f, nullptr, nullptr, 0};
  return mocca_rdr::HeightFieldBank{h->d_hf, h->hf_rows, h->hf_cols, h->hf_scale, h->d_hf_range, h->hf_n_fields > 1 ? h->d_hf_field.get() : nullptr,
                                    (size_t)h->hf_planes * h->hf_rows * h->hf_cols};
}
// what reset / step / observe cannot run without: the mocap / phase envs read their targets, reset poses and reward references from the
// motion table, the planner envs their ground from the height field
int need_attachments(const Call& c) {
  const mocca_handle h = c.h;
  if (h->task_id == MOCCA_TASK_CASSIE && h->model.cassie_mode != MOCCA_CASSIE_PLAIN && !h->d_traj)
    return c.say("this Cassie blob (cassie_mode != 0) needs mocca_set_trajectory before reset / step / observe");
  return need_heightfield(c, "", "before reset / step / observe");
}

// (mocca_reset stands here, ahead of launch_step: the kernels keep the order in which the host code first names them)
int mocca_reset(mocca_handle h, const uint8_t* mask_dev, uint64_t seed, float* obs_dev, void* stream) {
  ENTRY(h, "mocca_reset");
  if (!obs_dev) return c.null_arg("obs_dev");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  h->seed = seed;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.mask = mask_dev; a.obs = obs_dev;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_pending(c, s)) return rc;
  if (h->tape) {  // recorded draws instead of Philox (mocca_set_draw_tape)
    a.tape = h->tape; a.tape_n = h->tape_n;
    launch_taped_reset(h->topo, h->task_id, h->n_envs, s, a);
  } else {
    dispatch<LaunchReset>(h->topo, h->task_id, h->n_envs, s, a);
  }
  return c.launched();
}

// what the randomisation kernels key their draws by (mocca_randomise.h)
mocca_rand::RandKeys rand_keys(mocca_handle h) {
  return mocca_rand::RandKeys{h->d_task, MOCCA_TASK_WORDS, MOCCA_TW_T, MOCCA_TW_EPISODE, h->env_offset, h->n_envs, (uint32_t)h->seed,
                              (uint32_t)(h->seed >> 32)};
}

// the step-kernel launch of mocca_step / mocca_plan_step (base_value: the controller's value estimates, or null); the handle's device is current
int launch_step(const Call& c, const float* act_dev, const float* base_value, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
                hipStream_t s) {
  const mocca_handle h = c.h;
  StepArgs a = make_args(h);
  a.act = act_dev; a.obs = obs_dev; a.rew = rew_dev; a.done = done_dev; a.info = info_dev;
  a.base_value = base_value;
  const bool judge = h->cur_on && h->auto_reset;   // the adaptive curriculum's launch behind the step kernel (with auto-reset off done is sticky:
  if (judge && !a.info) a.info = h->d_cur_info;    // counting episode ends is then the caller's, mocca_curriculum_apply); it reads the info words
  if (int rc = flush_pending(c, s)) return rc;
  if (h->rand_on) {   // strength, latency and pushes act on what the step kernel reads: one small launch in front of it, nothing without an attachment
    mocca_rand::PerturbArgs p{rand_keys(h), h->rand_cfg, act_dev, h->d_rand_eff, h->d_rand_ring, h->d_dyn, DYN_STRIDE, mocca_act_dim(h)};
    mocca_rand::launch_perturb(s, p);
    HIP_TRY(c, hipGetLastError());
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
      HIP_TRY(c, hipGetLastError());
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
  if (judge) {   // the episodes that ended in this step move their envs' levels: one small launch, nothing without an attachment
    HIP_TRY(c, hipGetLastError());
    mocca_cur::launch_curriculum(s, curriculum_args(h, done_dev, a.info));
  }
  return c.launched();
}

mocca_rdr::SceneArgs scene_args(mocca_handle h) {
  mocca_rdr::SceneArgs a{};
  a.model = h->d_model; a.dyn = h->d_dyn; a.task = h->d_task; a.terrain = h->d_terrain;
  a.dyn_stride = DYN_STRIDE; a.terrain_stride = TERRAIN_STRIDE; a.task_id = h->task_id;
  return a;
}

extern "C" {

int mocca_abi_version(void) { return MOCCA_ABI_VERSION; }
size_t mocca_model_sizeof(void) { return sizeof(MoccaModel); }

const char* mocca_last_error(mocca_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

int mocca_create(const void* model_blob, size_t nbytes, int task_id, int n_envs, int device, mocca_handle* out) try {
  const Call c(nullptr, "mocca_create");
  if (!out) return c.null_arg("out");
  *out = nullptr;
  if (!model_blob || nbytes != sizeof(MoccaModel)) return c.say("model blob has the wrong size");
  if (n_envs <= 0) return c.say("n_envs must be positive");
  if (task_id != MOCCA_TASK_WALKER3D_CUSTOM && task_id != MOCCA_TASK_WALKER3D_STEPPER && task_id != MOCCA_TASK_CASSIE &&
      task_id != MOCCA_TASK_WALKER3D_PLANNER)
    return c.say("unknown task id");
  std::unique_ptr<mocca_ctx> h(new mocca_ctx());   // (every return below that is not the last one frees it, and with it what it owns on the device)
  std::memcpy(&h->model, model_blob, sizeof(MoccaModel));
  if (h->model.magic != MOCCA_MODEL_MAGIC || h->model.version != MOCCA_MODEL_VERSION) return c.say("bad model blob magic/version");
  int rc = check_topology(h->model, task_id, &h->topo, g_err);
  if (rc != MOCCA_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) { g_err = "no such HIP device"; return MOCCA_E_NODEVICE; }
  h->task_id = task_id; h->n_envs = n_envs; h->device = device;
  h->compact = compact_ok(h->model, h->topo);
  h->prio = MOCCA_PRIO_T1 + 64 * MOCCA_PRIO_T2 + 4096 * MOCCA_PRIO_T3;
  h->planar = h->topo == TOPO_WALKER2D || h->topo == TOPO_CRAB2D || h->model.planar != 0;
  h->wide = wide_needed(h->model);
  if (h->wide && mocca_r64_args_sizeof() != sizeof(StepArgs)) return c.say("the 64-row kernel instance was built from another StepArgs");
  // pace priorities make the waves of a SIMD finish together -- right when all of a batch is resident (or whole generations are); the compact
  // instance exists for batches beyond one generation, whose partial last generation wants its slots refilled one by one: measured 1.5 - 2.5 %
  // slower with the pace than with the row-count priorities (8192 / 16384 envs), so its default is off
  if (h->compact) h->pace = 0;
  h->obs_dim = task_id == MOCCA_TASK_CASSIE
                   ? (h->model.cassie_mode == MOCCA_CASSIE_PLAIN ? 6 + 2 * h->model.n_ordered + 2 : 12 + 2 * h->model.n_ordered + 2)  // env_cassie.py:344-346 / :633
                   : 6 + 2 * h->model.n_joints + h->model.n_feet + (task_id == MOCCA_TASK_WALKER3D_STEPPER ? 5 * (h->model.lookbehind + 2) : 2);
  if (task_id == MOCCA_TASK_CASSIE && (h->model.cassie_mode < MOCCA_CASSIE_PLAIN || h->model.cassie_mode > MOCCA_CASSIE_PHASE_MIRROR ||
                                       (h->model.cassie_mode != MOCCA_CASSIE_PLAIN && h->model.n_ordered != 14)))
    return c.say("Cassie blob: unknown cassie_mode (the mocap / phase envs need the 14 ordered joints)");
  if (task_id == MOCCA_TASK_WALKER3D_STEPPER &&
      (h->model.n_planks < 1 || h->model.n_planks > MOCCA_MAX_PLANKS || h->model.lookbehind < 1 || h->model.lookbehind > 2))
    return c.say("Stepper blob: n_planks must be 1..4 and lookbehind 1 or 2");
  hipError_t e;
  DeviceGuard guard(device);  // the caller's current device is restored on return
  if ((e = guard.err) != hipSuccess) return c.hip("hipSetDevice", e);
  if ((e = h->d_model.alloc(1, false)) != hipSuccess) return c.hip("hipMalloc(model)", e);
  if ((e = hipMemcpy(h->d_model, &h->model, sizeof(MoccaModel), hipMemcpyHostToDevice)) != hipSuccess) return c.hip("hipMemcpy(model)", e);
  const size_t n = (size_t)n_envs;
  if ((e = h->d_dyn.alloc(n * DYN_STRIDE, false)) != hipSuccess) return c.hip("hipMalloc(state)", e);
  if ((e = h->d_task.alloc(n * MOCCA_TASK_WORDS, false)) != hipSuccess) return c.hip("hipMalloc(task)", e);
  if ((e = h->d_terrain.alloc(n * TERRAIN_STRIDE, true)) != hipSuccess) return c.hip("hipMalloc(terrain)", e);
  if ((e = h->d_pace_acc.alloc(1, true)) != hipSuccess) return c.hip("hipMalloc(pace samples)", e);
  // task records: episode = -1 so the first reset is episode 0; applied_gain = 1
  {
    std::vector<uint32_t> tmp(n * MOCCA_TASK_WORDS);
    const float one = 1.0f;
    uint32_t one_bits; std::memcpy(&one_bits, &one, 4);
    for (size_t i = 0; i < n; ++i) {
      tmp[i * MOCCA_TASK_WORDS + MOCCA_TW_EPISODE] = (uint32_t)-1;
      tmp[i * MOCCA_TASK_WORDS + MOCCA_TW_APPLIED_GAIN] = one_bits;
    }
    if ((e = hipMemcpy(h->d_task, tmp.data(), tmp.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return c.hip("hipMemcpy(task)", e);
  }
  // identity quaternion so an un-reset env is still a valid state
  {
    std::vector<float> tmp(n * DYN_STRIDE);
    for (size_t i = 0; i < n; ++i) tmp[i * DYN_STRIDE + 6] = 1.0f;
    if ((e = hipMemcpy(h->d_dyn, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return c.hip("hipMemcpy(state)", e);
  }
  *out = h.release();
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(nullptr, "mocca_create")); }

int mocca_destroy(mocca_handle h) {
  delete h;   // its DevBufs free the device memory
  return MOCCA_OK;
}

int mocca_n_envs(mocca_handle h) { return h ? h->n_envs : Call(h, "mocca_n_envs").null_handle(); }
int mocca_obs_dim(mocca_handle h) { return h ? h->obs_dim : Call(h, "mocca_obs_dim").null_handle(); }
int mocca_act_dim(mocca_handle h) {
  if (!h) return Call(h, "mocca_act_dim").null_handle();
  return h->task_id == MOCCA_TASK_CASSIE ? h->model.n_ctrl - 2 : h->model.n_joints;
}
int mocca_plan_dim(mocca_handle h) {
  ENTRY(h, "mocca_plan_dim");
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return c.bad("only the planner task takes plans");
  return mocca_ctrl::CTRL_PLAN;
}
int mocca_state_dim(mocca_handle h) { return h ? MOCCA_STATE_DIM(h->model.n_joints, h->model.n_slots) : Call(h, "mocca_state_dim").null_handle(); }

int mocca_step(mocca_handle h, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev,
               void* stream) {
  ENTRY(h, "mocca_step");
  if (!act_dev || !obs_dev || !rew_dev || !done_dev) return c.null_arg("act_dev, obs_dev, rew_dev and done_dev");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  return launch_step(c, act_dev, nullptr, obs_dev, rew_dev, done_dev, info_dev, (hipStream_t)stream);
}

int mocca_task_step(mocca_handle h, const float* act_dev, const int32_t* touch_dev, const int32_t* target_dev, const int32_t* body_dev,
                    float* obs_dev, float* rew_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  ENTRY(h, "mocca_task_step");
  if (!act_dev || !obs_dev || !rew_dev || !done_dev) return c.null_arg("act_dev, obs_dev, rew_dev and done_dev");
  if (!touch_dev && h->task_id != MOCCA_TASK_CASSIE) return c.say("mocca_task_step needs the foot contact flags");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.act = act_dev; a.obs = obs_dev; a.rew = rew_dev; a.done = done_dev; a.info = info_dev;
  a.inj_touch = touch_dev; a.inj_target = target_dev; a.inj_body = body_dev;
  a.tape = h->tape; a.tape_n = h->tape_n;
  a.dbg = nullptr;
  if (int rc = flush_pending(c, (hipStream_t)stream)) return rc;
  launch_task_step(h->topo, h->task_id, h->n_envs, (hipStream_t)stream, a);
  return c.launched();
}

int mocca_set_draw_tape(mocca_handle h, const float* tape_dev, int n_per_env) {
  ENTRY(h, "mocca_set_draw_tape");
  if (tape_dev && n_per_env <= 0) return c.bad("n_per_env must be positive with a tape");
  h->tape = tape_dev; h->tape_n = tape_dev ? n_per_env : 0;
  return MOCCA_OK;
}

int mocca_set_debug_buffer(mocca_handle h, int32_t* dbg_dev) {
  ENTRY(h, "mocca_set_debug_buffer");
  h->dbg = dbg_dev;
  return MOCCA_OK;
}

int mocca_set_terminal_obs_buffer(mocca_handle h, float* final_obs_dev) {
  ENTRY(h, "mocca_set_terminal_obs_buffer");
  h->final_obs = final_obs_dev;
  return MOCCA_OK;
}

int mocca_set_episode_stats(mocca_handle h, float* masks_dev, float* bad_masks_dev, float* totals_dev, void* records, int n_slots,
                            size_t slot_stride_bytes) {
  ENTRY(h, "mocca_set_episode_stats");
  const bool on = masks_dev || bad_masks_dev || totals_dev || records;
  if (records && (n_slots < 1 || slot_stride_bytes < (size_t)h->n_envs * sizeof(mocca_episode_rec) || ((uintptr_t)records & 15u) || (slot_stride_bytes & 15u))) {
    return c.say("episode records: n_slots >= 1 slots of n_envs 16-byte records, 16-byte aligned, slot_stride_bytes >= 16 n_envs");
  }
  DeviceGuard guard(h->device);
  if (on && !h->d_ep_ret) {
    HIP_TRY(c, h->d_ep_ret.alloc((size_t)h->n_envs, true));
  } else if (!on && h->d_ep_ret) {
    HIP_TRY(c, hipDeviceSynchronize());   // a launch in flight may still add to it
    h->d_ep_ret.reset();
  }
  h->ep_masks = masks_dev; h->ep_bad = bad_masks_dev; h->ep_totals = totals_dev;
  h->ep_rec = (char*)records; h->ep_slots = records ? n_slots : 0; h->ep_stride = records ? slot_stride_bytes : 0;
  return MOCCA_OK;
}
uint32_t mocca_episode_serial(mocca_handle h) { return h ? h->ep_serial : 0u; }

int mocca_set_seed(mocca_handle h, uint64_t seed) {
  ENTRY(h, "mocca_set_seed");
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
  ENTRY(h, "mocca_set_trajectory");
  if (!table_host || n_frames <= 0 || !(max_time > 0.0) || !(control_step > 0.0)) return c.bad("empty table or non-positive times");
  DeviceGuard guard(h->device);
  const size_t floats = (size_t)n_frames * MOCCA_TRAJ_STRIDE;
  DevBuf<float> traj;
  hipError_t e = traj.alloc(floats, false);
  if (e == hipSuccess) e = hipMemcpy(traj, table_host, floats * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(c, e)) return rc;
  h->d_traj.swap(traj);
  h->traj_n = n_frames; h->traj_tmax = max_time; h->traj_cstep = control_step;
  return MOCCA_OK;
}

int mocca_observe(mocca_handle h, float* obs_dev, void* stream) {
  ENTRY(h, "mocca_observe");
  if (!obs_dev) return c.null_arg("obs_dev");
  if (need_attachments(c) != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  StepArgs a = make_args(h);
  a.obs = obs_dev;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = flush_pending(c, s)) return rc;
  dispatch<LaunchObserve>(h->topo, h->task_id, h->n_envs, s, a);
  return c.launched();
}

int mocca_get_state(mocca_handle h, float* state_dev, void* stream) {
  ENTRY(h, "mocca_get_state");
  if (!state_dev) return c.null_arg("state_dev");
  DeviceGuard guard(h->device);
  const size_t w = (size_t)mocca_state_dim(h) * sizeof(float);
  HIP_TRY(c, hipMemcpy2DAsync(state_dev, w, h->d_dyn, DYN_STRIDE * sizeof(float), w, h->n_envs, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_state(mocca_handle h, const float* state_dev, void* stream) {
  ENTRY(h, "mocca_set_state");
  if (!state_dev) return c.null_arg("state_dev");
  DeviceGuard guard(h->device);
  const size_t w = (size_t)mocca_state_dim(h) * sizeof(float);
  HIP_TRY(c, hipMemcpy2DAsync(h->d_dyn, DYN_STRIDE * sizeof(float), state_dev, w, w, h->n_envs, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_get_task(mocca_handle h, uint32_t* task_dev, void* stream) {
  ENTRY(h, "mocca_get_task");
  if (!task_dev) return c.null_arg("task_dev");
  DeviceGuard guard(h->device);
  if (int rc = flush_pending(c, (hipStream_t)stream)) return rc;
  HIP_TRY(c, hipMemcpyAsync(task_dev, h->d_task, (size_t)h->n_envs * MOCCA_TASK_WORDS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_task(mocca_handle h, const uint32_t* task_dev, void* stream) {
  ENTRY(h, "mocca_set_task");
  if (!task_dev) return c.null_arg("task_dev");
  DeviceGuard guard(h->device);
  // a restored snapshot wins over an earlier scalar applied_gain: every env's MOCCA_TW_APPLIED_GAIN is the snapshot's; the handle's own copy (what a
  // Custom env's reset writes, robot.applied_gain persists across resets) keeps the value of the last mocca_set_param
  h->gain_pending = false;
  HIP_TRY(c, hipMemcpyAsync(h->d_task, task_dev, (size_t)h->n_envs * MOCCA_TASK_WORDS * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_get_terrain(mocca_handle h, float* terrain_dev, void* stream) {
  ENTRY(h, "mocca_get_terrain");
  if (!terrain_dev) return c.null_arg("terrain_dev");
  DeviceGuard guard(h->device);
  HIP_TRY(c, hipMemcpyAsync(terrain_dev, h->d_terrain, (size_t)h->n_envs * TERRAIN_STRIDE * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}
int mocca_set_terrain(mocca_handle h, const float* terrain_dev, void* stream) {
  ENTRY(h, "mocca_set_terrain");
  if (!terrain_dev) return c.null_arg("terrain_dev");
  DeviceGuard guard(h->device);
  HIP_TRY(c, hipMemcpyAsync(h->d_terrain, terrain_dev, (size_t)h->n_envs * TERRAIN_STRIDE * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_param(mocca_handle h, int param_id, double value) {
  ENTRY(h, "mocca_set_param");
  switch (param_id) {
    case MOCCA_PARAM_AUTO_RESET: h->auto_reset = value != 0; break;
    case MOCCA_PARAM_EVAL_MODE: h->eval_mode = value != 0; h->pvec_on[1] = false; break;
    case MOCCA_PARAM_CURRICULUM:
      if (h->cur_on)
        return c.bad("the scalar MOCCA_PARAM_CURRICULUM would drop the level vector of the attached curriculum: use mocca_set_param_v with broadcast");
      h->curriculum = (int)value < 0 ? 0 : ((int)value > 9 ? 9 : (int)value); h->pvec_on[0] = false; break;
    case MOCCA_PARAM_APPLIED_GAIN:  // acts on the next apply_action: the task records carry the value the kernel uses; this call has no
      h->gain = (float)value; h->pvec_on[2] = false; h->gain_pending = true;   // stream, so the write is enqueued by the next call that has
      break;                                                                    // one (flush_pending), ordered on the caller's stream
    case MOCCA_PARAM_RANDOM_POSE: h->random_pose = value != 0; break;
    case MOCCA_PARAM_HOST_RETARGET: h->host_retarget = value != 0; break;
    case MOCCA_PARAM_SEED: h->seed = (uint64_t)value; break;
    case MOCCA_PARAM_ENV_OFFSET: h->env_offset = (int)value; break;
    case MOCCA_PARAM_ISSUE_PRIORITY:
      if (value < 0 || value >= 262144) return c.say("MOCCA_PARAM_ISSUE_PRIORITY is t1 + 64 t2 + 4096 t3 with each threshold in 0..63");
      h->prio = (int)value;
      break;
    case MOCCA_PARAM_RANDOM_REWARD:
      if (value != 0 && value != 1 && value != 2) return c.say("MOCCA_PARAM_RANDOM_REWARD is 0, 1 or 2");
      h->random_reward = (int)value; break;
    case MOCCA_PARAM_PERSIST_IMPULSES: h->persist_warm = value != 0; break;
    case MOCCA_PARAM_PACE_TICKS:
      if (value < -64 || value > 1e9) return c.say("MOCCA_PARAM_PACE_TICKS is a tick count > 0, 0 (off) or -k (self-calibrating, k / 16 of the mean wave time, k <= 64)");
      h->pace = (int)value; break;
    case MOCCA_PARAM_ORDER_EVERY:
      if (value < 0 || value > 1e6) return c.say("MOCCA_PARAM_ORDER_EVERY is a step count >= 0");
      h->order_every = (int)value; h->order_age = h->order_every;
      if (h->order_every > 0 && !h->d_order) {   // (allocated here, not in mocca_step)
        DeviceGuard guard(h->device);
        HIP_TRY(c, h->d_order.alloc((size_t)h->n_envs, false));
      }
      break;
    case MOCCA_PARAM_KERNEL_VARIANT: {
      if (value != (double)(int)value || value < 0 || value > 7 || ((int)value & 3) == 3) return c.say("MOCCA_PARAM_KERNEL_VARIANT is 0 (automatic), 1 (force the 48-row instance) or 2 (force the 64-row instance), plus 4 to build the Delassus matrix on the VALU");
      const int inst = (int)value & 3;
      if (inst == 1 && h->wide) return c.say("MOCCA_PARAM_KERNEL_VARIANT = 1: this blob needs the 64-row instance (caps beyond 48 rows / 12 contacts, or sweep_alternate)");
      h->force_full = inst; h->delassus_valu = ((int)value & 4) != 0; break;
    }
    default: return c.say("unknown parameter id");
  }
  return MOCCA_OK;
}

int mocca_set_param_v(mocca_handle h, int param_id, const float* values_dev, int broadcast, void* stream) {
  ENTRY(h, "mocca_set_param_v");
  if (!values_dev) return c.null_arg("values_dev");
  const int slot = param_id == MOCCA_PARAM_CURRICULUM ? 0 : param_id == MOCCA_PARAM_EVAL_MODE ? 1 : param_id == MOCCA_PARAM_APPLIED_GAIN ? 2 : -1;
  if (slot < 0) return c.say("this parameter has no per-env form");
  DeviceGuard guard(h->device);
  if (!h->d_pvec[slot]) HIP_TRY(c, h->d_pvec[slot].alloc((size_t)h->n_envs, false));
  hipStream_t s = (hipStream_t)stream;
  launch_per_env(copy_param_kernel, h, s, h->d_pvec[slot], values_dev, broadcast != 0, h->n_envs);
  HIP_TRY(c, hipGetLastError());
  if (slot == 2) {  // applied_gain acts at once (robots.py:33)
    // the per-env values supersede a scalar mocca_set_param(APPLIED_GAIN) that was not flushed yet: left pending, the next call with a
    // stream would overwrite every env's word with the stale scalar (call order must win, as it did when the scalar write was synchronous)
    h->gain_pending = false;
    launch_per_env(set_task_word_kernel, h, s, h->d_task, MOCCA_TW_APPLIED_GAIN, h->d_pvec[slot], 0.0f, 0, h->n_envs);
    HIP_TRY(c, hipGetLastError());
  }
  h->pvec_on[slot] = true;
  return MOCCA_OK;
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
  ENTRY(h, "mocca_kernel_info");
  hipFuncAttributes fa;
  int nb = 0;
  hipError_t e = hipSuccess;
  switch (step_instance(h)) {
    case INST_COMPACT: mocca_r32_kernel_info(h->topo, h->task_id, &fa, &nb, &e); break;
    case INST_WIDE: mocca_r64_kernel_info(h->topo, h->task_id, &fa, &nb, &e); break;
    default: dispatch<KernelInfo>(h->topo, h->task_id, &fa, &nb, &e);
  }
  HIP_TRY(c, e);
  if (vgprs) *vgprs = fa.numRegs;
  if (sgprs) *sgprs = -1;   // hipFuncAttributes has no scalar-register field: -1 = not reported (the count is in the code object's metadata: build.py -v prints it)
  if (lds_bytes) *lds_bytes = (int)fa.sharedSizeBytes;
  if (scratch_bytes) *scratch_bytes = (int)fa.localSizeBytes;
  if (max_blocks_per_cu) *max_blocks_per_cu = nb;
  return MOCCA_OK;
}

}  // extern "C"
