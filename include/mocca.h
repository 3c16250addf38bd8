/*
 * mocca.h -- C ABI of libmocca_hip.so, the MI355X-native replacement for the
 * pybullet client the reference env owns (`EnvBase._p`,
 * /root/reference/mocca_envs/env_base.py:55) and for everything the reference
 * does through it on the env.step()/reset() path.
 *
 * There is no FFI seam in the reference (it is pure Python over the pybullet
 * CPython extension); the seam is introduced here, at the `_p` object.  Each
 * entry point cites the reference calls it stands in for.
 *
 * Conventions
 *   - every pointer named *_dev is device memory of the GPU the handle was
 *     created on (e.g. torch tensor .data_ptr()); tensors are caller-owned,
 *     contiguous, row-major [n_envs][dim].
 *   - `stream` is a hipStream_t passed as void*; work is enqueued
 *     asynchronously, no call synchronises the device except the *_host
 *     helpers and mocca_create/mocca_destroy.
 *   - return 0 on success, negative MOCCA_E_* otherwise; the message is
 *     available from mocca_last_error().  Nothing throws across the ABI.
 *   - a non-finite state is NOT an error: it sets done, as the reference does
 *     (env_locomotion.py:205-207).
 *   - a handle is not thread-safe; use one handle per (process, device).
 */
#ifndef MOCCA_H
#define MOCCA_H

#include <stddef.h>
#include <stdint.h>

#include "mocca_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MOCCA_ABI_VERSION 8

typedef struct mocca_ctx *mocca_handle;

enum {
  MOCCA_OK = 0,
  MOCCA_E_ARG = -1,      /* bad argument / blob */
  MOCCA_E_HIP = -2,      /* HIP runtime error */
  MOCCA_E_TOPOLOGY = -3, /* blob topology differs from the compiled kernel's */
  MOCCA_E_NODEVICE = -4,
};

/* mocca_set_param ids */
enum {
  MOCCA_PARAM_AUTO_RESET = 0,  /* vec-env semantics: a done env is reset inside step() and returns the reset obs */
  MOCCA_PARAM_EVAL_MODE = 1,   /* Walker3DCustomEnv.evaluation_mode(), env_locomotion.py:76-77 */
  MOCCA_PARAM_CURRICULUM = 2,  /* set_env_params({"curriculum": k}), env_base.py:103-106 (takes effect at reset) */
  MOCCA_PARAM_RANDOM_POSE = 3, /* robot_random_start, env_locomotion.py:45 */
  MOCCA_PARAM_HOST_RETARGET = 4, /* Custom env: leave close_count >= stop_frames for the host to re-randomise the
                                    target (env_locomotion.py:214-222) with ITS RandomState, as the facade does */
  MOCCA_PARAM_SEED = 5,        /* Philox key used by step() for in-kernel draws (also set by mocca_reset) */
  MOCCA_PARAM_ENV_OFFSET = 6,  /* global index of this handle's env 0: draws are keyed by (seed, offset + env, episode),
                                  so a shard of a larger batch reproduces exactly the envs it owns */
  MOCCA_PARAM_RANDOM_REWARD = 8, /* Walker3DStepperEnv(random_reward=True), env_locomotion.py:533-547: the 8 reward terms are weighted by
                                    U(0.8, 1.2) numbers drawn every step.  1: drawn in the kernel (8 draws per step); 2: supplied by
                                    the host in task words 30..37 before each step (the single-env classes: np_random stays on the host) */
  MOCCA_PARAM_APPLIED_GAIN = 7, /* set_robot_params({"applied_gain": g}), env_base.py:108-115 / robots.py:16,33: acts on the
                                   next apply_action; the Stepper overwrites it at reset from its curriculum (:489).  The scalar form has
                                   no stream argument: the value is written into the task records by the next call that takes a stream,
                                   on that stream.  A later mocca_set_task restores the snapshot's per-env gains (word 21); the handle's
                                   own copy -- what a Custom env's reset writes -- stays at the last value set here */
  MOCCA_PARAM_ISSUE_PRIORITY = 9, /* TIMING ONLY (no reference counterpart, results do not depend on it): constraint-row counts above which a
                                     wave runs at issue priority 1 / 2 / 3 in the step kernel, packed t1 + 64 t2 + 4096 t3 (each 0..63).
                                     A launch lasts as long as its slowest wave and an env's cost grows with its rows, so the best
                                     thresholds follow the batch's row distribution; default 4 / 7 / 12 (flat-ground walker, blob v13 physics) */
  MOCCA_PARAM_PERSIST_IMPULSES = 10, /* no reference counterpart.  Words 13 + 2 n_joints .. of the state record (mocca_get_state) hold the normal
                                        impulse of every terrain contact slot in the LAST substep.  A blob that warm-starts its contact rows
                                        (MoccaModel.warmstart != 0) reads and writes them every step; the compiled blobs do not (Bullet does not
                                        warm start multibody contacts), and then mocca_step neither loads nor stores them -- 272 B per env-step of
                                        dead traffic until ABI 4 -- unless this parameter is 1 (tests and tools that want the impulses as a
                                        diagnostic).  Results do not depend on it. */
  MOCCA_PARAM_KERNEL_VARIANT = 11,   /* TIMING ONLY.  mocca_create picks the step-kernel instance from the blob: max_rows <= 32 and
                                        max_contacts <= 10 on a tree without loop closures run the COMPACT instance (32 x 32 Delassus matrix,
                                        the articulated-body view aliased under it: less LDS per env, more resident waves per CU); every other
                                        blob within 48 rows / 12 contacts the 48-row instance; a blob whose caps exceed those (max_rows <= 64,
                                        max_contacts <= 20) or that sets MoccaModel.sweep_alternate the 64-row ACCURACY instance (every lane of the wave a row; 17 KB of LDS per env and
                                        a two-waves-per-SIMD register budget: Bullet caps neither rows nor contacts, and this instance exists to
                                        measure what the product's caps change).  1 forces the 48-row instance for a blob that would run the
                                        compact one, 2 forces the 64-row instance for any blob (A/B runs), 0 = automatic.  The instances execute
                                        the same arithmetic in the same order: on the same blob results are bit-identical.
                                        Bit 2 (add 4 to any of the above): the step kernel builds the Delassus matrix A = J X^T with the VALU
                                        dot products for every row count.  Without it a substep of a tree without loop closures that holds 8 to
                                        32 rows (8 to 16 in the compact instance; not the 48-row planner kernel) builds A with
                                        v_mfma_f32_16x16x4_f32, which evaluates the same fma chain in the same order: results are
                                        bit-identical with and without the bit (A/B runs).  Values: 0, 1, 2, 4, 5, 6. */
  MOCCA_PARAM_ORDER_EVERY = 12,      /* TIMING ONLY.  K > 0: every K-th mocca_step first sorts the envs by the constraint-row count their last step
                                        ended with and the step kernel starts the heaviest first (a launch of more envs than the chip holds at
                                        once ends with the waves it started last: they should be the light ones); 0: index order.  Envs never
                                        interact, so the order changes when an env runs, not what it computes. */
  MOCCA_PARAM_PACE_TICKS = 13,       /* TIMING ONLY.  PACE priorities instead of the row-count priorities above.  The hardware serves equal-priority
                                        waves of a SIMD oldest-first, so its four resident waves finish one after the other and the launch waits
                                        for the last, which runs alone.  With a pace P a wave compares the shader-clock ticks it has used with
                                        the share of the env.step it has done (64 units per substep + 2 per constraint row) and runs at issue
                                        priority 3 / 2 / 1 / 0 as its estimated finish lies beyond 17/16 of, beyond, within 1/16 below, or
                                        further below P: the waves of a SIMD finish together.  value > 0: P in ticks; value = -k (1 <= k <= 64):
                                        self-calibrating, P = k/16 of the mean wave time of the last 64 .. 128 sampled waves (one wave in 61 adds
                                        its time to a device-side accumulator; until the first sample a handle falls back to the row-count
                                        priorities); 0: off.  Default -18; 0 for a blob that runs the compact instance (batches beyond one generation of
                                        resident waves: measured slower with it).  Since ABI 7 the calibration keeps no host state: mocca_step can be
                                        captured in a hipGraph with any pace; only ORDER_EVERY > 0 and the episode-record ring (mocca_set_episode_stats)
                                        keep per-launch HOST state that a capture would freeze. */
};

/* words of the per-env debug record (mocca_set_debug_buffer): words 0..11 the active set of the LAST physics substep, words 12..15
 * cumulative over every substep since the caller last cleared the buffer, words 16..18 a signature of EVERY substep of the last mocca_step */
#define MOCCA_DEBUG_WORDS 20
enum {
  MOCCA_DBG_ROWS = 0,        /* constraint rows solved                                  */
  MOCCA_DBG_LIMIT_ROWS = 1,  /* of which joint-limit rows                               */
  MOCCA_DBG_CONTACTS = 2,    /* contacts kept (each gives 1 normal + 2 friction rows)   */
  MOCCA_DBG_SLOTS_LO = 3,    /* bit s: terrain contact slot s is within the margin      */
  MOCCA_DBG_SLOTS_HI = 4,
  MOCCA_DBG_LIMITS_LO = 5,   /* bit 2j + side: limit candidate of joint j (0 lower, 1 upper) */
  MOCCA_DBG_LIMITS_HI = 6,
  MOCCA_DBG_SELF = 7,        /* self-collision pairs within the margin                  */
  MOCCA_DBG_CLAMP_LO = 8,    /* bit l: the row on solver lane l ended the LAST PGS iteration on a bound (unilateral rows at 0, friction  */
  MOCCA_DBG_CLAMP_HI = 9,    /* rows at +-mu lambda_n).  Lanes: limit / closure / planar / normal rows 0.. in row order, friction rows */
                             /* of contact i on lanes 46 - 2i and 47 - 2i                                                               */
  MOCCA_DBG_CLAMPSIG_LO = 10, /* the same mask folded over ALL iterations: sig = rotl64(sig, 7) ^ mask -- every discrete decision the   */
  MOCCA_DBG_CLAMPSIG_HI = 11, /* solver took in the substep                                                                             */
  /* cap pressure (Bullet has neither cap), cumulative: */
  MOCCA_DBG_CAP_CONTACTS = 12, /* substeps in which more contacts were within the margin than max_contacts                             */
  MOCCA_DBG_CAP_ROWS = 13,     /* substeps in which limit + closure + 3 x (kept contacts) rows exceeded max_rows                        */
  MOCCA_DBG_SUBSTEPS = 14,     /* substeps counted                                                                                      */
  MOCCA_DBG_ROWS_WANTED = 15,  /* largest row count an uncapped solver would have held                                                  */
  /* every discrete decision of the last mocca_step, all its substeps (4; Cassie: 50): h = 0 at the step's start, then per substep and for
   * w = 0 .. 11:  h = (h ^ (uint32) word w) * 0x9E3779B97F4A7C15 (mod 2^64).  Two implementations that took the same decisions in every
   * substep agree on it: whole-step comparisons can then be held to arithmetic tolerances (tests/test_gpu_parity.py) */
  MOCCA_DBG_STEPSIG_LO = 16,
  MOCCA_DBG_STEPSIG_HI = 17,
  MOCCA_DBG_STEPSIG_N = 18,    /* substeps folded into it */
  MOCCA_DBG_RESERVED = 19,
};

int mocca_abi_version(void);
size_t mocca_model_sizeof(void);

/* EnvBase.initialize_scene_and_robot (env_base.py:49-101): BulletClient(DIRECT), scene + physics
 * parameters, loadMJCF / loadSDF / loadURDF.  `model_blob` is a MoccaModel; `task_id` a MOCCA_TASK_*. */
int mocca_create(const void *model_blob, size_t nbytes, int task_id, int n_envs, int device, mocca_handle *out);
/* EnvBase.close (env_base.py:44-47): disconnect. */
int mocca_destroy(mocca_handle h);

int mocca_n_envs(mocca_handle h);
int mocca_obs_dim(mocca_handle h);   /* 52 (Custom, env_locomotion.py:58; Planner, :1003-1005) / 65 (Stepper, :386-393) / 36 (CassieEnv) / 42 (CassiePhase*, env_cassie.py:633) */
int mocca_act_dim(mocca_handle h);   /* 21, robots.py:21-23 (the planner envs too: mocca_step takes the base controller's joint actions) */
int mocca_plan_dim(mocca_handle h);  /* planner task: 15 = (base_lookahead + base_lookbehind) x base_step_param_dim, env_locomotion.py:1006-1009; else MOCCA_E_ARG */
int mocca_state_dim(mocca_handle h); /* MOCCA_STATE_DIM */

/* env.reset() (env_locomotion.py:79-109 / :481-513) for every env whose mask byte is non-zero
 * (NULL = all).  Draws come from Philox keyed by (seed, env, episode).  obs_dev: [N][obs_dim] f32;
 * rows of unmasked envs are left untouched. */
int mocca_reset(mocca_handle h, const uint8_t *mask_dev, uint64_t seed, float *obs_dev, void *stream);

/* env.step(a) (env_locomotion.py:111-141 / :515-568): apply_action (robots.py:31-40) ->
 * stepSimulation (bullet_utils.py:352-353) -> calc_state (robots.py:42-95) -> reward/termination.
 *   act_dev  [N][act_dim] f32 (clipped to [-1,1] inside, robots.py:33)
 *   obs_dev  [N][obs_dim] f32, rew_dev [N] f32
 *   done_dev [N] u8: bit0 = terminated (self.done), bit1 = TimeLimit (max_episode_steps, __init__.py:55)
 *   info_dev [N] i32 or NULL: Stepper "steps_reached" (env_locomotion.py:562-566), 0 for Custom */
int mocca_step(mocca_handle h, const float *act_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev,
               int32_t *info_dev, void *stream);

/* The task layer of env.step(a) alone -- everything of env_locomotion.py:111-141 / :515-568 EXCEPT stepSimulation:
 * the stored dynamic state is taken as the post-physics state, and the contact queries the reference makes after
 * stepping (robots.py:74-86 feet_contact; calc_feet_state's target-plank test, env_locomotion.py:634-650;
 * LaikagoCustomEnv's body contacts, :880-890) are supplied by the caller.  Same kernel source as mocca_step with zero
 * substeps.  Used to replay the reference's own scripted episodes (tests/golden) through the HIP path.
 *   touch_dev  [N][n_feet] i32, target_dev [N][n_feet] i32 or NULL, body_dev [N] i32 or NULL; rest as mocca_step. */
int mocca_task_step(mocca_handle h, const float *act_dev, const int32_t *touch_dev, const int32_t *target_dev,
                    const int32_t *body_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev, int32_t *info_dev,
                    void *stream);

/* Replace the Philox draws of mocca_reset / mocca_task_step by uniforms read from tape_dev [N][n_per_env] f32, indexed
 * by the episode's draw counter (task word 10) -- the numbers `np_random` gave the reference in the recorded episode.
 * NULL detaches.  mocca_step (the physics path) never reads the tape.  The buffer must outlive its use. */
int mocca_set_draw_tape(mocca_handle h, const float *tape_dev, int n_per_env);

/* robot.calc_state() + the task's observation tail on the CURRENT state, without stepping
 * (robots.py:42-95 with env_locomotion.py:102-109 / :712-759).  Used after set_state/set_task, e.g. by the
 * single-env facade whose reset draws come from a host numpy RandomState like the reference's.
 * Updates the task record's potentials (calc_potential) and, for the Stepper, walk_target. */
int mocca_observe(mocca_handle h, float *obs_dev, void *stream);

/* In-memory snapshot of the simulation (the role of saveState/restoreState, env_base.py:101): dynamic
 * state [N][state_dim] f32, task record [N][MOCCA_TASK_WORDS] 32-bit words, terrain [N][128] f32
 * (Stepper: 20 rows x 6 then the n_planks (3 or 4) live plank rows as floats). Device pointers. */
int mocca_get_state(mocca_handle h, float *state_dev, void *stream);
int mocca_set_state(mocca_handle h, const float *state_dev, void *stream);
int mocca_get_task(mocca_handle h, uint32_t *task_dev, void *stream);
int mocca_set_task(mocca_handle h, const uint32_t *task_dev, void *stream);
int mocca_get_terrain(mocca_handle h, float *terrain_dev, void *stream);
int mocca_set_terrain(mocca_handle h, const float *terrain_dev, void *stream);

/* set_env_params / evaluation_mode / auto-reset switch (see MOCCA_PARAM_*) */
int mocca_set_param(mocca_handle h, int param_id, double value);
/* Per-env form for MOCCA_PARAM_CURRICULUM / _EVAL_MODE / _APPLIED_GAIN (each env of the reference owns its own
 * attributes, env_base.py:103-115): values_dev [N] f32 is COPIED into the handle; broadcast != 0 reads values_dev[0]
 * for every env.  A later scalar mocca_set_param of the same id drops the vector (MOCCA_PARAM_CURRICULUM's is refused while a
 * curriculum is attached, mocca_set_curriculum). */
int mocca_set_param_v(mocca_handle h, int param_id, const float *values_dev, int broadcast, void *stream);
/* full 64-bit Philox key (MOCCA_PARAM_SEED travels through a double: exact below 2^53 only) */
int mocca_set_seed(mocca_handle h, uint64_t seed);
/* dbg_dev [N][MOCCA_DEBUG_WORDS] i32 receives the active set of each env's last substep on every mocca_step; NULL stops it */
int mocca_set_debug_buffer(mocca_handle h, int32_t *dbg_dev);
/* Terminal observations under MOCCA_PARAM_AUTO_RESET.  The reference's step() returns the observation of the FINAL state together with
 * done (env_locomotion.py:128-141), and so does gym's TimeLimit wrapper on truncation (__init__.py:55); with auto-reset mocca_step's
 * obs_dev row of a finished env already holds the first observation of its next episode.  final_obs_dev [N][obs_dim] f32 (caller-owned,
 * NULL detaches): on every mocca_step the row of each env whose done byte is non-zero receives that final observation -- bit-identical
 * to what the same step returns with auto-reset off; rows of the other envs are left untouched. */
int mocca_set_terminal_obs_buffer(mocca_handle h, float *final_obs_dev);
/* Monitor + TimeLimitMask + the PPO loop's mask columns, inside the launch.  The reference's trainers (README.md:33-39) wrap every env in
 * baselines' Monitor (info["episode"] = {"r": return, "l": length} in the step that ends an episode) and a TimeLimitMask
 * (info["bad_transition"] when gym's TimeLimit, /root/reference/mocca_envs/__init__.py:55, cut the episode), then build `masks` / `bad_masks`
 * from `done` / `infos` on the host.  With any of the four pointers non-NULL every mocca_step also, per env (the handle keeps the running
 * return itself; mocca_reset zeroes it for the envs it resets):
 *   masks_dev     [N] f32 or NULL: 0.0 where done != 0 in this step, else 1.0
 *   bad_masks_dev [N] f32 or NULL: 0.0 where the TimeLimit bit of done is set, else 1.0
 *   totals_dev    [4] f32 or NULL: += {return, length, 1, TimeLimit bit} of every episode that ends (atomics; the caller zeroes it when it likes)
 *   records       NULL, or a ring of n_slots slots, slot_stride_bytes apart, of [N] mocca_episode_rec in DEVICE-VISIBLE memory -- device memory or
 *                 pinned host memory (hipHostMalloc / torch pin_memory: the kernel then writes the few records of a step straight into the
 *                 host's memory and nothing is copied).  The k-th mocca_step after this call (k = 1, 2, ...; mocca_episode_serial() returns
 *                 the NEXT k) writes slot k mod n_slots: record i only if env i finished in that step, with serial = k -- a record whose
 *                 serial differs is left over from n_slots steps ago.  The caller reads a slot once the step's stream work has completed.
 * All NULL detaches (synchronises the device).  The slot / serial are host state of the handle: under hipGraph replay they stay frozen,
 * masks and totals do not. */
typedef struct mocca_episode_rec {
  uint32_t serial; /* which mocca_step wrote it */
  float ret;       /* Monitor's r: sum of the episode's rewards (f32) */
  int32_t length;  /* Monitor's l: steps */
  uint32_t flags;  /* bits 0..1 the step's done byte (bit1: TimeLimit -> "bad_transition"), bits 8.. the step's info word (Stepper: steps_reached) */
} mocca_episode_rec;
int mocca_set_episode_stats(mocca_handle h, float *masks_dev, float *bad_masks_dev, float *totals_dev, void *records, int n_slots,
                            size_t slot_stride_bytes);
uint32_t mocca_episode_serial(mocca_handle h);

/* 1 if the library was compiled with a profiling switch that makes results wrong or slow by construction
 * (MOCCA_SKIP_*, MOCCA_DUMMY_VALU, MOCCA_STAMPS); the Python binding refuses such a build unless told otherwise */
int mocca_is_diagnostic_build(void);

/* The reference motion of the Cassie mocap / phase envs: what `self.traj = CassieTrajectory()` (env_cassie.py:576) holds and
 * `base_angles / base_velocities / resetJoints / get_obs` (:589-605,636-642) read through joint_angles(t), joint_speeds(t),
 * rod_joint_angles(t), max_time().  table_host [n_frames][MOCCA_TRAJ_STRIDE] f32 (HOST memory, copied into the handle):
 * 14 joint angles in ordered-joint order, 14 joint speeds, 4 rod angles (right z, right y, left z, left y).  A time t maps to
 * frame int((t mod max_time) / max_time * n_frames); t = istep * control_step / n_llc (mocap_time, :359-360), evaluated in
 * double precision.  Required before reset / step when the blob's cassie_mode != MOCCA_CASSIE_PLAIN. */
int mocca_set_trajectory(mocca_handle h, const float *table_host, int n_frames, double max_time, double control_step);

/* The terrain of the planner envs: what `self.terrain = HeightField(...); self.terrain.reload(data=filename)` builds
 * (env_locomotion.py:1011-1021, bullet_objects.py:338-393: createCollisionShape(GEOM_HEIGHTFIELD, meshScale [1/scale, 1/scale, 1]), body at
 * z = (max + min) / 2, lateralFriction 1, contactStiffness 30000, contactDamping 1000 -- the last three are blob numbers).
 * heights_host [rows][cols] f32 (HOST memory, copied into the handle; x runs along the columns), `scale` grid points per metre.  The grid is
 * centred on the origin, every cell two triangles split from (ix + 1, iy) to (ix, iy + 1); a sphere / capsule end collides with the closest
 * triangle among the 2 W x 2 W cells around the grid point nearest to its centre, W = ceil((radius + contact margin) x scale + 1/2) -- every
 * cell it can reach (W = 1 for feet and limbs at 4 points per metre, 2 for the walker's 14 cm pelvis and Mike's 23 cm waist sphere, mike.xml:20,
 * whose contact ends MikePlannerEnv's episode; a grid on which a sphere would span more than 4 cells each way is refused);
 * outside the grid there is no ground.  By default one grid is shared by all envs of the handle
 * (the reference loads the same file for every env): this call is mocca_set_heightfield_bank with n_fields = 1.
 * A grid is required before reset / step / observe with MOCCA_TASK_WALKER3D_PLANNER. */
int mocca_set_heightfield(mocca_handle h, const float *heights_host, int rows, int cols, double scale);

/* The terrain BANK of the planner envs: n_fields height fields of one shape in device memory, every env standing on one of them -- what
 * `HeightField.reload(data=None)` (bullet_objects.py:355-441) gives one env at a time, a fresh random terrain, for a whole batch.  Physics,
 * the reset's target height, mocca_height_scan and mocca_render read the env's OWN field.
 *   mocca_set_heightfield_bank: heights_host [n_fields][rows][cols] f32 (HOST memory, copied), or NULL for a bank of zeros to be generated into;
 *     n_fields 1 .. MOCCA_HF_MAX_FIELDS.  The checks of mocca_set_heightfield (at least 2 x 2, positive scale, a grid that is not too fine
 *     for the robot); waits for the launches in flight; planner task only.  The range [zmin, zmax] of every field is kept on the device beside
 *     the bank (the ray caster clips to it).  Every env is put on field 0 and redraw-at-reset is switched off.  NULL with n_fields == 0 detaches.
 *   mocca_generate_heightfields: fills fields first .. first + count - 1 with the reference's generator (get_random_height_field,
 *     bullet_objects.py:395-441: n_peaks super-Gaussian peaks / scale + Perlin noise of 4 x 4 and 8 x 8 lattice cells, minus the mean of the
 *     5 x 5 corner platform the robot starts over, which is flattened to exactly 0) in f32, times `gain` (finite, > 0: the difficulty knob),
 *     and writes their ranges.  Asynchronous on `stream`: no allocation, no host read, no atomics -- the caller orders it against the step
 *     launches on the same stream.  n_peaks 1 .. MOCCA_HF_MAX_PEAKS; rows and cols must be multiples of 8 (the lattices divide them).
 *     The draws: uniform (w >> 8) 2^-24 of word d & 3 of philox4x32(d >> 2, block, field index in the bank, 3, seed low, seed high).  Block 0,
 *     d = 256 a + k: parameter k of array a, in the reference's order -- height 0.1 + 2.9 u, centre along the first axis and along the
 *     second (-half + 2 half u, half = size / scale / 2), the two spreads 1 + 15 u, the two exponents 2 (1 + int(5 u)); the stride is 256
 *     whatever n_peaks is, so fewer peaks are a prefix.  Block 1, d = 0 .. 24: the gradient angles 2 pi u of the 5 x 5 lattice, row-major; block
 *     2, d = 0 .. 80: those of the 9 x 9 lattice.  The first grid axis is the ROW index (the reference's quirk).  The field's index in the bank
 *     keys it: every handle that generates the same bank with the same seed holds the same fields.
 *   mocca_set_env_fields: field_dev int32 [n_envs] (DEVICE memory), the field of every env; NULL puts all envs on field 0.  The values are
 *     checked against the bank on the host after waiting for `stream` (it may synchronise, as mocca_render does for its env ids).
 *     redraw_at_reset != 0: every reset of env e -- mocca_reset and the auto-reset inside mocca_step / mocca_plan_step / mocca_act_plan_step --
 *     first draws field = (uint64(w) * n_fields) >> 32, w = word 0 of philox4x32(0, episode, global env id, 2, seed low, seed high) with the
 *     reset's seed, BEFORE the walk target's height is looked up.  Counter word 3 = 2 is a domain of its own and the episode's draw counter
 *     is not touched: every other draw keeps its value.  The index lives in an array of the handle, not in the task record: a snapshot of a
 *     bank run is state + task + env fields.
 *   mocca_get_env_fields / mocca_get_heightfields: the readbacks, asynchronous on `stream`: int32 [n_envs], f32 [count][rows][cols]
 *     (DEVICE memory).
 * MOCCA_E_ARG, the handle unchanged: not the planner task, n_fields outside its range, no bank attached, first / count outside the bank,
 * rows or cols no multiple of 8 (generate), n_peaks outside 1 .. 256, a gain that is not finite and positive, an env field outside the bank. */
#define MOCCA_HF_MAX_FIELDS 1024
#define MOCCA_HF_MAX_PEAKS 256
int mocca_set_heightfield_bank(mocca_handle h, const float *heights_host, int n_fields, int rows, int cols, double scale);
int mocca_generate_heightfields(mocca_handle h, int first, int count, uint64_t seed, int n_peaks, double gain, void *stream);
int mocca_set_env_fields(mocca_handle h, const int32_t *field_dev, int redraw_at_reset, void *stream);
int mocca_get_env_fields(mocca_handle h, int32_t *field_dev, void *stream);
int mocca_get_heightfields(mocca_handle h, int first, int count, float *out_dev, void *stream);

/* The base controller of the planner envs (env_locomotion.py:1029-1040): the agent's action is a 15-number plan; inside step() an actor-critic
 * pair of MLPs turns [robot_state(50), plan x action_scale] (65 floats, :1093) into the 21 joint actions, and the critic's value is part of the
 * reward, progress + log(max(1, value)) / 3 (:1101).  params_host [n_floats] f32 and layers_host [n_layers_total][8] i32 (HOST memory): the
 * actor's layers first (input to head), then the critic's; each row {net 0 / 1, in, out, in rounded up to a multiple of 16, out rounded up
 * likewise, activation (0 identity, 1 relu, 2 tanh, 3 softsign), offset of W[out][in] (row-major) in params_host, offset of b[out]}.  The
 * library pads the layers with zeros to the matrix cores' 16 x 16 tile and keeps them in the kernel's own order
 * (mocca_envs_amd/csrc/mocca_controller.h).  At most 8 layers per net, widths <= 256, hidden widths multiples of 16, 65 in, 21 / 1 out; every
 * dimension and offset is checked (MOCCA_E_ARG with a message).  Only for MOCCA_TASK_WALKER3D_PLANNER.  params_host == NULL detaches.
 * Synchronises the device.
 * While a controller is attached, every mocca_reset / mocca_step / mocca_task_step / mocca_observe also keeps the first 50 floats of the
 * observation it produced (`self.robot_state`; under auto-reset the new episode's first observation) in a buffer of the handle, wherever
 * obs_dev pointed: the controller's next input.  It is defined from the first such call after attaching. */
int mocca_set_base_controller(mocca_handle h, const float *params_host, size_t n_floats, const int32_t *layers_host, int n_layers_total,
                              double action_scale);
/* Observation statistics for the attached controller: what a controller trained by this project's own PPO on a Stepper id carries (the
 * policy kernel normalises its input, mocca_set_policy above all nets; bare layers cannot express the clamp).  mean_host and inv_std_host:
 * f32 [65] in HOST memory, copied into the handle; they apply to the controller's whole input row [robot_state(50), plan(15) x action_scale],
 * after the scale and before both nets, entry k < 65 by the policy kernel's line in its order of operations,
 * v = fminf(fmaxf((v - mean[k]) * inv_std[k], -clip), clip) (inv_std = 1 / sqrt(var + eps), formed by the caller in f32); the padding
 * columns and the rows past the batch stay exact zeros.  With nothing attached mocca_plan_step gives the bits it gave without this call.
 * Needs an attached controller.  mean_host == NULL (both NULL) detaches; mocca_set_base_controller drops the statistics on replace and on
 * detach, as mocca_set_policy drops its attachments.  May synchronise.  Errors (MOCCA_E_ARG with a message, the handle left as it was): a
 * NULL handle, no controller attached, exactly one of the two arrays NULL, a non-finite mean, an inv_std that is non-finite or negative, a
 * clip that is not finite and > 0. */
int mocca_set_base_controller_norm(mocca_handle h, const float *mean_host, const float *inv_std_host, double clip);
/* env.step(plan) of the planner envs: the controller kernel (one launch: both nets, all envs; f32 on the matrix cores), then the step kernel on
 * its joint actions, both on `stream`; the reward carries the value term -- rew_dev, and with it Monitor's returns, totals and records
 * (mocca_set_episode_stats).  plan_dev [N][15] f32; the rest as mocca_step, and capturable in a hipGraph under the same conditions.
 * MOCCA_E_ARG without a controller.  mocca_step on the same handle keeps its meaning: joint actions in, progress-only reward. */
int mocca_plan_step(mocca_handle h, const float *plan_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev, int32_t *info_dev, void *stream);
/* what the controller produced in the last mocca_plan_step: action_dev [N][21] f32 (before apply_action's clip) and value_dev [N] f32
 * (either may be NULL) */
int mocca_get_base_outputs(mocca_handle h, float *action_dev, float *value_dev, void *stream);

/* ---- where the links are, and what an env looks like (no reference counterpart for the first; the second stands in for
 *      EnvBase.render(mode="rgb_array"), env_base.py:120-159: getCameraImage with FOV 60, near 0.1, far 100) ---- */

/* Link frames of every env from the state the handle currently holds: frames_dev [N][n_bodies][15] f32, per body R (9, row-major,
 * world <- body), the body origin in world (3), the body's centre of mass in world (3).  A small kernel of its own (one thread per env);
 * asynchronous on `stream`. */
int mocca_get_link_frames(mocca_handle h, float *frames_dev, void *stream);

/* A camera record, MOCCA_CAMERA_FLOATS f32: eye (3), right (3), up (3), forward (3) -- orthonormal, right = forward x up --,
 * tan(fov_y / 2), aspect (width / height), near, far.  The pinhole of computeViewMatrixFromYawPitchRoll(upAxisIndex=2, roll 0) +
 * computeProjectionMatrixFOV: the eye sits `dist` behind the target along `forward`, `up` has a non-negative z.  (mocca_envs_amd/render.py
 * Camera counts yaw from +x: yaw 0, pitch 0 looks along +x with +z up.)
 * Pixel centres: pixel (column i, row j), row 0 at the TOP of the image, looks along
 *   d = forward + sx * right + sy * up,   sx = (2 (i + 1/2) / W - 1) * tan(fov_y / 2) * aspect,   sy = (1 - 2 (j + 1/2) / H) * tan(fov_y / 2)
 * from the eye.  d . forward = 1, so the ray parameter t of a hit is its distance along the view axis: the depth. */
#define MOCCA_CAMERA_FLOATS 16
#define MOCCA_RENDER_MAX_SIZE 4096 /* width and height: 1 .. 4096 */

/* values of the id image: -1 nothing, 0 .. n_geoms - 1 the robot geom that was hit, then: */
enum {
  MOCCA_RENDER_ID_NONE = -1,
  MOCCA_RENDER_ID_GROUND = 32,       /* = MOCCA_MAX_GEOMS: the plane z = 0 (Custom and Cassie tasks) */
  MOCCA_RENDER_ID_PLANK0 = 33,       /* + k: live plank k of the Stepper's terrain record, k < MOCCA_MAX_PLANKS */
  MOCCA_RENDER_ID_HEIGHTFIELD = 37,  /* the planner envs' terrain */
  MOCCA_RENDER_ID_TARGET = 38,       /* the walk target, a 0.15 m sphere (VSphere, env_locomotion.py:65,580,1027): visual only, it collides with nothing */
  MOCCA_RENDER_ID_LINK0 = 64,        /* + b: link b of a robot that is drawn as its skeleton (below), 1 <= b < n_bodies */
};

/* One ray per pixel through the scene of env env_ids_dev[v], seen by camera v, for v < n_views (the same env may be listed more than once):
 * the robot's geoms (spheres and capsules at the link frames above; a model whose geoms ALL have radius 0 -- Cassie, whose links are meshes in
 * the reference and hull support points here -- is drawn as its skeleton instead: a capsule of 4 cm radius from every link's parent origin to its own
 * origin, and for a link without children one from its origin through its centre of mass to twice that distance), the ground plane z = 0 (Custom and Cassie tasks), the live planks of the
 * Stepper's terrain record (oriented boxes, or upright cylinders for MOCCA_PLANK_CYLINDER), the planner envs' height field (the triangle
 * split mocca_set_heightfield documents, walked cell by cell along the ray) and the walk target of the walker tasks.  Meshes, textures and
 * shadows are not drawn.  Outputs, each optional (NULL):
 *   rgb_dev   [n_views][H][W][3] u8: base colour x (0.35 + 0.65 max(0, n . l)), l = (0.36, -0.48, 0.80) towards the one light, rounded to
 *             nearest.  Base colours: robot geoms a palette of 8 by body index, ground a two-tone 1 m checker, planks wood, height field a
 *             tint from low (green) to high (sand), target red; background (0.53, 0.71, 0.90) unshaded = (135, 181, 230).  Cosmetic.
 *   depth_dev [n_views][H][W] f32: distance along the view axis in metres; exactly `far` where nothing is hit.  Hits nearer than `near`
 *             are not seen (a surface is hit where the ray ENTERS it).
 *   id_dev    [n_views][H][W] i32: MOCCA_RENDER_ID_*.
 * Reads the state, task and terrain records and writes none of them.  Errors (MOCCA_E_ARG, with a message): an env index outside
 * 0 .. n_envs - 1, a planner handle before mocca_set_heightfield, width or height outside 1 .. MOCCA_RENDER_MAX_SIZE, n_views < 1.
 * The env indices are checked on the host: the call waits for `stream` once, before it launches (rendering is not on the training path;
 * not capturable in a hipGraph).  The first call, and a call with more views than any before, allocates. */
int mocca_render(mocca_handle h, const int32_t *env_ids_dev, int n_views, const float *cameras_dev, int width, int height, uint8_t *rgb_dev,
                 float *depth_dev, int32_t *id_dev, void *stream);

/* ---- what the ground around the robot looks like, ON the training path (no reference counterpart; the nearest is `use_egl`,
 *      env_base.py:160-201: a camera image for the policy) ---- */

/* The terrain height scan.  A pattern of n points (px, py), metres, in the robot's HEADING frame (x ahead, y to the left) is attached once;
 * mocca_height_scan then writes, for every env e and point p,
 *     clamp(hit_z - base_z, -max_drop, +z_above)
 * where the base position and quaternion are words 0..6 of the state record, (cos yaw, sin yaw) come from the quaternion exactly as the
 * observation's heading does (no atan2 / sin / cos round trip away from the gimbal branches, which are handled alike), the world point is
 * xy = base_xy + R_z(yaw) (px, py), and hit_z is where the vertical ray that runs DOWN from z_start = base_z + z_above first meets the
 * terrain: -max_drop where it meets nothing (or nothing within max_drop below the base), +z_above where the start point already lies
 * inside a solid.  Only terrain is seen -- never the robot's own geoms or the walk target: the plane z = 0 (Custom and Cassie tasks); the live
 * planks of the Stepper's terrain record, staged as mocca_render stages them (oriented boxes, upright cylinders for MOCCA_PLANK_CYLINDER;
 * no ground); the planner envs' height field, the surface of the cell under the point with the triangle split mocca_set_heightfield
 * documents (outside the grid there is no ground).
 *   mocca_set_height_scan  points_host [n_points][2] f32 (HOST memory, copied into the handle), 1 <= n_points <= MOCCA_SCAN_MAX_POINTS, finite;
 *                          z_above >= 0, max_drop > 0.  points_host == NULL detaches.  May synchronise the device.
 *   mocca_scan_dim         n_points, 0 when no pattern is attached.
 *   mocca_height_scan      obs_dev == NULL: row e is out_dev[e * row_stride .. + n_points).  obs_dev [N][obs_dim] f32: row e is
 *                          [obs (obs_dim) | scan (n_points)] -- the same launch copies the observation, so a trainer's widened policy input
 *                          costs one extra launch and no concatenation.  Floats of a row beyond what is written are left untouched; out_dev
 *                          must not overlap obs_dev.  One kernel, one wave per env, asynchronous on `stream`: no allocation, no host read, no
 *                          synchronisation, no atomics -- capturable in a hipGraph together with mocca_step / mocca_plan_step.  Reads the
 *                          state, task and terrain records and writes none of them; the scan belongs to the state the handle holds when
 *                          the launch runs (after an auto-reset step: the new episode's first state, like the observation).
 * Errors (MOCCA_E_ARG, with a message): mocca_height_scan before mocca_set_height_scan, n_points outside 1 .. MOCCA_SCAN_MAX_POINTS, a
 * non-finite point, z_above < 0 or max_drop <= 0, row_stride smaller than the row, a planner handle before mocca_set_heightfield. */
#define MOCCA_SCAN_MAX_POINTS 256
int mocca_set_height_scan(mocca_handle h, const float *points_host, int n_points, double z_above, double max_drop);
int mocca_scan_dim(mocca_handle h);
int mocca_height_scan(mocca_handle h, float *out_dev, int row_stride, const float *obs_dev, void *stream);

/* The egocentric depth camera: a small depth image per env from a pinhole that rides on one of the robot's links, cast with mocca_render's
 * geometry -- the same pixel centres, rays and depth (t along the view axis) -- but for all N envs in one launch on the training path.
 * Mount: mount_host [6] f32 (HOST memory) is the eye's offset (3) in `body`'s frame, then roll, pitch, yaw in radians.  The camera's axes
 * in the MOUNT frame are the columns of R_z(yaw) R_y(pitch) R_x(roll) (the planks' Euler order): forward = column 0, up = column 2,
 * right = forward x up.  With all angles zero the camera looks along the mount's +x with +z up; a POSITIVE pitch looks down.  The mount
 * frame is `body`'s R of mocca_get_link_frames (a rigid mount), or with MOCCA_DEPTH_STABILISED R_z(yaw) of the base's heading, from the
 * (cos yaw, sin yaw) mocca_height_scan uses.  In both modes the eye is origin_body + R_body offset.
 * Seen: the plane z = 0 (Custom and Cassie tasks), the live planks, the env's own height field from the bank and, with
 * MOCCA_DEPTH_SEE_ROBOT, the robot as mocca_render draws it (its geoms, or its skeleton).  The walk target is never seen: it is visual only.
 *   mocca_set_depth_camera  body 0 .. n_bodies - 1; 1 <= width, height <= 64, width * height <= MOCCA_DEPTH_MAX_PIXELS; 0 < fov_y < pi
 *                           (radians); 0 < near < far; flags a sum of MOCCA_DEPTH_*.  mount_host == NULL detaches.  Allocates nothing.
 *   mocca_depth_dim         width * height, 0 when no camera is attached.
 *   mocca_depth_camera      obs_dev == NULL: row e is out_dev[e * row_stride .. + width * height).  obs_dev [N][obs_dim] f32: row e is
 *                           [obs (obs_dim) | depth] -- the same launch copies the observation, as mocca_height_scan does.  Entry
 *                           j * width + i of the image is the depth in metres of pixel (column i, row j), row 0 on top; exactly `far`
 *                           where nothing is entered in [near, far).  Floats of a row beyond what is written are left untouched; out_dev
 *                           must not overlap obs_dev.  cameras_dev [N][MOCCA_CAMERA_FLOATS] f32 or NULL: the camera records the rays were
 *                           cast from (pass them to mocca_render to watch what the robot sees); bit for bit the same with and without
 *                           MOCCA_DEPTH_SEE_ROBOT.  One kernel, one wave per env, asynchronous on `stream`: no allocation, no host read,
 *                           no synchronisation, no atomics -- capturable in a hipGraph together with mocca_step / mocca_plan_step /
 *                           mocca_act_step.  Reads the state, task and terrain records and writes none of them; a non-finite pose
 *                           leaves finite depths in [near, far], `far` along every ray that is not finite.  An [obs | scan | depth] row: mocca_height_scan with obs_dev, then this call with out_dev
 *                           advanced by obs_dim + scan_dim and obs_dev == NULL.
 * Errors (MOCCA_E_ARG, with a message; the handle is unchanged and nothing is launched): body outside 0 .. n_bodies - 1, width or height
 * outside 1 .. 64 or their product above MOCCA_DEPTH_MAX_PIXELS, a non-finite mount, fov_y outside (0, pi), near <= 0, far <= near, a
 * non-finite near or far, unknown flag bits, mocca_depth_camera before mocca_set_depth_camera, row_stride smaller than the row, out_dev
 * NULL, a planner handle before mocca_set_heightfield. */
#define MOCCA_DEPTH_MAX_PIXELS 256
#define MOCCA_DEPTH_STABILISED 1   /* orientation from the base's heading only */
#define MOCCA_DEPTH_SEE_ROBOT  2   /* the robot's own geoms (or its skeleton) occlude */
int mocca_set_depth_camera(mocca_handle h, int body, const float *mount_host /* [6] */, int width, int height, double fov_y, double near,
                           double far, int flags);
int mocca_depth_dim(mocca_handle h);
int mocca_depth_camera(mocca_handle h, float *out_dev, int row_stride, const float *obs_dev, float *cameras_dev, void *stream);

/* ---- the trainer's own policy on the device (no reference counterpart: the reference's trainers, README.md:33-39, run their
 *      pytorch-a2c-ppo-acktr `actor_critic.act()` in torch, four small kernels and a sampler per step) ---- */

/* A diagonal-Gaussian actor-critic: an actor MLP (the mean), a critic MLP, a state-independent log_std[act_dim] and, optionally, the
 * observation normalisation x = clamp((x - mean[k]) * inv_std[k], -clip, +clip) (VecNormalize; inv_std = 1 / sqrt(var + eps), formed by the
 * caller in f32) in front of both nets.  Layout, arithmetic and the noise: mocca_envs_amd/csrc/mocca_policy.h.
 *
 * mocca_set_policy      replaces building the trainer's `Policy(obs_shape, action_space)`: SHAPES only.  layers_host [n_layers_total][8] i32 (HOST
 *                       memory), the rows of mocca_set_base_controller -- {net 0 actor / 1 critic, in, out, in rounded up to a multiple of 16, out
 *                       rounded up likewise, activation (0 identity, 1 relu, 2 tanh, 3 softsign), ignored, ignored} --, the actor's layers first.
 *                       At most 8 layers per net; a net's first layer takes in_dim inputs (1 .. 336); hidden widths multiples of 16 up to 256;
 *                       the actor ends in act_dim (1 .. 32) outputs, the critic in 1; clip finite and > 0.  Every dimension is checked
 *                       (MOCCA_E_ARG with a message).  Allocates the kernel's image; layers_host == NULL detaches.  May synchronise.
 * mocca_update_policy   replaces nothing in the trainer -- it is what makes `optimizer.step()` visible to the kernel: call it once per PPO
 *                       iteration.  params_dev [n_floats] f32 (DEVICE memory): per layer in table order W[out][in] row-major then b[out], then
 *                       log_std[act_dim]; optionally mean[in_dim] and inv_std[in_dim] follow (n_floats tells which; without them the input is
 *                       not normalised).  One repack kernel on `stream` writes the image; no synchronisation, no host read: inside or between
 *                       replays of a captured graph the next mocca_act on the stream sees the new parameters.
 * mocca_act             replaces `value, action, action_log_prob = actor_critic.act(obs)`: one launch.  in_dev [N][in_stride] f32, the first
 *                       in_dim floats of each row are read (rollouts.obs[t], or a wider [obs | scan] row).  eps_dev [N][act_dim] f32 or NULL;
 *                       deterministic != 0: action = mean; both off: noise drawn in the kernel from (seed, global env id, the env's step and
 *                       episode counters) -- two calls without a mocca_step in between draw the same noise.  Outputs: action_dev [N][act_dim]
 *                       (not clipped: apply_action clips), logp_dev [N] or NULL (sum over j of -eps^2 / 2 - log_std - log(2 pi) / 2), value_dev
 *                       [N] or NULL, mean_dev [N][act_dim] or NULL.  No allocation, no synchronisation, no atomics, no host state.
 * mocca_act_step        replaces `act()` followed by `envs.step(action)`: mocca_act, then mocca_step on action_dev, on the same stream; the
 *                       step's results are mocca_step's bit for bit, and the pair is capturable in a hipGraph under mocca_step's conditions.
 * mocca_act_plan_step   replaces, in a trainer of the planner envs' high-level policy, `act()` followed by `envs.step(plan)`: mocca_act with
 *                       plan_dev [N][15] as its action_dev, then mocca_plan_step on plan_dev, on the same stream -- three launches in a linear
 *                       chain (policy, base controller, step).  The results are those of the two calls bit for bit (noise keying, NULL
 *                       options, in_stride-wide rows, the reward's log(max(1, value)) / 3 term).  No allocation, no synchronisation, no
 *                       host read: capturable in a hipGraph under mocca_step's conditions.  MOCCA_E_ARG with a message, nothing launched:
 *                       mocca_act's and mocca_plan_step's own errors, a task other than the planner task, no base controller, an
 *                       attached policy whose act_dim is not mocca_plan_dim(h).
 * mocca_set_policy_symmetry  replaces SymmetricRL's symmetric network (`SymmetricNet` around the actor and the critic, built from the env's
 *                       `get_mirror_indices()`): the attached policy becomes mirror-symmetric by construction,
 *                           mean_sym(s) = 1/2 (f(n(s)) + M_a f(n(M_o s)))        value_sym(s) = 1/2 (V(n(s)) + V(n(M_o s)))
 *                       with (M x)[k] = sign[k] * x[perm[k]], n the normalisation (the mirror acts on the raw row) and log_std replaced by
 *                       1/2 (log_std[j] + log_std[act_perm[j]]).  in_perm_host i32 / in_sign_host f32 [in_dim], act_perm_host i32 /
 *                       act_sign_host f32 [act_dim] (HOST memory, copied into the handle).  Each table must be valid: indices in range,
 *                       perm[perm[k]] == k, sign[k] +1 or -1, sign[perm[k]] == sign[k] (so that M M = I); a violation is MOCCA_E_ARG with a
 *                       message and leaves the handle as it was.  While attached, mocca_act / mocca_act_step launch the kernel's symmetric
 *                       instance -- still one launch, twice the matrix work; their contract holds as it stands (outputs, NULL options, noise
 *                       keying, capture conditions; mean_dev receives mean_sym).  in_perm_host == NULL detaches; mocca_set_policy drops an
 *                       attached symmetry (the shapes may have changed); mocca_update_policy leaves it alone.  May synchronise.
 * mocca_set_policy_mirror_loss  attaches SymmetricRL's mirror-symmetry LOSS (`--mirror_method loss`, `symmetry_coef`) FOR THE GRADIENT ONLY:
 *                       the four tables of mocca_set_policy_symmetry under the same validity rules, and mirror_coef, a finite weight
 *                       >= 0 (0: the term is monitored, not trained on).  The policy stays the plain one: while attached, mocca_act /
 *                       mocca_act_step launch the plain instance and give the bits they give with nothing attached; mocca_ppo_grad_mirror
 *                       (below) is the gradient, mocca_ppo_update runs it, and mocca_ppo_grad / mocca_ppo_grad_sym refuse.  The two
 *                       attachments exclude each other -- a symmetric network has zero mirror loss by construction --: each setter
 *                       refuses while the other's attachment is in place, the caller detaches first.  in_perm_host == NULL detaches;
 *                       mocca_set_policy drops the attachment; mocca_update_policy leaves it alone.  A violation (an invalid table, a
 *                       negative or non-finite mirror_coef, a symmetry attached) is MOCCA_E_ARG with a message and leaves the handle as
 *                       it was.  May synchronise.
 * mocca_set_policy_mirror_dup  attaches SymmetricRL's DUPLICATED TUPLES (every rollout tuple (s, a) is
 *                       trained on together with its mirror image (M_o s, M_a a)) FOR THE GRADIENT ONLY: the four tables of
 *                       mocca_set_policy_symmetry under the same validity rules.  The policy stays the plain one: while attached,
 *                       mocca_act / mocca_act_step launch the plain instance and give the bits they give with nothing attached;
 *                       mocca_ppo_grad_dup (below) is the gradient, mocca_ppo_update runs it, and mocca_ppo_grad / mocca_ppo_grad_sym /
 *                       mocca_ppo_grad_mirror refuse.  The THREE attachments (symmetry, mirror loss, duplicated rows) exclude one
 *                       another: each setter refuses while another's attachment is in place and names it, the caller detaches first.
 *                       in_perm_host == NULL detaches; mocca_set_policy drops the attachment; mocca_update_policy leaves it alone.  A
 *                       violation is MOCCA_E_ARG with a message and leaves the handle as it was.  May synchronise.
 * Errors (MOCCA_E_ARG, with a message): a NULL handle, any bad dimension, mocca_update_policy / mocca_act / mocca_set_policy_symmetry before
 * mocca_set_policy, mocca_act before mocca_update_policy, n_floats that fits neither form, in_stride < in_dim, mocca_act_step with act_dim other
 * than the env's, an invalid mirror table, a negative or non-finite mirror_coef, any of the three mirror attachments while another is in place, global env ids (MOCCA_PARAM_ENV_OFFSET + n_envs) beyond 2^28 (the noise's counter holds 16 x env id
 * in one 32-bit word). */
int mocca_set_policy(mocca_handle h, const int32_t *layers_host, int n_layers_total, int in_dim, int act_dim, double clip);
int mocca_update_policy(mocca_handle h, const float *params_dev, size_t n_floats, void *stream);
int mocca_act(mocca_handle h, const float *in_dev, int in_stride, const float *eps_dev, int deterministic, float *action_dev, float *logp_dev,
              float *value_dev, float *mean_dev, void *stream);
int mocca_act_step(mocca_handle h, const float *in_dev, int in_stride, const float *eps_dev, int deterministic, float *action_dev,
                   float *logp_dev, float *value_dev, float *mean_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev, int32_t *info_dev,
                   void *stream);
int mocca_act_plan_step(mocca_handle h, const float *in_dev, int in_stride, const float *eps_dev, int deterministic, float *plan_dev,
                        float *logp_dev, float *value_dev, float *mean_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev,
                        int32_t *info_dev, void *stream);
int mocca_set_policy_symmetry(mocca_handle h, const int32_t *in_perm_host, const float *in_sign_host, const int32_t *act_perm_host,
                              const float *act_sign_host);
int mocca_set_policy_mirror_loss(mocca_handle h, const int32_t *in_perm_host, const float *in_sign_host, const int32_t *act_perm_host,
                                 const float *act_sign_host, double mirror_coef);
int mocca_set_policy_mirror_dup(mocca_handle h, const int32_t *in_perm_host, const float *in_sign_host, const int32_t *act_perm_host,
                                const float *act_sign_host);

/* ---- the end of a rollout on the device (no reference counterpart: the reference's trainers run these in torch, a Python loop over the
 *      rollout's steps and a handful of reductions per iteration) ---- */

/* mocca_gae         replaces `rollouts.compute_returns(next_value, use_gae=True, gamma, gae_lambda, use_proper_time_limits=True)` and the
 *                   advantage normalisation of `ppo.update` (`advantages = returns[:-1] - value_preds[:-1]`, then `(advantages -
 *                   advantages.mean()) / (advantages.std() + 1e-5)`): two launches.  All arrays contiguous f32 on the device, N = n_envs,
 *                   T = n_steps: rew_dev [T][N]; value_dev, masks_dev, bad_masks_dev [T + 1][N] -- a2c-ppo-acktr's storage with the trailing 1
 *                   dropped; value_dev[T] is next_value, rows 1 .. T of the two masks are read.  Each line element below is ONE IEEE f32
 *                   operation, in this order, never contracted into an FMA:
 *                       g = f32(gamma);  c = f32(gamma * lam, the product in double);  s = f32(reward_scale);  gae = 0
 *                       for t = T - 1 .. 0:
 *                           delta  = ((r[t] * s) + ((g * v[t + 1]) * m[t + 1])) - v[t]
 *                           gae    = (delta + ((c * m[t + 1]) * gae)) * bm[t + 1]
 *                           adv[t] = gae;   ret[t] = gae + v[t]
 *                   so an episode cut by the TimeLimit (bad_masks = 0) has advantage 0 at the cut and nothing flows through it.  returns_dev
 *                   and adv_dev [T][N] (returns_dev may be NULL; adv_dev and moments_dev may be NULL only with normalise == 0).  The sums of
 *                   adv and adv^2 are taken in f64 in a fixed order (per env, per workgroup, then the workgroups in index order; no atomics:
 *                   the same bits on every run); with B = T N, moments_dev[0] = mean = f32(S1 / B) and moments_dev[1] = std =
 *                   f32(sqrt(max(S2 - S1^2 / B, 0) / (B - 1))) (Bessel's correction, torch's .std(); NaN for B = 1); normalise != 0
 *                   rewrites adv <- (adv - mean) / (std + f32(adv_eps)) in f32 with a correctly rounded division.  1 <= T <= 65536.
 * mocca_obs_stats   replaces VecNormalize's `ob_rms.update(obs)` (baselines' RunningMeanStd) over a whole rollout: two launches.  rows_dev
 *                   [n_rows][row_stride] f32, the first dim (1 .. 336) floats of a row are read and nothing beyond them (rollouts.obs[1:],
 *                   or wider [obs | scan | ...] rows).  state_dev f64 [1 + 2 dim] = count, mean[dim], var[dim], CALLER-owned; a fresh state is
 *                   count 1e-4, mean 0, var 1.  In f64, with d = x - mean[k] summed in a fixed order (no atomics) and n = n_rows:
 *                       bm = mean + sum(d) / n;  bv = sum(d^2) / n - (sum(d) / n)^2;  delta = bm - mean;  tot = count + n
 *                       mean' = mean + delta n / tot;  var' = (var count + bv n + delta^2 count n / tot) / tot;  count' = tot
 *                   The state is written back; mean_dev[k] = f32(mean') and inv_std_dev[k] = 1.0f / sqrtf(f32(var') + f32(eps)) (square
 *                   root and division correctly rounded) go to two caller arrays of dim floats, either may be NULL -- meant to be the tail
 *                   of the params_dev that mocca_update_policy takes, so that the trainer's flat parameter tensor needs no torch.cat.
 * Both keep their scratch in the handle: it is allocated on the first call and on a later call that needs more (more envs' workgroups, more
 * rows or a larger dim), and such a call may synchronise.  Every other call is asynchronous on `stream`: no allocation, no host read, no
 * synchronisation, no atomics -- after one warm call with the same shapes both are capturable in a hipGraph (a linear chain on one stream).
 * They read and write none of the handle's env records.
 * Errors (MOCCA_E_ARG, with a message): a NULL handle or required pointer, n_steps outside 1 .. 65536, normalise with T N < 2 or without
 * adv_dev / moments_dev, non-finite gamma / lam / reward_scale, a non-finite or negative adv_eps / eps, dim outside 1 .. 336, row_stride <
 * dim, n_rows < 1. */
int mocca_gae(mocca_handle h, const float *rew_dev, const float *value_dev, const float *masks_dev, const float *bad_masks_dev,
              int n_steps, double gamma, double lam, double reward_scale, float *returns_dev, float *adv_dev,
              int normalise, double adv_eps, float *moments_dev, void *stream);
int mocca_obs_stats(mocca_handle h, const float *rows_dev, int64_t n_rows, int row_stride, int dim, double *state_dev, double eps,
                    float *mean_dev, float *inv_std_dev, void *stream);

/* ---- a PPO minibatch step on the device (no reference counterpart: the reference's trainers run it in torch, a few dozen small launches
 *      per minibatch) ---- */

/* mocca_ppo_grad    replaces the body of `ppo.update`'s minibatch loop up to `optimizer.step()`: `evaluate_actions`, the clipped surrogate,
 *                   the value loss, `loss.backward()` -- four launches, for the plain policy of mocca_set_policy (the symmetric one: mocca_ppo_grad_sym below).  R rollout rows, B = n_rows
 *                   of them form the minibatch.  obs_dev [R][obs_stride] f32: the first in_dim floats of a row are read, RAW (normalised in
 *                   the kernel exactly as mocca_act does); action_dev [R][act_dim] the stored samples; old_logp_dev, adv_dev, returns_dev
 *                   [R]; old_value_dev [R], may be NULL when value_clip == 0.  idx_dev [B] i64 (a chunk of torch.randperm): minibatch row b
 *                   is rollout row idx_dev[b]; NULL: rows 0 .. B - 1.  THE INDEX RANGE IS NOT CHECKED on the device: every idx_dev[b] must
 *                   lie in 0 .. R - 1, that is the caller's duty.  With every mean over the B rows:
 *                       logp = sum_j ( -1/2 ((a_j - mu_j) / sigma_j)^2 - log_std_j - 1/2 log 2 pi )      r = exp(logp - old_logp)
 *                       L_pi = -mean( min(r A, clamp(r, 1 - clip, 1 + clip) A) )
 *                       L_v  = 1/2 mean( (v - ret)^2 )      value_clip != 0: 1/2 mean( max((v - ret)^2, (v_old + clamp(v - v_old, -clip, clip) - ret)^2) )
 *                       H    = sum_j ( log_std_j + 1/2 + 1/2 log 2 pi )
 *                       L    = L_pi + value_coef L_v - entropy_coef H
 *                   The gradient is torch autograd's for that expression: a row reaches the actor unless A > 0 and r > 1 + clip, or A < 0
 *                   and r < 1 - clip; the value-clip max passes the gradient of the larger term, of the unclipped one at a tie.  Per row,
 *                   each line ONE IEEE f32 operation in this order, never contracted into an FMA; ib = 1.0f / f32(B), lo = 1.0f - f32(clip),
 *                   hi = 1.0f + f32(clip), c = f32(clip), mu / v the heads of the actor / critic, ls = log_std:
 *                       for j ascending:   s = expf(ls[j]);  d = a[j] - mu[j];  z = d / s
 *                                          t = -0.5f * z;  t = t * z;  t = t - ls[j];  t = t - 0.9189385...;  logp = logp + f64(t)
 *                       dl = f32(logp - f64(old_logp));  r = expf(dl)      (logp alone is summed in f64: ~20 terms of size 1 added in
 *                                                                           f32 would leave 1e-6 in every ratio)
 *                       s1 = r * A;  rc = min(max(r, lo), hi);  s2 = rc * A;  surrogate = min(s1, s2)
 *                       g = A * r;  g = g * ib;  g = -g            (dL/dlogp; g = 0 for a row that does not reach the actor)
 *                       for j:             w = z / s;  dL/dmu[j] = g * w
 *                                          q = z * z;  q = q - 1.0f;  dL/dlog_std[j] (the row's term) = g * q
 *                       e = v - ret;  l = e * e;  dv = e
 *                       value_clip:        dd = v - v_old;  dc = min(max(dd, -c), c);  vc = v_old + dc;  e2 = vc - ret;  l2 = e2 * e2
 *                                          if (dd < -c or dd > c) and l2 > l:  l = l2;  dv = 0
 *                                          (where the clamp passes, -c <= dd <= c, vc IS v and the two terms are the same function of v: a
 *                                          tie, so the unclipped term and its gradient are used rather than a rounding of vc)
 *                       value loss = 0.5f * l;  dv = f32(value_coef) * dv;  dL/dv = dv * ib
 *                   Through the layers: dZ = dA * act'(x), the derivative formed in the forward from the pre-activation x -- tanh:
 *                   sech^2 x = 4 e / (1 + e)^2 with e = expf(-2 |x|); relu: 1 where x > 0; softsign: 1 / (1 + |x|)^2; identity: 1 -- and kept
 *                   where dZ will go: the same functions as 1 - y y and (1 - |y|)^2 of the output y, without their cancellation where a unit
 *                   saturates.  The matrix products run on the matrix cores in f32 with a fixed order of sums
 *                   (mocca_envs_amd/csrc/mocca_ppo.h), rows ascending: the same inputs give the same bits on every run and on every
 *                   device.  grad_dev [n_head] f32 in mocca_update_policy's order -- per layer W[out][in] row-major then b[out], actor then
 *                   critic, then log_std[act_dim], n_head = that order's length without mean / inv_std -- is fully overwritten; log_std's
 *                   entry is the rows' sum minus f32(entropy_coef).  stats_dev [8] f32 or NULL: mean of the surrogate (= -L_pi), L_v,
 *                   H (summed in f64, stored as f32), mean(old_logp - logp), the fraction of rows with r outside [lo, hi] (the count divided by B), the sum of grad_dev^2
 *                   (summed in f64, stored as f32), 0, 0.  The means multiply by ib.
 *                   The forward is mocca_act's layer loop with ONE difference: tanh is (float)tanh((double)x), rounded once, where
 *                   mocca_act calls tanhf; logp and the value recomputed at unchanged weights therefore differ from what mocca_act stored by
 *                   an ulp or two, and the first minibatch's ratio is 1 +- 1e-6 rather than exactly 1.
 *                   Scratch (every layer's activations and their gradients for B rows) is kept in the handle: allocated on the first call
 *                   and on one that needs more, and such a call may synchronise.  Its size is 4 B (in_pad + 2 sum of the layers' out_pad
 *                   + 48) bytes plus 16 padded gradients at most: for the 52 -> 256 -> 256 -> {21, 1} policy 9 KB per row, 150 MB at
 *                   B = 16384 and 38 GB at the bound of 2^22 rows, where the allocation may fail (MOCCA_E_HIP; the handle keeps its old
 *                   scratch).  A call that grows the scratch FREES the old one: a graph captured at a smaller B still points to it and
 *                   must be recaptured -- warm the handle with the largest B it will see before capturing.  Every other call is asynchronous on `stream`: no
 *                   allocation, no host read, no synchronisation, no atomics -- after one warm call with the same B it is capturable in a
 *                   hipGraph as a linear chain.  It reads the policy image that mocca_update_policy last wrote (an update between two
 *                   replays is seen) and none of the handle's env records; it writes only grad_dev, stats_dev and its scratch.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): a NULL handle; called before mocca_set_policy / mocca_update_policy; a
 * NULL obs_dev, action_dev, old_logp_dev, adv_dev, returns_dev or grad_dev; value_clip with old_value_dev NULL; n_rows < 1 or > 2^22;
 * obs_stride < in_dim; a non-finite or negative clip, value_coef or entropy_coef; a handle with mirror tables attached
 * (mocca_set_policy_symmetry) -- the symmetric policy's gradient is mocca_ppo_grad_sym: call that, or detach the tables first; a handle
 * with a mirror loss attached (mocca_set_policy_mirror_loss) -- that loss's gradient is mocca_ppo_grad_mirror; a handle with duplicated
 * rows attached (mocca_set_policy_mirror_dup) -- their gradient is mocca_ppo_grad_dup. */
int mocca_ppo_grad(mocca_handle h, const float *obs_dev, int obs_stride, const float *action_dev, const float *old_logp_dev,
                   const float *adv_dev, const float *returns_dev, const float *old_value_dev, const int64_t *idx_dev, int64_t n_rows,
                   double clip, double value_coef, double entropy_coef, int value_clip, float *grad_dev, float *stats_dev, void *stream);

/* mocca_ppo_grad_sym  mocca_ppo_grad for the mirror-symmetric policy of mocca_set_policy_symmetry (SymmetricRL's symmetric network): replaces
 *                   the same minibatch body with `evaluate_actions` of the symmetric net -- two passes through both nets forward and back --
 *                   in the same four launches.  The argument list, the arrays, idx_dev (NOT range-checked), grad_dev's order and stats_dev
 *                   are mocca_ppo_grad's.  It differentiates mocca_act's symmetric policy: with x1 = n(s) and x2 = n(M_o s) -- the mirror
 *                   (M x)[k] = sign[k] * x[perm[k]] taken on the RAW row, the statistics indexed by k --,
 *                       f1 = actor(x1)   f2 = actor(x2)   v1 = critic(x1)   v2 = critic(x2)
 *                   and per row, each line ONE IEEE f32 operation in this order, never contracted into an FMA, pj = act_perm[j]:
 *                       for j ascending:   mm = f2[pj] * act_sign[j];  mu[j] = f1[j] + mm;  mu[j] = 0.5f * mu[j]
 *                                          ls[j] = log_std[j] + log_std[pj];  ls[j] = 0.5f * ls[j]
 *                       v = v1 + v2;  v = 0.5f * v
 *                   mocca_ppo_grad's per-row lines follow UNCHANGED on mu, ls and v: logp summed in f64, r, the surrogate, g,
 *                   dL/dmu[j] = g * w, the row's log_std term g * q, the value loss with its clamp tie rule, dL/dv.  The heads receive
 *                       for j:             h = 0.5f * dL/dmu[j];  dL/df1[j] = h;  dL/df2[pj] = h * act_sign[j]
 *                                          (each pj is written once: act_perm is a bijection)
 *                       dL/dv1 = dL/dv2 = 0.5f * dL/dv
 *                   and both passes run mocca_ppo_grad's backward; every weight's and bias's gradient is the sum over BOTH passes (the
 *                   matrix cores add them in one fixed order, as-given and mirrored columns interleaved eight by eight).  log_std: with T[j]
 *                   the rows' sum of g * q_j (the row chunks added in chunk order, as in mocca_ppo_grad),
 *                       grad[log_std j] = 0.5f * (T[j] + T[pj]) - f32(entropy_coef)
 *                   (H = sum_j ls[j] + const has derivative 1 with respect to every log_std[j]: the perm is a bijection).  stats_dev keeps
 *                   its meanings: the means are over the B rows, not the 2 B columns; stats[2] is the entropy of the SYMMETRISED log_std,
 *                   sum_j (f64(ls[j]) + 1/2 + 1/2 log 2 pi) in f64 with j ascending, ls[j] the f32 value above.
 *                   The forward is mocca_act's symmetric instance with mocca_ppo_grad's one difference (tanh rounded once).
 *                   Scratch: the handle's, shared with mocca_ppo_grad, and TWICE its size per row -- the activations of both passes,
 *                   16 ceil(B / 8) scratch rows: 8 (in_pad + 2 sum of the layers' out_pad + 48) B bytes, 18 KB per row for the 52 -> 256 ->
 *                   256 -> {21, 1} policy, 300 MB at B = 16384; n_rows is 1 .. 2^21, so that the scratch's row count stays within what
 *                   mocca_ppo_grad allows.  Growing FREES the old scratch, for the pair: a symmetric call at some B after a plain call
 *                   at the same B grows it, and a graph captured before -- of either call -- must be recaptured; warm the handle with the
 *                   largest call it will see (a symmetric call at B covers a plain one at 2 B) before capturing.  A captured call also
 *                   holds the mirror tables' device arrays: mocca_set_policy_symmetry and mocca_set_policy replace them, and a graph
 *                   captured before must be recaptured.  Otherwise mocca_ppo_grad's conditions hold as they stand: asynchronous on `stream`,
 *                   no allocation, no host read, no synchronisation, no atomics, every sum's order a function of B and the shapes alone
 *                   -- the same inputs give the same bits --, capturable as a linear chain after one warm call with the same B; it sees
 *                   a mocca_update_policy made between two replays; it writes only grad_dev, stats_dev and its scratch.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): those of mocca_ppo_grad with n_rows > 2^21 in place of 2^22; and a
 * policy WITHOUT mirror tables attached (mocca_set_policy_symmetry) -- the plain policy's gradient is mocca_ppo_grad; a handle with a mirror
 * loss attached (mocca_ppo_grad_mirror is its gradient) or with duplicated rows attached (mocca_ppo_grad_dup is theirs). */
int mocca_ppo_grad_sym(mocca_handle h, const float *obs_dev, int obs_stride, const float *action_dev, const float *old_logp_dev,
                       const float *adv_dev, const float *returns_dev, const float *old_value_dev, const int64_t *idx_dev, int64_t n_rows,
                       double clip, double value_coef, double entropy_coef, int value_clip, float *grad_dev, float *stats_dev, void *stream);

/* mocca_ppo_grad_mirror  mocca_ppo_grad with SymmetricRL's mirror-symmetry loss added (mocca_set_policy_mirror_loss): the PLAIN policy, and an
 *                   auxiliary term that pulls it towards mirror symmetry, in the same four launches.  The argument list, the arrays,
 *                   idx_dev (NOT range-checked) and grad_dev's order are mocca_ppo_grad's.  With f1 = actor(n(s)), f2 = actor(n(M_o s))
 *                   -- the mirror (M x)[k] = sign[k] * x[perm[k]] taken on the RAW row, as in mocca_ppo_grad_sym --, pj = act_perm[j], A =
 *                   act_dim:
 *                       L   = L_ppo (mocca_ppo_grad's L of the plain policy) + mirror_coef L_m
 *                       d_j = f1[j] - act_sign[j] f2[pj]        L_m = 1 / (B A) sum_rows sum_j d_j^2
 *                   which is torch's `(mirror(actor(mirror_obs)) - actor(obs)).pow(2).mean()`; BOTH passes carry gradient, nothing is
 *                   detached (a trainer whose loss differs by a constant factor folds it into mirror_coef).  mu = f1, ls = log_std and
 *                   v = critic(n(s)) are NOT symmetrised: mocca_ppo_grad's per-row lines, log_std's gradient and the entropy apply to
 *                   them unchanged.  The mirror term per row, each line ONE IEEE f32 operation in this order, never contracted into an
 *                   FMA; ib as in mocca_ppo_grad:
 *                       ia = 1.0f / f32(A);  k2 = f32(2 mirror_coef)      (the product in double)
 *                       for j ascending:   mm = f2[pj] * act_sign[j];  d = f1[j] - mm
 *                                          q = d * d;  m64 = m64 + f64(q)
 *                                          u = d * ib;  u = u * ia;  u = u * k2
 *                                          dL/df1[j] = (g * w) + u          (mocca_ppo_grad's dL/dmu[j] plus u)
 *                                          dL/df2[pj] = -(u * act_sign[j])  (each pj is written once: act_perm is a bijection)
 *                       the row's mirror term = f32(m64) * ia
 *                   Both actor passes run mocca_ppo_grad's backward and every actor weight's and bias's gradient is the sum over both, as
 *                   in mocca_ppo_grad_sym.  The critic receives NO mirror term: its mirrored columns hold zeros and contribute exactly
 *                   nothing to any gradient.  stats_dev [8]: [0..5] keep mocca_ppo_grad's meanings, [6] = 0, [7] = L_m -- the rows' mirror
 *                   terms summed in f64 like the other statistics (row chunks in chunk order), times ib.
 *                   Scratch, the n_rows bound (2^21), the grow-FREES-the-old rule and the capture conditions are mocca_ppo_grad_sym's: twice
 *                   the plain call's scratch per row, shared with the other two calls; a captured call holds the attachment's device
 *                   tables, and mirror_coef is a kernel argument, BAKED INTO a captured call: mocca_set_policy_mirror_loss and
 *                   mocca_set_policy ask for a new capture.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): those of mocca_ppo_grad with n_rows > 2^21 in place of 2^22; and a
 * handle WITHOUT a mirror loss attached (mocca_set_policy_mirror_loss); a handle with duplicated rows attached (mocca_ppo_grad_dup is
 * their gradient). */
int mocca_ppo_grad_mirror(mocca_handle h, const float *obs_dev, int obs_stride, const float *action_dev, const float *old_logp_dev,
                          const float *adv_dev, const float *returns_dev, const float *old_value_dev, const int64_t *idx_dev, int64_t n_rows,
                          double clip, double value_coef, double entropy_coef, int value_clip, float *grad_dev, float *stats_dev, void *stream);

/* mocca_ppo_grad_dup  mocca_ppo_grad on MIRROR-DUPLICATED rows (mocca_set_policy_mirror_dup; SymmetricRL's duplicated tuples): the PLAIN policy
 *                   and mocca_ppo_grad's loss L, un-symmetrised and with no term added, over 2 B samples in the same four launches.  The
 *                   argument list, the arrays, idx_dev (NOT range-checked) and grad_dev's order are mocca_ppo_grad's.  With the mirror
 *                   (M x)[k] = sign[k] * x[perm[k]]:
 *                       sample b      the row as given: s, a, old_logp, adv, returns, old_value
 *                       its twin      observation M_o s -- mirrored on the RAW row and then normalised by k, exactly as
 *                                     mocca_ppo_grad_sym stages it --; action a'[j] = a[act_perm[j]] * act_sign[j], ONE f32 operation, exact;
 *                                     the row's OWN old_logp, adv, returns and old_value
 *                   Every mean is over the 2 B samples: ib = 1.0f / f32(2 B).  mocca_ppo_grad's per-row lines -- logp in f64, r, the
 *                   surrogate, g, dL/dmu, the row's log_std term, the value loss with its clamp tie rule -- apply UNCHANGED to each
 *                   sample, one IEEE f32 operation per line, never contracted into an FMA.  log_std's gradient is the sum of g * q_j over
 *                   all 2 B samples minus f32(entropy_coef); H is the plain one.  Actor and critic both see the twins.
 *                   Copying old_logp to the twin is the METHOD's own assumption, that pi_old is close to mirror-symmetric: a twin's ratio
 *                   is pi(M_a a | M_o s) / pi_old(a | s), so the twins are OFF-POLICY by the policy's asymmetry -- their ratio leaves 1
 *                   and the clip range by as much as the policy is asymmetric --, and stats[7] below measures exactly that.  An exact
 *                   importance ratio, pi_old(M_a a | M_o s) computed at collection, is NOT offered: it would need a second old_logp
 *                   array through this call's and mocca_ppo_update's signature.
 *                   stats_dev [8]: [0..5] keep mocca_ppo_grad's meanings over the 2 B samples -- [4] the count of clipped samples of both
 *                   kinds divided by f32(2 B) --, [6] = 0, [7] = the twins' share of [3]: the sum over the B twins of old_logp - logp_twin
 *                   (summed like the other statistics), times ib; [3] - [7] is the as-given rows' share.
 *                   Scratch, the n_rows bound (2^21), the grow-FREES-the-old rule and the capture conditions are mocca_ppo_grad_sym's: twice
 *                   the plain call's scratch per row, shared by all four calls; a captured call holds the attachment's device tables:
 *                   mocca_set_policy_mirror_dup and mocca_set_policy ask for a new capture.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): those of mocca_ppo_grad with n_rows > 2^21 in place of 2^22; and a
 * handle WITHOUT duplicated rows attached (mocca_set_policy_mirror_dup). */
int mocca_ppo_grad_dup(mocca_handle h, const float *obs_dev, int obs_stride, const float *action_dev, const float *old_logp_dev,
                       const float *adv_dev, const float *returns_dev, const float *old_value_dev, const int64_t *idx_dev, int64_t n_rows,
                       double clip, double value_coef, double entropy_coef, int value_clip, float *grad_dev, float *stats_dev, void *stream);

/* ---- PPO's optimiser step and update loop on the device (no reference counterpart: the reference's trainers run clip_grad_norm_, Adam and
 *      the minibatch loop in torch and Python) ---- */

/* mocca_adam_step   replaces `nn.utils.clip_grad_norm_(params, max_grad_norm)`, `optimizer.step()` of torch.optim.Adam (no weight decay, no
 *                   amsgrad) and the mocca_update_policy that makes the step visible to the kernels -- three launches on `stream`.
 *                   params_dev [n_floats] f32: the flat tensor mocca_update_policy takes, in either of its two lengths, updated IN PLACE.
 *                   Its first n_params floats (1 .. n_head, n_head the length without mean / inv_std) are the trainable ones; n_head -
 *                   act_dim keeps log_std out of the norm and the step (a fixed action noise).  grad_dev: at least n_params f32 in the same
 *                   order (mocca_ppo_grad's grad_dev).  moments_dev f32 [2][n_head]: Adam's m, then v; caller-owned, fresh state zeros.
 *                   clock_dev f64 [4]: {t, beta1^t, beta2^t, skipped steps}; caller-owned, fresh state {0, 1, 1, 0}.
 *                   Launch A, one workgroup of 256: S = sum f64(g[i])^2 over i < n_params -- thread tid adds i = tid, tid + 256, ..
 *                   ascending, then the tree sq[tid] += sq[tid + h], h = 128 .. 1 -- and, in f64,
 *                       nrm = sqrt(S);  coef = max_grad_norm > 0 ? min(1, max_grad_norm / (nrm + 1e-6)) : 1, rounded once to f32
 *                   S not finite (a NaN or an infinity in the gradient): the step is SKIPPED -- clock[3] += 1; params, moments, t and the
 *                   two products stay bit for bit as they were, so that one bad minibatch does not poison a long run.  Otherwise
 *                       t += 1;  p1 = p1 * beta1;  p2 = p2 * beta2          (running products: every bit is defined without pow)
 *                       ss = f32(lr / (1 - p1));  bc = f32(sqrt(1 - p2));  b2 = f32(beta2);  w1 = f32(1 - beta1);  w2 = f32(1 - beta2);
 *                       e = f32(eps)
 *                   Launch B, one thread per trainable float, each line ONE IEEE f32 operation in this order, never contracted into an
 *                   FMA, square root and division correctly rounded:
 *                       g = grad[i] * coef
 *                       d = g - m;  d = d * w1;  m = m + d
 *                       v = v * b2;  q = g * g;  q = q * w2;  v = v + q
 *                       s = sqrtf(v);  s = s / bc;  s = s + e
 *                       u = m / s;  u = ss * u;  p = p - u
 *                   Launch C is mocca_update_policy's repack of params_dev, n_floats: the next mocca_act / mocca_ppo_grad on the stream
 *                   sees the step (and a call before any mocca_update_policy fills the image).  Floats of params_dev and moments_dev
 *                   beyond n_params are not touched.  Asynchronous on `stream`; the first call allocates a 32-byte record and the
 *                   gradient buffer of mocca_ppo_update in the handle and may synchronise, every other call allocates nothing, reads
 *                   nothing on the host and uses no atomics: after one warm call it is capturable in a hipGraph.  The clock is on the
 *                   device, so a replay advances it; lr, the betas, eps and max_grad_norm are kernel arguments and are BAKED INTO a
 *                   captured call -- a trainer that decays lr captures again or calls eagerly.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): a NULL handle, params_dev, grad_dev, moments_dev or clock_dev; called
 * before mocca_set_policy; n_floats that fits neither form; n_params outside 1 .. n_head; a non-finite or negative lr or eps; a beta outside
 * [0, 1); a NaN or negative max_grad_norm (0: no clip). */
int mocca_adam_step(mocca_handle h, float *params_dev, size_t n_floats, const float *grad_dev, int64_t n_params, float *moments_dev,
                    double *clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm, void *stream);

/* mocca_ppo_update  replaces a2c-ppo-acktr's `ppo.update(rollouts)`: epochs x M minibatches of [shuffle, gradient, clip, Adam, repack] in one
 *                   call, nothing read on the host.  R = n_rollout_rows, B = minibatch_rows, M = R / B minibatches per epoch, the
 *                   remainder dropped (`BatchSampler(.., drop_last=True)`).  The arrays obs_dev .. old_value_dev, clip, value_coef,
 *                   entropy_coef and value_clip are mocca_ppo_grad's; params_dev .. max_grad_norm are mocca_adam_step's.  Per epoch ONE
 *                   launch fills a handle-owned i64 [R] with a permutation of 0 .. R - 1; per minibatch u follow the four launches of
 *                   mocca_ppo_grad -- of mocca_ppo_grad_sym when the policy has mirror tables attached, of mocca_ppo_grad_mirror when a
 *                   mirror loss is attached, of mocca_ppo_grad_dup when duplicated rows are: this entry point serves all four --
 *                   with idx_dev = that array + u B and a handle-owned gradient [n_head], then mocca_adam_step's three launches on it.
 *                   The result is, bit for bit, what that sequence of calls gives.
 *                   The permutation is closed-form and defined in integers: w = max(2, bit_length(R - 1)) rounded up to even,
 *                   half = w / 2, mask = 2^half - 1.  One pass maps x = (L << half) | Rr through six Feistel rounds
 *                       (L, Rr) <- (Rr, L ^ (F & mask))
 *                       F = philox4x32(c0 = Rr, c1 = round, c2 = t mod 2^32, c3 = t >> 32, k0 = seed mod 2^32, k1 = seed >> 32)[0]
 *                   (Philox4x32-10); entry b starts at x = b and takes passes until x < R.  A pass is a bijection of 0 .. 2^w - 1, so the
 *                   walk returns below R and the entries are a bijection of 0 .. R - 1.  t is clock_dev[0] as the fill kernel READS IT ON
 *                   THE DEVICE when the epoch starts: a replayed graph shuffles anew, and a fresh clock with the same seed repeats a run.
 *                   stats_dev [epochs M][8] f32 or NULL: row k holds the k-th minibatch's mocca_ppo_grad statistics, with [6] overwritten
 *                   by the clip coefficient applied (0 on a skipped step) and [7] left as the gradient call wrote it (L_m with a mirror loss attached, the twins' share of [3] with duplicated rows, else
 *                   0); the trainer's `value_loss_epoch` etc. are the
 *                   rows' mean, and the rows' [3] is what a KL monitor reads.
 *                   params_dev must hold what mocca_update_policy (or mocca_adam_step) last wrote.  mocca_ppo_grad's conditions hold as
 *                   they stand -- growing either scratch FREES the old one: warm the handle with the largest B and R it will see --; the
 *                   call is a linear chain of epochs (1 + 7 M) launches on `stream`, capturable after one warm call of the same shapes,
 *                   with mocca_adam_step's scalars and `seed` baked in.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was and nothing is launched): those of mocca_adam_step and of mocca_ppo_grad
 * (/ mocca_ppo_grad_sym / mocca_ppo_grad_mirror / mocca_ppo_grad_dup) but for their grad_dev and idx_dev; minibatch_rows outside 1 .. n_rollout_rows; epochs < 1; n_rollout_rows < 1 or
 * beyond mocca_ppo_grad's bound (2^22, with mirror tables, a mirror loss or duplicated rows 2^21). */
int mocca_ppo_update(mocca_handle h, const float *obs_dev, int obs_stride, const float *action_dev, const float *old_logp_dev,
                     const float *adv_dev, const float *returns_dev, const float *old_value_dev, int64_t n_rollout_rows,
                     int64_t minibatch_rows, int epochs, double clip, double value_coef, double entropy_coef, int value_clip,
                     float *params_dev, size_t n_floats, int64_t n_params, float *moments_dev, double *clock_dev, double lr,
                     double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed, float *stats_dev, void *stream);

/* mocca_distill_grad  a regression (behaviour-cloning / DAgger) minibatch step on mocca_ppo_grad's machinery: the loss
 *                       L = distill_coef 1/(B A) sum_rows sum_j (mu_j - t_j)^2 + value_coef 0.5 mean_rows (v - vt)^2
 *                   -- torch's `distill_coef * (mean - target).pow(2).mean() + value_coef * 0.5 * (v - vt).pow(2).mean()` -- and its gradient
 *                   with respect to every parameter of the PLAIN policy, in the same four launches.  obs_dev, obs_stride, idx_dev (NOT
 *                   range-checked), n_rows = B, grad_dev's order and the forward (tanh rounded once) are mocca_ppo_grad's.  target_dev
 *                   [R][act_dim] f32: the actions to regress the actor's mean mu onto (a teacher's means, a controller's outputs);
 *                   value_target_dev [R] f32 or NULL: what the critic regresses onto.  Per row, each line ONE IEEE f32 operation in this
 *                   order, never contracted into an FMA (A = act_dim, t the row's targets):
 *                       ib = 1.0f / f32(B);  ia = 1.0f / f32(A);  k2 = f32(2 * distill_coef)   (the product in double)
 *                       for j ascending:   d = mu[j] - t[j];  q = d * d;  m = m + f64(q)
 *                                          u = d * ib;  u = u * ia;  dL/dmu[j] = u * k2
 *                       the row's distillation term = f32(m) * ia
 *                       value_target given:  e = v - vt;  l = e * e;  value loss = 0.5f * l;  dv = f32(value_coef) * e;  dL/dv = dv * ib
 *                       value_target NULL:   value loss = 0, dL/dv = 0: every entry of the critic's gradient is then exactly +0
 *                   log_std takes no gradient: its entries of grad_dev are exactly +0.0f.  Through the layers and in the sums the
 *                   arithmetic is mocca_ppo_grad's.  grad_dev [n_head] is fully overwritten.  stats_dev [8] f32 or NULL: 0, L_v, H as
 *                   mocca_ppo_grad forms it, 0, 0, the sum of grad_dev^2, 0, L_d = mean_rows mean_j (mu_j - t_j)^2 (the rows' terms
 *                   summed in f64 within a row chunk, the chunks' sums added in chunk order, times ib).
 *                   The scratch is mocca_ppo_grad's own (one buffer in the handle serves both calls; the same size for the same B), the
 *                   bound on n_rows 2^22, and mocca_ppo_grad's conditions hold as they stand: a call that grows the scratch FREES the old
 *                   one and may synchronise; every other call is asynchronous on `stream` and capturable after one warm call with the
 *                   same B; it reads the image mocca_update_policy last wrote and writes only grad_dev, stats_dev and its scratch.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was): a NULL handle; called before mocca_set_policy / mocca_update_policy; a
 * NULL obs_dev, target_dev or grad_dev; n_rows < 1 or > 2^22; obs_stride < in_dim; a non-finite or negative distill_coef or value_coef; a
 * handle with ANY mirror attachment (mocca_set_policy_symmetry, mocca_set_policy_mirror_loss, mocca_set_policy_mirror_dup) -- detach it:
 * distilling into a symmetric network is not provided. */
int mocca_distill_grad(mocca_handle h, const float *obs_dev, int obs_stride, const float *target_dev, const float *value_target_dev,
                       const int64_t *idx_dev, int64_t n_rows, double distill_coef, double value_coef, float *grad_dev, float *stats_dev,
                       void *stream);

/* mocca_distill_update  mocca_ppo_update's loop around mocca_distill_grad: `epochs` passes over R = n_rollout_rows stored rows, each a fresh
 *                   shuffle (the same Feistel permutation, keyed by `seed` and clock_dev[0] read on the device) cut into M = R / B
 *                   minibatches of B = minibatch_rows rows, the remainder dropped; per minibatch the four launches of mocca_distill_grad
 *                   with idx_dev = the permutation + u B and a handle-owned gradient, then mocca_adam_step's three launches.  Bit for
 *                   bit what that sequence of calls gives.  obs_dev .. value_target_dev, distill_coef and value_coef are
 *                   mocca_distill_grad's; params_dev .. max_grad_norm are mocca_adam_step's.  stats_dev [epochs M][8] f32 or NULL: row k
 *                   holds the k-th minibatch's mocca_distill_grad statistics with [6] overwritten by the clip coefficient applied.
 *                   mocca_ppo_update's conditions hold as they stand: a linear chain of epochs (1 + 7 M) launches, capturable after one
 *                   warm call of the same shapes.
 * Errors (MOCCA_E_ARG, with a message; the handle is left as it was and nothing is launched): those of mocca_adam_step and of
 * mocca_distill_grad but for their grad_dev and idx_dev; minibatch_rows outside 1 .. n_rollout_rows; epochs < 1; n_rollout_rows < 1 or > 2^22. */
int mocca_distill_update(mocca_handle h, const float *obs_dev, int obs_stride, const float *target_dev, const float *value_target_dev,
                         int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double distill_coef, double value_coef,
                         float *params_dev, size_t n_floats, int64_t n_params, float *moments_dev, double *clock_dev, double lr,
                         double beta1, double beta2, double eps, double max_grad_norm, uint64_t seed, float *stats_dev, void *stream);

/* mocca_set_teacher   a SECOND, independent policy image in the handle: a frozen teacher that labels the rows a student visits.  The layer
 *                   table, in_dim, act_dim, clip and every shape check are mocca_set_policy's; layers_host NULL detaches.  The teacher may
 *                   differ from the policy of mocca_set_policy in in_dim and in layers.  It takes no mirror attachment, and nothing done to
 *                   it touches that policy, its mirror attachment, mocca_act's results or the gradient calls'.  May synchronise.
 * mocca_update_teacher  the teacher's weights, as mocca_update_policy takes the policy's: params_dev of either length (with or without
 *                   mean / inv_std), one repack launch on `stream`, nothing synchronises.
 * mocca_teacher_act   the teacher's actor mean and value on n_rows rows in ONE launch of the policy kernel's plain instance, deterministic:
 *                   the arithmetic of mocca_act with deterministic = 1 (with the same weights, the same bits).  in_dev [n_rows][in_stride]
 *                   f32, the first in_dim floats of a row are read; n_rows is any count >= 1 (at most 2^22), not tied to n_envs: the
 *                   deterministic path reads no env record.  mean_dev [n_rows][act_dim]; value_dev [n_rows] or NULL (the critic is then
 *                   not run).  No allocation, no synchronisation, no host read: capturable.
 * Errors (MOCCA_E_ARG, with a message): mocca_set_teacher / mocca_update_teacher: those of mocca_set_policy / mocca_update_policy.
 * mocca_teacher_act: called before mocca_set_teacher and mocca_update_teacher; a NULL in_dev or mean_dev; in_stride < in_dim; n_rows < 1. */
int mocca_set_teacher(mocca_handle h, const int32_t *layers_host, int n_layers_total, int in_dim, int act_dim, double clip);
int mocca_update_teacher(mocca_handle h, const float *params_dev, size_t n_floats, void *stream);
int mocca_teacher_act(mocca_handle h, const float *in_dev, int in_stride, int64_t n_rows, float *mean_dev, float *value_dev, void *stream);

/* ---- PPO with a privileged critic (an asymmetric actor-critic; no reference counterpart: the reference's trainers give both nets one
 *      observation) ---- */

/* The critic is a training-time device and is thrown away at deployment, so it may read what the robot will never have: the simulator's
 * exact geometry (TorchVecEnv's `envs.privileged`, [obs | scan]).  The actor keeps reading what the robot really has.  PPO's loss separates
 * -- the surrogate and the entropy depend on the actor and log_std alone, the value term on the critic alone -- and every sum's order is a
 * function of B and the shapes alone, so each output below is, BIT FOR BIT, an output of the existing calls on a suitable plain policy:
 * action, logp, mean and the actor's / log_std's gradient those of a plain policy with the same actor on the actor's rows; the value and the
 * critic's gradient those of a plain policy of in_dim = critic_in_dim with the same critic on the critic's rows; likewise stats[0..4] and
 * [7].  stats[5], the sum of grad_dev^2, is the only statistic of the gradient call that mixes both nets (and, in the update's rows, [6],
 * the clip coefficient formed from it).  Arithmetic and layout: csrc/mocca_policy.h and csrc/mocca_ppo.h, Privileged critic.
 *
 * mocca_set_policy_priv   mocca_set_policy with the critic's FIRST layer taking critic_in_dim inputs (1 .. 336; it may equal in_dim, be
 *                       smaller or larger): the same table, the same rules, the actor's first layer takes in_dim.  The image gains the
 *                       critic's statistics, and the parameter vector of mocca_update_policy / mocca_adam_step is: the layers, log_std,
 *                       then optionally mean[in_dim], inv_std[in_dim], critic_mean[critic_in_dim], critic_inv_std[critic_in_dim] -- ALL
 *                       FOUR OR NONE: n_floats is n_head or n_head + 2 in_dim + 2 critic_in_dim.  One device flag word switches the
 *                       normalisation of both nets; the critic's is clamp((x - critic_mean[k]) * critic_inv_std[k], -clip, +clip), the
 *                       same f32 operations in the same order with the same clip.  layers_host == NULL detaches.  mocca_set_policy on
 *                       the same handle returns it to a plain policy; either call drops the binding of mocca_set_critic_rows.  May
 *                       synchronise.
 *                       NOT PROVIDED with a privileged critic: the three mirror attachments (mirror tables for the critic's row are a
 *                       later addition) -- mocca_set_policy_symmetry / _mirror_loss / _mirror_dup refuse on such a policy and
 *                       mocca_set_policy_priv refuses while one of them is attached, each with a message, the caller detaches first --;
 *                       distillation INTO such a policy (mocca_distill_grad / mocca_distill_update refuse).  mocca_set_teacher,
 *                       mocca_update_teacher and mocca_teacher_act are untouched: a teacher is a plain policy.
 * mocca_set_critic_rows   binds the rows the critic's workgroups of mocca_act / mocca_act_step / mocca_act_plan_step read: rows_dev
 *                       [n_envs][row_stride] f32, CALLER-owned (`envs.privileged`), the first critic_in_dim floats of row i belong to env
 *                       i.  A fixed address, read at every launch: the three calls stay capturable (mocca_set_terminal_obs_buffer is
 *                       the precedent).  rows_dev == NULL detaches.  With value_dev NULL the critic is not run and no binding is needed.
 * mocca_ppo_grad_priv     mocca_ppo_grad for such a policy: its argument list with critic_obs_dev [R][critic_stride] f32 added, the
 *                       storage's critic rows, RAW, gathered through the same idx_dev (NOT range-checked); the four launches, the per-row
 *                       lines, grad_dev's order (the critic's first W is [out][critic_in_dim]) and stats_dev are mocca_ppo_grad's.
 *                       Scratch: mocca_ppo_grad's plus 4 B critic_in_pad bytes (the critic's normalised input), the handle's one
 *                       buffer: the grow-FREES-the-old rule and the capture conditions hold as they stand.  n_rows 1 .. 2^22.
 * mocca_ppo_update_priv   mocca_ppo_update for such a policy: its argument list with critic_obs_dev, critic_stride added; bit for bit the
 *                       sequence mocca_ppo_grad_priv + mocca_adam_step per minibatch, under the same shuffle.
 * Errors (MOCCA_E_ARG, with a message; the handle and every output are left as they were, nothing is launched): mocca_set_policy_priv:
 * those of mocca_set_policy, critic_in_dim outside 1 .. 336, a critic whose first layer does not take critic_in_dim, a mirror attachment
 * in place.  mocca_set_critic_rows: a NULL handle, a policy without a privileged critic (or none), row_stride < critic_in_dim.  mocca_act /
 * mocca_act_step / mocca_act_plan_step: value_dev asked for on such a policy with no rows bound.  mocca_set_policy_symmetry /
 * _mirror_loss / _mirror_dup: a policy with a privileged critic.  mocca_ppo_grad_priv / mocca_ppo_update_priv: those of mocca_ppo_grad /
 * mocca_ppo_update, a NULL critic_obs_dev, critic_stride < critic_in_dim, a policy WITHOUT a privileged critic (mocca_ppo_grad /
 * mocca_ppo_update are its calls).  mocca_ppo_grad / _sym / _mirror / _dup, mocca_ppo_update, mocca_distill_grad and mocca_distill_update on
 * a policy WITH one: the message names mocca_ppo_grad_priv / mocca_ppo_update_priv; distillation into such a policy is not provided. */
int mocca_set_policy_priv(mocca_handle h, const int32_t *layers_host, int n_layers_total, int in_dim, int critic_in_dim, int act_dim,
                          double clip);
int mocca_set_critic_rows(mocca_handle h, const float *rows_dev, int row_stride);
int mocca_ppo_grad_priv(mocca_handle h, const float *obs_dev, int obs_stride, const float *critic_obs_dev, int critic_stride,
                        const float *action_dev, const float *old_logp_dev, const float *adv_dev, const float *returns_dev,
                        const float *old_value_dev, const int64_t *idx_dev, int64_t n_rows, double clip, double value_coef,
                        double entropy_coef, int value_clip, float *grad_dev, float *stats_dev, void *stream);
int mocca_ppo_update_priv(mocca_handle h, const float *obs_dev, int obs_stride, const float *critic_obs_dev, int critic_stride,
                          const float *action_dev, const float *old_logp_dev, const float *adv_dev, const float *returns_dev,
                          const float *old_value_dev, int64_t n_rollout_rows, int64_t minibatch_rows, int epochs, double clip,
                          double value_coef, double entropy_coef, int value_clip, float *params_dev, size_t n_floats, int64_t n_params,
                          float *moments_dev, double *clock_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm,
                          uint64_t seed, float *stats_dev, void *stream);

/* ---- domain randomisation on the device: motor strength, action latency, pushes, sensor noise (no reference counterpart: the reference's
 *      robot has the same dynamics in every env and every episode) ---- */

/* These entry points are ADDITIVE: MOCCA_ABI_VERSION stays 8, and a handle that calls none of them launches and computes exactly what it
 * did before.  Nothing here touches the step kernel: everything acts on its inputs and outputs -- the action buffer it reads, the state
 * record it loads, the observation row it wrote.  Arithmetic, keying and kernel layout: mocca_envs_amd/csrc/mocca_randomise.h.
 *
 * Keying.  Every draw is Philox4x32-10 under the handle's seed key (MOCCA_PARAM_SEED / mocca_reset), with the counter (g, c1, E, c3):
 * g = MOCCA_PARAM_ENV_OFFSET + env, the GLOBAL env id; E the env's episode counter (task word MOCCA_TW_EPISODE); c1 = 0 or the env's step
 * counter T (task word MOCCA_TW_T); both counters READ FROM THE TASK RECORD WHEN THE KERNEL RUNS.  Nothing is kept on the host: every launch
 * below can be captured in a hipGraph, a shard reproduces the rows it owns, and a restored task record (mocca_set_task) restores the draws.
 * c3 = domain + 256 b with the domains 4 and 5 (0 .. 3 are the envs' own draws, policy noise, the field choice and the terrain generator:
 * no other draw moves) and a block index b.  A uniform is u = (w >> 8) 2^-24, a signed uniform s = 2 u - 1.
 *     episode parameters  (g, 0, E, 4):          strength = fmaf(u0, strength_hi - strength_lo, strength_lo)
 *                                                 delay = delay_min + (w1 >> 8) % (delay_max - delay_min + 1)
 *                                                 phase = (w2 >> 8) % push_interval
 *     the push of step T  (g, T, E, 4 + 256):    dvx = push_max s0, dvy = push_max s1
 *     noise of column k   (g, T, E, 5 + 256 (k / 4)), word k % 4:  out[k] = fmaf(scale[k], s, row[k])
 *
 * mocca_set_randomisation  attaches (cfg == NULL: detaches) the randomisation of the PLANT.  From then on every launch of the step kernel --
 *                   mocca_step, mocca_plan_step, mocca_act_step, mocca_act_plan_step -- is preceded, on the same stream, by ONE small launch
 *                   that reads the action buffer the step kernel would have read (the caller's, the policy's output or the base
 *                   controller's) and writes a handle-owned effective-action buffer [N][act_dim], which the step kernel reads instead.
 *                   Nothing is launched without an attachment.  Per env:
 *                     motor strength   v = strength * clip(a, -1, 1), the clip as the step kernel spells it (a NaN passes through).  The
 *                                      step computes gain * applied_gain * clip(.), so v scales the torque; the step's energy penalty, which
 *                                      reads the same buffer, sees v as well.  MOCCA_TASK_CASSIE takes the range [1, 1] ALONE: its action
 *                                      is a PD target, not a torque (the clip to [-1, 1] applies there too).
 *                     latency          a handle-owned ring [N][delay_max + 1][act_dim]: slot T % (delay_max + 1) receives v, and the
 *                                      effective action is the v stored at step T - delay when T >= delay, else 0.  Indexed by T: a reset --
 *                                      mocca_reset or the auto-reset inside the step kernel -- needs no clearing pass.  THE RING IS NOT
 *                                      PART OF THE mocca_get_state / mocca_get_task SNAPSHOT: a restored snapshot with delay > 0 reads, for
 *                                      its first `delay` steps, whatever the ring held; mocca_task_step advances T without writing it.
 *                     pushes           push_interval > 0, T > 0 and (T + phase) % push_interval == 0: dvx and dvy are added to words 7 and
 *                                      8 of the env's state record, the base's linear velocity in the world frame.  The Walker2D and Crab2D
 *                                      topologies and blobs with planar != 0 take dvx alone (the draw is taken, word 8 is not written).
 *                                      The planner's base controller reads the robot state the previous step left: IT SEES A PUSH ONE
 *                                      STEP LATE.
 *                   May allocate and synchronise; no step ever does.  mocca_task_step has no physics and is not perturbed.  One handle:
 *                   the multi-handle wrappers of the Python layer do not offer it.
 * mocca_get_effective_action  out_dev [N][act_dim] <- what the last step's kernel read; one copy on `stream`.
 * mocca_set_sensor_noise   scale_host [dim] f32, dim = obs_dim, copied into the handle (NULL detaches); may synchronise.
 * mocca_sensor_noise       out_dev[e][k] = fmaf(scale[k], s, rows_dev[e][k]) for k < dim, rows in_stride / out_stride floats apart; in place is
 *                   allowed (out_dev == rows_dev with equal strides), columns at or beyond dim are not written.  T and E are the env's
 *                   counters NOW -- after the step that wrote the row --, so two calls without a step in between give the same rows.
 * mocca_randomisation_record  out_dev[e][0 .. 3] <- strength, delay, steps until the env's next push (0: the next step is pushed; -1: no
 *                   pushes), 0 -- a pure function of the task record's E and T, so the row describes the episode the env is in now, also
 *                   right after an auto-reset.  Rows row_stride floats apart (the tail of a privileged critic's row).
 * The three launches allocate nothing, read nothing on the host, use no atomics and do not synchronise.
 * Errors (MOCCA_E_ARG, with a message, before any launch; the handle and every output are left as they were): mocca_set_randomisation: a
 * strength range outside (0, 1] or reversed; one other than [1, 1] on MOCCA_TASK_CASSIE; negative or reversed delays, delay_max >
 * MOCCA_RAND_MAX_DELAY; a negative or non-finite push_max; push_interval outside 0 .. 65536.  mocca_set_sensor_noise: dim != obs_dim, a
 * negative or non-finite scale.  mocca_sensor_noise before mocca_set_sensor_noise, mocca_randomisation_record / mocca_get_effective_action
 * before mocca_set_randomisation; a NULL pointer; in_stride or out_stride < obs_dim, row_stride < MOCCA_RAND_WORDS. */
#define MOCCA_RAND_WORDS 4
#define MOCCA_RAND_MAX_DELAY 7
typedef struct mocca_randomisation {
  float strength_lo, strength_hi; /* per-episode motor strength, 0 < lo <= hi <= 1 */
  int32_t delay_min, delay_max;   /* per-episode action latency in steps, 0 <= min <= max <= MOCCA_RAND_MAX_DELAY */
  int32_t push_interval;          /* steps between pushes, 0 (none) .. 65536; each episode draws its phase */
  float push_max;                 /* largest |dvx|, |dvy| of a push, m/s */
} mocca_randomisation;
int mocca_set_randomisation(mocca_handle h, const mocca_randomisation *cfg);
int mocca_get_effective_action(mocca_handle h, float *out_dev, void *stream);
int mocca_set_sensor_noise(mocca_handle h, const float *scale_host, int dim);
int mocca_sensor_noise(mocca_handle h, const float *rows_dev, int in_stride, float *out_dev, int out_stride, void *stream);
int mocca_randomisation_record(mocca_handle h, float *out_dev, int row_stride, void *stream);

/* ---- observation-action history on the training path (no reference counterpart) ---- */

/* These entry points are ADDITIVE: MOCCA_ABI_VERSION stays 8, and a handle that calls none of them launches exactly what it launched before.
 * Nothing here touches the step kernel.  A feed-forward actor on the current row cannot tell which plant it has (mocca_set_randomisation):
 * strength and delay show only in what was commanded against what happened over the last few steps.  mocca_history writes that -- past
 * observations and past actions -- as the tail of the policy's row, one launch, capturable.  Index rules, race argument and kernel layout:
 * mocca_envs_amd/csrc/mocca_history.h.
 *
 * The rule.  Configuration: K = steps, 1 .. MOCCA_HIST_MAX_STEPS; s = stride, 1 .. MOCCA_HIST_MAX_STRIDE; an ordered list of C distinct
 * observation columns cols[0 .. C), 0 <= C <= obs_dim; an action width A, 0 .. 32; C + A >= 1; block width K (C + A) <= MOCCA_HIST_MAX_DIM.
 * Per env the handle owns a ring of R = K s + 1 slots of C + A floats and a tag of two uint32 per slot.  At attach time the ring is zeroed
 * and every tag is set to a value no episode holds (t = 0xFFFFFFFF).  mocca_history is ONE launch; per env, with t the task word MOCCA_TW_T
 * and E the task word MOCCA_TW_EPISODE, both READ FROM THE TASK RECORD WHEN THE KERNEL RUNS (nothing is kept on the host), it
 *   1. stores the current frame: in slot t % R the observation part takes rows[e][cols[0 .. C)], the action part +0.0, the tag (E, t);
 *   2. completes the previous frame: if t >= 1, act_dev != NULL and the tag of slot (t - 1) % R equals (E, t - 1), the action part of that
 *      slot takes act[e][0 .. A);
 *   3. emits the block, NEWEST FIRST: pair j = 1 .. K sits at offset (j - 1)(C + A) and is [o_u[cols] | a_u] with u = t - j s -- the
 *      observation the policy read j s steps ago and the action it then output.  A pair is valid iff t >= j s and the tag of slot u % R
 *      equals (E, u); an invalid pair is C + A words of +0.0.  A valid pair comes from the ring, except the action part when j s == 1: it is
 *      taken from act[e] directly (+0.0 when act_dev == NULL).
 * No thread reads a ring word that another thread of the same launch writes: the launch writes slot t % R and the action part of slot
 * (t - 1) % R; step 3 reads slots of u = t - j s with 1 <= j s <= R - 1, never slot t % R; of slot (t - 1) % R it reads the tag and the
 * observation part, which an earlier launch wrote, and takes the action part -- the one word being written -- from act[e] instead.
 * Consequences: the ring is indexed by T and tagged by (E, T), so mocca_reset, the step kernel's auto-reset and a mocca_set_task that moves T
 * need no clearing pass: an episode only ever reads what it wrote itself.  A call that was skipped shows up as a zero pair, never as
 * another episode's data.  Two calls without a step in between write and emit the same words.  Everything is a copy or a zero.
 * Limits: THE RING IS NOT PART OF THE mocca_get_state / mocca_get_task SNAPSHOT -- a restored task record that returns to an (E, T) the ring
 * has already seen reads those frames; mocca_task_step advances T without a history call.
 *
 * mocca_set_history  attaches (steps == 0: detaches; the other arguments are then not read) the history: cols_host [n_cols] int32 is copied
 *                   into the handle, act_dim is A (the env's action width, the plan's on a planner env, or 0).  May allocate and
 *                   synchronise.  One handle: the multi-handle wrappers of the Python layer do not offer it.
 * mocca_history_dim  steps * (n_cols + act_dim).
 * mocca_history      rows_dev: the policy's rows, row_stride floats apart, columns 0 .. obs_dim - 1 read; act_dev: the action the policy output
 *                   on the PREVIOUS row (what the step that led here ran on), act_stride floats apart, or NULL (after a reset); out_dev: the
 *                   block's first float, rows out_stride floats apart.  rows_dev and out_dev may lie in the same row (in place: head columns
 *                   are read, tail columns written; the block must not overlap the columns read).  Floats of a row outside the block are
 *                   never written.  Allocates nothing, reads nothing on the host, uses no atomics and does not synchronise.
 * Errors (MOCCA_E_ARG, with a message, before any launch; the handle and every output are left as they were): mocca_set_history: a column
 * outside 0 .. obs_dim - 1 or repeated; steps, stride, act_dim or the block width out of range; n_cols + act_dim == 0.  mocca_history and
 * mocca_history_dim without an attachment; mocca_history: a NULL rows_dev or out_dev, row_stride < obs_dim, out_stride <
 * mocca_history_dim, act_stride < act_dim with a non-NULL act_dev. */
#define MOCCA_HIST_MAX_STEPS 16
#define MOCCA_HIST_MAX_STRIDE 8
#define MOCCA_HIST_MAX_DIM 1024
int mocca_set_history(mocca_handle h, const int32_t *cols_host, int n_cols, int act_dim, int steps, int stride); /* steps == 0 detaches */
int mocca_history_dim(mocca_handle h);   /* steps * (n_cols + act_dim); MOCCA_E_ARG without an attachment */
int mocca_history(mocca_handle h, const float *rows_dev, int row_stride, const float *act_dev /* may be NULL */, int act_stride,
                  float *out_dev, int out_stride, void *stream);

/* ---- per-env adaptive curriculum of the Stepper envs on the device (the reference's trainer moves ONE level for all envs from the
 *      host, set_env_params({"curriculum": k}); here every env earns its own) ---- */

/* These entry points are ADDITIVE: MOCCA_ABI_VERSION stays 8, and a handle that calls none of them launches and computes exactly what it
 * did before.  Nothing here touches the step kernel: at every reset it already reads a per-env level from the vector of
 * mocca_set_param_v(MOCCA_PARAM_CURRICULUM) -- terrain ranges and applied gain follow at reset, the terminal height at once -- and every step
 * it already writes done and the info word (steps_reached).  What is added is the rule that turns an env's own episode outcomes into its
 * own level, one small launch behind the step, so that no trainer reads episode records in the middle of a rollout.  The rule, the
 * ownership argument and the kernel layout: mocca_envs_amd/csrc/mocca_curriculum.h.
 *
 * The rule.  State per env, owned by the handle: the level -- the f32 word of that vector, the single source of truth and the very word
 * the step kernel reads --, streak (int32) and hold (int32, 0 or 1).  ONE launch; every env whose done byte is non-zero, s its info word:
 *   1. hold != 0: hold <- 0 and NOTHING ELSE.  The auto-reset inside the step kernel runs before this launch, so when a level changes the
 *      env's next episode already stands on terrain of the old level: a new level first shapes the episode AFTER next.  The episode in
 *      flight at a change is neither judged nor counted.
 *   2. L = the vector's word read as the step kernel reads it: truncated to int, clamped to 0 .. 9.
 *   3. with totals attached: totals[L] += {1, s, success ? 1 : 0, failure ? 1 : 0} (f32 atomics on whole numbers: exact and order-free
 *      below 2^24).
 *   4. success, s >= promote_at: streak <- max(streak, 0) + 1; at streak >= patience: streak <- 0, and L' = L + 1 if L < max_level, else with
 *      recycle L' = min_level + ((uint64(w) * (max_level - min_level + 1)) >> 32), else L' = L.
 *   5. failure, s <= demote_at: streak <- min(streak, 0) - 1; at streak <= -patience: streak <- 0, L' = max(L - 1, min_level).
 *   6. neither: streak <- 0.
 *   7. L' != L: the vector's word <- (float)L', hold <- 1.
 * The recycle draw: w is word 0 of Philox4x32-10 under the handle's seed key with the counter (g, 0, E, 6): g = MOCCA_PARAM_ENV_OFFSET + env,
 * E the env's episode counter (task word MOCCA_TW_EPISODE) READ FROM THE TASK RECORD WHEN THE KERNEL RUNS.  Domain 6 in counter word 3 is new:
 * 0 .. 3 are the envs' own draws, policy noise, the field choice and the terrain generator, 4 and 5 the randomisation's; no other draw
 * moves.  Nothing is kept on the host: the launch can be captured in a hipGraph and a shard reproduces its envs.
 * Each thread owns its env: no thread reads a word another thread of the launch writes; the totals are only added to, atomically.
 *
 * mocca_set_curriculum  attaches (cfg == NULL: detaches) the rule.  Attaching switches the level vector on: it starts from the vector where
 *                   that is on already, else from the scalar level broadcast, clamped into [min_level, max_level]; streak and hold start
 *                   at 0.  level_totals_dev: [10][4] f32 per level {episodes judged, sum of steps_reached, successes, failures}, caller-
 *                   owned, zeroed by the caller when it likes, or NULL.  While attached and MOCCA_PARAM_AUTO_RESET is 1, mocca_step and
 *                   mocca_act_step enqueue the rule's launch directly behind the step kernel on the step's stream (where info_dev is
 *                   NULL the step writes its info words to a buffer of the handle's): policy and step stay one call, a rollout stays
 *                   one graph, and a graph captured after attaching replays the rule.  With auto-reset off nothing is launched: done is
 *                   sticky there, and counting episode ends is the caller's, through mocca_curriculum_apply.  While attached the scalar
 *                   mocca_set_param(MOCCA_PARAM_CURRICULUM) is refused -- it would drop the vector --: mocca_set_param_v with broadcast
 *                   does the same job.  mocca_set_param_v keeps working; A HOST WRITE OF LEVELS IS JUDGED AS IF THE LEVEL HAD ALWAYS
 *                   BEEN THAT: streak and hold stay as they are.  Detaching leaves the levels in the vector and takes the scalar again.
 *                   May allocate and synchronise; no step does.
 * mocca_get_curriculum  level_dev / streak_dev / hold_dev: [N] int32 each or NULL; one launch on `stream`, no synchronise.
 * mocca_curriculum_apply  the same kernel on the caller's done bytes [N] u8 and info words [N] i32: for callers with a loop of their own.
 * Limits: STREAK, HOLD AND THE VECTOR ARE NOT PART OF THE mocca_get_state / mocca_get_task SNAPSHOT.  The planner ids are out of scope:
 * difficulty bands of the terrain bank would need the field choice in the step kernel's reset to change.  One handle: the multi-handle
 * wrappers of the Python layer do not offer it.
 * Errors (MOCCA_E_ARG, with a message, before any launch; the handle is left as it was): mocca_set_curriculum on a task other than
 * MOCCA_TASK_WALKER3D_STEPPER (the quadruped and Mike Stepper ids are that task); demote_at >= promote_at; patience outside 1 ..
 * MOCCA_CUR_MAX_PATIENCE; levels outside 0 <= min_level <= max_level <= MOCCA_CUR_MAX_LEVEL; recycle other than 0 or 1.
 * mocca_get_curriculum / mocca_curriculum_apply without an attachment; mocca_curriculum_apply: a NULL done_dev or info_dev. */
#define MOCCA_CUR_MAX_LEVEL 9
#define MOCCA_CUR_MAX_PATIENCE 64
typedef struct mocca_curriculum {
  int32_t promote_at, demote_at; /* an episode with steps_reached >= promote_at is a success, <= demote_at a failure; demote_at < promote_at */
  int32_t patience;              /* that many successes (failures) in a row move the level up (down), 1 .. MOCCA_CUR_MAX_PATIENCE */
  int32_t min_level, max_level;  /* 0 <= min_level <= max_level <= MOCCA_CUR_MAX_LEVEL */
  int32_t recycle;               /* 1: an env promoted at max_level restarts at a level drawn uniformly from the band */
} mocca_curriculum;
int mocca_set_curriculum(mocca_handle h, const mocca_curriculum *cfg, float *level_totals_dev /* [10][4] or NULL, caller-owned */);
int mocca_get_curriculum(mocca_handle h, int32_t *level_dev, int32_t *streak_dev, int32_t *hold_dev, void *stream);
int mocca_curriculum_apply(mocca_handle h, const uint8_t *done_dev, const int32_t *info_dev, void *stream);

/* registers, LDS and scratch of the step kernel as built (for DESIGN.md / bench), as the HIP runtime reports them; *sgprs = -1: the
 * runtime has no scalar-register attribute (hipFuncAttributes), the count is printed by `python -m mocca_envs_amd.build -v` */
int mocca_kernel_info(mocca_handle h, int *vgprs, int *sgprs, int *lds_bytes, int *scratch_bytes, int *max_blocks_per_cu);

const char *mocca_last_error(mocca_handle h);

#ifdef __cplusplus
}
#endif
#endif /* MOCCA_H */
