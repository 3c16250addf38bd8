// mocca_curriculum.h -- the per-env adaptive curriculum of the Stepper envs (include/mocca.h mocca_set_curriculum, mocca_curriculum_apply):
// the rule that turns an env's own episode outcomes into its own level, on the device, behind the step.  The level is the f32 word of the
// handle's per-env vector (MOCCA_PARAM_CURRICULUM's, mocca_set_param_v) that the step kernel's reset already reads; nothing here touches
// the step kernel.  The rule and the work of one thread are ONE set of functions for the device and the host: this header compiles as
// plain C++ without HIP, so a CPU test pins it, bit for bit, against the numpy restatement (tests/test_curriculum.py,
// tests/curriculum_reference.py).
//
// The rule.  Configuration: promote_at > demote_at, patience 1 .. 64, 0 <= min_level <= max_level <= 9, recycle 0 or 1.  Per env the handle
// owns the level (the vector's f32 word), streak (int32) and hold (int32, 0 or 1).  ONE launch per call; every env whose done byte is
// non-zero, with s its info word (the Stepper's steps_reached):
//     1. hold != 0:  hold <- 0 and NOTHING ELSE.  The step kernel's auto-reset runs inside the step, before this launch: when a level
//                    changes, the env's next episode already stands on terrain of the old level, so a new level first shapes the episode
//                    AFTER next.  The episode in flight at a change is not judged, and not counted.
//     2. L = the vector's word as the step kernel's live_curriculum reads it: truncated to int, clamped to 0 .. 9.
//     3. totals != NULL:  totals[L] += {1, s, success ? 1 : 0, failure ? 1 : 0}  (f32 atomics on whole numbers: exact and order-free below 2^24)
//     4. success, s >= promote_at:  streak <- max(streak, 0) + 1; at streak >= patience: streak <- 0 and L' = L + 1 if L < max_level, else with
//                    recycle L' = min_level + ((uint64(w) * (max_level - min_level + 1)) >> 32), else L' = L.
//     5. failure, s <= demote_at:   streak <- min(streak, 0) - 1; at streak <= -patience: streak <- 0 and L' = max(L - 1, min_level).
//     6. neither:    streak <- 0.
//     7. L' != L:    the vector's word <- (float)L', hold <- 1.
// The recycle draw.  w is word 0 of Philox4x32-10 under the handle's seed key with the counter (g, 0, E, 6): g = env_offset + env the GLOBAL
// env id, E the env's episode counter (task word MOCCA_TW_EPISODE) READ FROM THE TASK RECORD WHEN THE KERNEL RUNS -- nothing is kept on the
// host, so the launch can be captured in a graph and a shard reproduces its envs.  Counter word 3 holds the domain: 0 the envs' own draws,
// 1 policy noise, 2 field choice, 3 the terrain generator, 4 and 5 the randomisation's (mocca_randomise.h); 6 is this file's.
// No thread reads a word another thread of the launch writes: thread e reads and writes level[e], streak[e], hold[e] and reads done[e],
// info[e] and env e's task record -- each thread owns its env.  The totals are only ever added to, by atomics.
// A host write of levels (mocca_set_param_v) while attached is judged as if the level had always been that: streak and hold stay.
// Limits.  streak, hold and the vector are NOT part of the mocca_get_state / mocca_get_task snapshot.
//
// Layout of the kernel (mocca_curriculum.hip): one THREAD per env, 256 to a workgroup; a thread loads its done byte and leaves when it is
// zero -- all but a few envs of a step.  Plain vector loads and stores, no allocation, no host read; the only atomics are the totals'.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MOCCA_CUR_HD __host__ __device__ inline
#else
#define MOCCA_CUR_HD inline
#endif

namespace mocca_cur {

constexpr int CUR_MAX_LEVEL = 9;          // = MOCCA_CUR_MAX_LEVEL
constexpr int CUR_MAX_PATIENCE = 64;      // = MOCCA_CUR_MAX_PATIENCE
constexpr int CUR_LEVELS = 10, CUR_TOTALS = 4;   // totals [CUR_LEVELS][CUR_TOTALS]: episodes, sum of steps_reached, successes, failures
constexpr uint32_t CUR_DOMAIN = 6u;       // counter word 3 of the recycle draw

// what mocca_set_curriculum holds, as the kernel takes it
struct CurConfig {
  int promote_at, demote_at, patience, min_level, max_level, recycle;
};

// mocca_philox.h's philox4x32 for both sides (that header is device-only), word 0
MOCCA_CUR_HD uint32_t cur_philox0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// the level a vector word stands for, spelled as the step kernel's live_curriculum (mocca_device.h)
MOCCA_CUR_HD int cur_level(float v) {
  const int c = (int)v;
  return c < 0 ? 0 : (c > CUR_MAX_LEVEL ? CUR_MAX_LEVEL : c);
}
// the level a recycled env restarts at: uniform over min_level .. max_level from the word w
MOCCA_CUR_HD int cur_recycled(const CurConfig& c, uint32_t w) {
  return c.min_level + (int)(((uint64_t)w * (uint64_t)(c.max_level - c.min_level + 1)) >> 32);
}
MOCCA_CUR_HD uint32_t cur_draw(uint32_t g, uint32_t episode, uint32_t k0, uint32_t k1) { return cur_philox0(g, 0u, episode, CUR_DOMAIN, k0, k1); }

// the totals take whole numbers: atomics on the device (threads of a launch share a level's row), plain sums on the host
MOCCA_CUR_HD void cur_add(float* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}

// thread `env` of an env whose done byte is non-zero: s its info word, g its global id, *episode_word its task word MOCCA_TW_EPISODE (read
// only where a draw is taken), level / streak / hold its own words, totals [CUR_LEVELS][CUR_TOTALS] or null
MOCCA_CUR_HD void cur_thread(const CurConfig& c, int s, uint32_t g, const uint32_t* episode_word, uint32_t k0, uint32_t k1, float* level,
                             int32_t* streak, int32_t* hold, float* totals) {
  if (*hold) { *hold = 0; return; }                                                 // 1
  const int L = cur_level(*level);                                                  // 2
  const bool success = s >= c.promote_at, failure = s <= c.demote_at;
  if (totals) {                                                                     // 3
    float* row = totals + L * CUR_TOTALS;
    cur_add(row + 0, 1.0f); cur_add(row + 1, (float)s);
    if (success) cur_add(row + 2, 1.0f);
    if (failure) cur_add(row + 3, 1.0f);
  }
  int next = L, run = *streak;
  if (success) {                                                                    // 4
    run = (run > 0 ? run : 0) + 1;
    if (run >= c.patience) {
      run = 0;
      if (L < c.max_level) next = L + 1;
      else if (c.recycle) next = cur_recycled(c, cur_draw(g, *episode_word, k0, k1));
    }
  } else if (failure) {                                                             // 5
    run = (run < 0 ? run : 0) - 1;
    if (run <= -c.patience) {
      run = 0;
      next = L - 1 > c.min_level ? L - 1 : c.min_level;
    }
  } else {                                                                          // 6
    run = 0;
  }
  *streak = run;
  if (next != L) { *level = (float)next; *hold = 1; }                               // 7
}

// the level mocca_set_curriculum starts an env at: what it had (the vector's word, or the scalar level), clamped into the band
MOCCA_CUR_HD int cur_start(const CurConfig& c, int level) { return level < c.min_level ? c.min_level : (level > c.max_level ? c.max_level : level); }

#if defined(__HIPCC__)
struct CurArgs {
  CurConfig cfg;
  const uint32_t* task;   // the task records: E is read when the kernel runs
  int task_words, tw_episode;
  int env_offset, n_envs;
  uint32_t seed_lo, seed_hi;
  const uint8_t* done;    // [N] the step's done bytes
  const int32_t* info;    // [N] the step's info words
  float* level;           // [N] the handle's level vector, the words the step kernel reads
  int32_t* streak;        // [N]
  int32_t* hold;          // [N]
  float* totals;          // [CUR_LEVELS][CUR_TOTALS] or null
};
constexpr int CUR_THREADS = 256;
void launch_curriculum(hipStream_t s, const CurArgs& a);
// mocca_set_curriculum: level[e] <- cur_start of (from_vector ? the word's level : scalar)
void launch_curriculum_start(hipStream_t s, const CurConfig& c, float* level, int from_vector, int scalar, int n_envs);
// mocca_get_curriculum: each output [N] int32 or null
void launch_curriculum_get(hipStream_t s, const float* level, const int32_t* streak, const int32_t* hold, int n_envs, int32_t* level_out,
                           int32_t* streak_out, int32_t* hold_out);
#endif

}  // namespace mocca_cur
