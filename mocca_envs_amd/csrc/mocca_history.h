// mocca_history.h -- the observation-action history of the policy's row (include/mocca.h mocca_set_history, mocca_history): the tail
// [o_{t-s} a_{t-s} | o_{t-2s} a_{t-2s} | ...] that lets a feed-forward actor compare what it commanded with what happened -- the only way it can
// tell a weak motor or a late command (mocca_randomise.h) from the plain plant.  Nothing here touches the step kernel.  The index rules --
// slot, tag match, pair validity, the source of every word -- and the work of one thread are ONE set of functions for the device and the
// host: this header compiles as plain C++ without HIP, so a CPU test pins it, bit for bit, against the numpy restatement
// (tests/test_history.py, tests/history_reference.py).
//
// The rule.  K = steps (1 .. 16), s = stride (1 .. 8), C distinct observation columns cols[0 .. C) (0 <= C <= obs_dim), A action entries
// (0 .. 32), C + A >= 1, block width K (C + A) <= 1024.  Per env the handle owns a ring of R = K s + 1 slots of C + A floats and a tag of two
// uint32 per slot; at attach time the ring is zero and every tag word is 0xFFFFFFFF, a step counter no episode holds.  ONE launch per call;
// per env, with t = task word MOCCA_TW_T and E = task word MOCCA_TW_EPISODE READ FROM THE TASK RECORD WHEN THE KERNEL RUNS (nothing is
// kept on the host: the launch is capturable):
//     1. store the current frame      slot t % R: observation part <- rows[e][cols[0 .. C)], action part <- +0.0, tag <- (E, t)
//     2. complete the previous frame  t >= 1, act != NULL and tag of slot (t - 1) % R == (E, t - 1): its action part <- act[e][0 .. A)
//     3. emit the block, newest first pair j = 1 .. K at offset (j - 1)(C + A) is [o_u[cols] | a_u], u = t - j s: the observation the policy
//                                     read j s steps ago and the action it then output.  Valid iff t >= j s and tag of slot u % R == (E, u);
//                                     an invalid pair is C + A words of +0.0.  A valid pair comes from the ring, EXCEPT the action part
//                                     when j s == 1: that is act[e] itself (+0.0 when act == NULL).
// No thread reads a ring word another thread of the same launch writes.  The launch writes slot t % R (all of it, and its tag) and the
// action part of slot (t - 1) % R.  Step 3 reads the slots and tags of u = t - j s with 1 <= j s <= K s = R - 1: u and t differ by less than R,
// so u % R != t % R and slot t % R, tag included, is never read.  Slot (t - 1) % R is read by step 2 (its tag) and by step 3 when j s == 1 (its
// tag and its observation part): neither is written by this launch, an earlier launch on the stream wrote them.  Its action part, which
// this launch does write, is the one word step 3 does not take from the ring: it takes act[e], the value being written.  Every other slot
// step 3 reads lies two or more steps back and is not written at all.
// Consequences.  The ring is indexed by T and tagged by (E, T): mocca_reset, the step kernel's auto-reset and a mocca_set_task that moves T
// need no clearing pass -- an episode only ever reads what it wrote itself; a skipped call shows up as a zero pair, never as another
// episode's data; two calls without a step in between write and emit the same words.  Everything is a copy or a zero.
// Limits.  The ring is NOT part of the mocca_get_state / mocca_get_task snapshot: a restored task record that returns to an (E, T) the ring
// has already seen reads those frames.  mocca_task_step advances T without a history call.
//
// Layout of the kernel (mocca_history.hip), as mocca_randomise.hip argues it: one THREAD per output float, 256 to a workgroup, envs packed
// back to back -- rows are tens to hundreds of floats, a wave per env would leave lanes idle.  Thread (e, w), w < K (C + A), emits word w of
// env e's block; the threads of pair 1 (w < C + A) also do the ring writes of steps 1 and 2 for their column, thread w == 0 the tag.  Stores
// run along rows; no atomics, no allocation, no host read, no synchronise.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MOCCA_HIST_HD __host__ __device__ inline
#else
#define MOCCA_HIST_HD inline
#endif

namespace mocca_hist {

constexpr int HIST_MAX_STEPS = 16;     // = MOCCA_HIST_MAX_STEPS
constexpr int HIST_MAX_STRIDE = 8;     // = MOCCA_HIST_MAX_STRIDE
constexpr int HIST_MAX_DIM = 1024;     // = MOCCA_HIST_MAX_DIM
constexpr int HIST_MAX_ACT = 32;
constexpr uint32_t HIST_NO_T = 0xFFFFFFFFu;   // the step counter of a tag no episode holds

// what mocca_set_history holds, as the kernel takes it
struct HistConfig {
  int steps, stride, n_cols, act_dim;
};
MOCCA_HIST_HD int hist_width(const HistConfig& c) { return c.n_cols + c.act_dim; }          // floats of a pair, and of a ring slot
MOCCA_HIST_HD int hist_slots(const HistConfig& c) { return c.steps * c.stride + 1; }        // R
MOCCA_HIST_HD int hist_dim(const HistConfig& c) { return c.steps * hist_width(c); }         // floats of the block

// the slot of step t (t is taken as the unsigned word it is: whatever a restored task record holds, a slot lies inside the ring)
MOCCA_HIST_HD int hist_slot(const HistConfig& c, uint32_t t) { return (int)(t % (uint32_t)hist_slots(c)); }
// does the slot of step u hold the frame (episode, u)?  tags: the env's [R][2]
MOCCA_HIST_HD bool hist_tag_is(const HistConfig& c, const uint32_t* tags, uint32_t episode, uint32_t u) {
  const uint32_t* tag = tags + 2 * hist_slot(c, u);
  return tag[0] == episode && tag[1] == u;
}
// pair j = 1 .. K as the step counter stands at t: the step u it shows, and whether the ring holds it
MOCCA_HIST_HD uint32_t hist_pair_step(const HistConfig& c, uint32_t t, int j) { return t - (uint32_t)(j * c.stride); }
MOCCA_HIST_HD bool hist_pair_valid(const HistConfig& c, const uint32_t* tags, uint32_t episode, uint32_t t, int j) {
  return t >= (uint32_t)(j * c.stride) && hist_tag_is(c, tags, episode, hist_pair_step(c, t, j));
}
// where entry p of a VALID pair j comes from (an invalid pair is HIST_ZERO throughout)
enum HistSource { HIST_ZERO = 0, HIST_RING = 1, HIST_ACT = 2 };
MOCCA_HIST_HD HistSource hist_source(const HistConfig& c, int j, int p, bool have_act) {
  if (p >= c.n_cols && j * c.stride == 1) return have_act ? HIST_ACT : HIST_ZERO;   // the word this launch writes: never read back
  return HIST_RING;
}

// thread (env, w): row, act (or null), ring [R][C + A], tags [R][2] and out are the env's own; t and episode its task words
MOCCA_HIST_HD void hist_thread(const HistConfig& c, uint32_t t, uint32_t episode, const float* row, const float* act, const int32_t* cols,
                               float* ring, uint32_t* tags, float* out, int w) {
  const int width = hist_width(c);
  const int j = w / width + 1, p = w - (j - 1) * width;
  // step 3 first: its loads are independent of the stores below (see the argument above)
  float v = 0.0f;
  if (hist_pair_valid(c, tags, episode, t, j)) {
    const HistSource src = hist_source(c, j, p, act != nullptr);
    if (src == HIST_RING) v = ring[hist_slot(c, hist_pair_step(c, t, j)) * width + p];
    else if (src == HIST_ACT) v = act[p - c.n_cols];
  }
  if (j == 1) {   // the ring writes of column p
    float* now = ring + hist_slot(c, t) * width;
    now[p] = p < c.n_cols ? row[cols[p]] : 0.0f;                                                        // step 1
    if (p >= c.n_cols && t >= 1u && act != nullptr && hist_tag_is(c, tags, episode, t - 1u))           // step 2
      ring[hist_slot(c, t - 1u) * width + p] = act[p - c.n_cols];
    if (p == 0) {
      uint32_t* tag = tags + 2 * hist_slot(c, t);
      tag[0] = episode; tag[1] = t;
    }
  }
  out[w] = v;
}

#if defined(__HIPCC__)
struct HistArgs {
  HistConfig cfg;
  const uint32_t* task;   // the task records: T and E are read when the kernel runs
  int task_words, tw_t, tw_episode;
  int n_envs;
  const int32_t* cols;    // [n_cols]
  float* ring;            // [N][R][C + A]
  uint32_t* tags;         // [N][R][2]
  const float* rows;      // the policy's rows, head columns read
  const float* act;       // [N] rows of act_stride floats, or null
  float* out;             // the block's first column, rows out_stride floats apart
  int row_stride, act_stride, out_stride;
};
constexpr int HIST_THREADS = 256;
void launch_history(hipStream_t s, const HistArgs& a);
#endif

}  // namespace mocca_hist
