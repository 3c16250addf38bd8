// mocca_randomise.h -- domain randomisation on the device (include/mocca.h mocca_set_randomisation, mocca_set_sensor_noise): per-episode motor
// strength and action latency, random pushes of the base, additive sensor noise, and the record that tells a privileged critic which plant
// an env has.  Everything acts on what the step kernel reads and writes -- the action buffer, the state record, the observation row --; the
// step kernel itself is untouched.  The arithmetic of every draw is ONE set of functions for the device and the host: this header compiles
// as plain C++ without HIP, so a CPU test pins it, bit for bit, against the numpy restatement (tests/test_randomisation.py).
//
// Keying.  All draws are Philox4x32-10 under the handle's seed key (seed low, seed high), the generator of mocca_philox.h (restated below
// for the host).  The counter is (g, c1, E, c3): g = env_offset + env the GLOBAL env id, E the env's episode counter (task word
// MOCCA_TW_EPISODE), c1 = 0 or the env's step counter T (task word MOCCA_TW_T), both read from the task record AT LAUNCH TIME -- nothing is
// kept on the host, so every launch can be captured in a graph, and a shard reproduces the rows it owns.  Counter word 3 holds the domain:
// 0 the envs' own draws, 1 policy noise, 2 field choice, 3 the terrain generator; this file takes 4 and 5, with a block index b in the upper
// bits, c3 = domain + 256 b (6 is the adaptive curriculum's recycle draw, mocca_curriculum.h).  A uniform is u = (w >> 8) * 2^-24, a signed uniform s = 2 u - 1 (both exact in f32).
//     episode parameters   (g, 0, E, 4)            strength = fmaf(u0, hi - lo, lo);  delay = delay_min + (w1 >> 8) % (delay_max - delay_min + 1);
//                                                  phase = (w2 >> 8) % push_interval   (integers: a float product can round up to the bound)
//     push at step T       (g, T, E, 4 + 256)      dvx = push_max * s0;  dvy = push_max * s1
//     noise of column k    (g, T, E, 5 + 256 (k / 4))   word k % 4:  out[k] = fmaf(scale[k], s, row[k])
//
// The perturb kernel (in front of every step-kernel launch of a handle with a randomisation attached) per env:
//     strength   c = clip(a, -1, 1) as the step kernel spells it (a NaN passes through); v = strength * c, one multiply.  The step computes
//                gain * applied_gain * clip(.), so v scales the torque.  The step kernel's energy penalty reads the same buffer: it sees v.
//     latency    a handle-owned ring [N][delay_max + 1][act_dim]: slot T % (delay_max + 1) receives v; the effective action is the value
//                stored at step T - delay when T >= delay, else 0.  Indexed by T, so no reset -- the step kernel's auto-reset included --
//                needs a clearing pass: an episode only ever reads slots it has written itself.
//     pushes     push_interval > 0, T > 0 and (T + phase) % push_interval == 0: dvx, dvy are added to words 7 and 8 of the env's state
//                record (the base's linear velocity, world frame).  Planar mechanisms (the Walker2D and Crab2D topologies, blobs with
//                planar != 0) take dvx alone: the draw is still taken, word 8 is not written.  The planner's robot_state buffer is NOT
//                touched: the base controller sees a push ONE STEP LATE, in the robot state the pushed step leaves behind.
// The record (RAND_WORDS floats per env: strength, delay, steps until the next push or -1, 0) is a pure function of E and T as the task
// record holds them, so it describes the episode the env is in NOW, also right after an auto-reset.
//
// Layout of the kernels (mocca_randomise.hip): one THREAD per float, 256 to a workgroup, envs packed back to back -- the rows are 4 to 65
// floats, and a wave per env would leave two thirds of its lanes idle at act_dim 21.  A thread recomputes its env's Philox block (a few
// dozen integer instructions against the memory latency it waits for anyway); stores run along rows; no atomics, no allocation, no host read.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MOCCA_RAND_HD __host__ __device__ inline
#else
#define MOCCA_RAND_HD inline
#endif
// every product below is ONE rounding: nothing is contracted into a fused multiply-add but the fmaf calls that say so
#if defined(__clang__)
#define MOCCA_RAND_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MOCCA_RAND_NO_CONTRACT
#endif

namespace mocca_rand {

constexpr int RAND_WORDS = 4;            // = MOCCA_RAND_WORDS
constexpr int RAND_MAX_DELAY = 7;        // = MOCCA_RAND_MAX_DELAY
constexpr int RAND_MAX_INTERVAL = 65536;
constexpr uint32_t RAND_DOMAIN_PLANT = 4u, RAND_DOMAIN_NOISE = 5u;   // counter word 3, low byte
constexpr uint32_t RAND_BLOCK = 256u;                                // ... and the stride of the block index above it
enum : uint32_t { RAND_BLOCK_EPISODE = 0u, RAND_BLOCK_PUSH = 1u };

// mocca_philox.h's philox4x32 for both sides (that header is device-only)
MOCCA_RAND_HD void rand_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

MOCCA_RAND_HD float rand_uniform(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
MOCCA_RAND_HD float rand_signed(uint32_t w) { MOCCA_RAND_NO_CONTRACT return 2.0f * rand_uniform(w) - 1.0f; }   // exact: 2 u has 24 bits below 2

// what mocca_set_randomisation holds, as the kernels take it
struct RandConfig {
  float strength_lo, strength_hi;
  int delay_min, delay_max;
  int push_interval;      // 0: no pushes
  float push_max;
  int planar;             // the mechanism moves in the x-z plane: dvy is forced to 0
};
struct EpisodeParams {
  float strength;
  int delay, phase;
};

MOCCA_RAND_HD EpisodeParams rand_episode(const RandConfig& c, uint32_t g, uint32_t episode, uint32_t k0, uint32_t k1) {
  uint32_t w[4];
  rand_philox(g, 0u, episode, RAND_DOMAIN_PLANT + RAND_BLOCK * RAND_BLOCK_EPISODE, k0, k1, w);
  EpisodeParams p;
  p.strength = fmaf(rand_uniform(w[0]), c.strength_hi - c.strength_lo, c.strength_lo);
  p.delay = c.delay_min + (int)((w[1] >> 8) % (uint32_t)(c.delay_max - c.delay_min + 1));
  p.phase = c.push_interval > 0 ? (int)((w[2] >> 8) % (uint32_t)c.push_interval) : 0;
  return p;
}

// the clip of the step kernel's apply_action, spelled as there: a NaN passes through
MOCCA_RAND_HD float rand_clip(float a) { return a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a); }
MOCCA_RAND_HD float rand_stored(float strength, float a) { MOCCA_RAND_NO_CONTRACT return strength * rand_clip(a); }

// the ring: slot of step T, and the slot the effective action of step T is read from (-1: none yet, the effective action is 0)
// (T is taken as the unsigned word it is: whatever a restored task record holds, a slot lies inside the ring)
MOCCA_RAND_HD int rand_slot(const RandConfig& c, uint32_t t) { return (int)(t % (uint32_t)(c.delay_max + 1)); }
MOCCA_RAND_HD int rand_read_slot(const RandConfig& c, uint32_t t, int delay) {
  return t >= (uint32_t)delay ? (int)((t - (uint32_t)delay) % (uint32_t)(c.delay_max + 1)) : -1;
}

MOCCA_RAND_HD bool rand_push_fires(const RandConfig& c, uint32_t t, int phase) {
  return c.push_interval > 0 && t > 0u && (t + (uint32_t)phase) % (uint32_t)c.push_interval == 0u;
}
// the velocity step of the push at step T: dv[0] along x, dv[1] along y (0 for a planar mechanism; the draw is taken all the same)
MOCCA_RAND_HD void rand_push(const RandConfig& c, uint32_t g, uint32_t t, uint32_t episode, uint32_t k0, uint32_t k1, float* dv) {
  MOCCA_RAND_NO_CONTRACT
  uint32_t w[4];
  rand_philox(g, t, episode, RAND_DOMAIN_PLANT + RAND_BLOCK * RAND_BLOCK_PUSH, k0, k1, w);
  dv[0] = c.push_max * rand_signed(w[0]);
  dv[1] = c.planar ? 0.0f : c.push_max * rand_signed(w[1]);
}
// steps until the next push as the step counter stands at T: 0 when the next step's launch pushes; -1 without pushes
MOCCA_RAND_HD int rand_until_push(const RandConfig& c, uint32_t t, int phase) {
  if (c.push_interval <= 0) return -1;
  const uint32_t t0 = t > 1u ? t : 1u, r = (t0 + (uint32_t)phase) % (uint32_t)c.push_interval;
  return (int)(t0 - t) + (r ? c.push_interval - (int)r : 0);
}
// word `word` of the env's record
MOCCA_RAND_HD float rand_record(const RandConfig& c, const EpisodeParams& p, uint32_t t, int word) {
  switch (word) {
    case 0: return p.strength;
    case 1: return (float)p.delay;
    case 2: return (float)rand_until_push(c, t, p.phase);
    default: return 0.0f;
  }
}

// column k of a noisy row
MOCCA_RAND_HD float rand_noise(float row, float scale, int k, uint32_t g, uint32_t t, uint32_t episode, uint32_t k0, uint32_t k1) {
  uint32_t w[4];
  rand_philox(g, t, episode, RAND_DOMAIN_NOISE + RAND_BLOCK * (uint32_t)(k >> 2), k0, k1, w);
  return fmaf(scale, rand_signed(w[k & 3]), row);
}

#if defined(__HIPCC__)
// what every launch reads of the handle: the task records for T and E, the key, the global id of env 0
struct RandKeys {
  const uint32_t* task;
  int task_words, tw_t, tw_episode;
  int env_offset, n_envs;
  uint32_t seed_lo, seed_hi;
};
struct PerturbArgs {
  RandKeys keys;
  RandConfig cfg;
  const float* act;     // [N][act_dim] what the step kernel would have read
  float* eff;           // [N][act_dim] what it reads instead
  float* ring;          // [N][delay_max + 1][act_dim]
  float* dyn;           // the state records; words 7, 8 take the push
  int dyn_stride, act_dim;
};
struct NoiseArgs {
  RandKeys keys;
  const float* scale;   // [dim]
  const float* rows;
  float* out;
  int in_stride, out_stride, dim;
};
struct RecordArgs {
  RandKeys keys;
  RandConfig cfg;
  float* out;
  int row_stride;
};
constexpr int RAND_THREADS = 256;
void launch_perturb(hipStream_t s, const PerturbArgs& a);
void launch_noise(hipStream_t s, const NoiseArgs& a);
void launch_record(hipStream_t s, const RecordArgs& a);
#endif

}  // namespace mocca_rand
