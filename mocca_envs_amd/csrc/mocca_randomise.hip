// mocca_randomise.hip -- the three kernels of the domain randomisation (include/mocca.h mocca_set_randomisation, mocca_sensor_noise,
// mocca_randomisation_record; the arithmetic and the keying are mocca_randomise.h).  Small memory-bound kernels over 4 to 65 floats per env:
// one thread per float, 256 to a workgroup, the envs' rows packed back to back, so that every lane but the last workgroup's tail has a
// float (a wave per env would idle 43 of 64 lanes at act_dim 21).  A thread forms its env's Philox block itself.  Stores run along rows;
// no atomics, no allocation, no host read: every launch is capturable.
#include "mocca_randomise.h"

namespace mocca_rand {

struct EnvKey {
  uint32_t g, t, episode;
};
__device__ __forceinline__ EnvKey env_key(const RandKeys& k, int env) {
  const uint32_t* tk = k.task + (size_t)env * k.task_words;
  return EnvKey{(uint32_t)(k.env_offset + env), tk[k.tw_t], tk[k.tw_episode]};
}

// in front of the step kernel: act -> ring -> eff, and the push into the state record.  Thread (env, j): column j of env's action.
__global__ __launch_bounds__(RAND_THREADS) void perturb_kernel(PerturbArgs a) {
  MOCCA_RAND_NO_CONTRACT
  const int i = (int)blockIdx.x * RAND_THREADS + (int)threadIdx.x;
  if (i >= a.keys.n_envs * a.act_dim) return;
  const int env = i / a.act_dim, j = i - env * a.act_dim;
  const EnvKey k = env_key(a.keys, env);
  const EpisodeParams p = rand_episode(a.cfg, k.g, k.episode, a.keys.seed_lo, a.keys.seed_hi);
  const float v = rand_stored(p.strength, a.act[i]);
  float* ring = a.ring + (size_t)env * (a.cfg.delay_max + 1) * a.act_dim;
  ring[rand_slot(a.cfg, k.t) * a.act_dim + j] = v;
  const int rs = rand_read_slot(a.cfg, k.t, p.delay);
  // delay 0 reads the slot this thread has just written; an older slot was written by an earlier launch on the stream
  a.eff[i] = rs < 0 ? 0.0f : (p.delay == 0 ? v : ring[rs * a.act_dim + j]);
  // the push: columns 0 and 1 carry dvx and dvy (a one-column action: column 0 carries both)
  if (j < 2 && rand_push_fires(a.cfg, k.t, p.phase)) {
    float dv[2];
    rand_push(a.cfg, k.g, k.t, k.episode, a.keys.seed_lo, a.keys.seed_hi, dv);
    float* st = a.dyn + (size_t)env * a.dyn_stride;
    if (j == 0) st[7] = st[7] + dv[0];
    if ((j == 1 || a.act_dim == 1) && !a.cfg.planar) st[8] = st[8] + dv[1];
  }
}

// out[env][k] = fmaf(scale[k], s, rows[env][k]) for k < dim; in place is allowed (a thread reads and writes its own float alone)
__global__ __launch_bounds__(RAND_THREADS) void sensor_noise_kernel(NoiseArgs a) {
  const int i = (int)blockIdx.x * RAND_THREADS + (int)threadIdx.x;
  if (i >= a.keys.n_envs * a.dim) return;
  const int env = i / a.dim, c = i - env * a.dim;
  const EnvKey k = env_key(a.keys, env);
  a.out[(size_t)env * a.out_stride + c] =
      rand_noise(a.rows[(size_t)env * a.in_stride + c], a.scale[c], c, k.g, k.t, k.episode, a.keys.seed_lo, a.keys.seed_hi);
}

// thread (env, w): word w of env's record
__global__ __launch_bounds__(RAND_THREADS) void record_kernel(RecordArgs a) {
  const int i = (int)blockIdx.x * RAND_THREADS + (int)threadIdx.x;
  if (i >= a.keys.n_envs * RAND_WORDS) return;
  const int env = i / RAND_WORDS, w = i % RAND_WORDS;
  const EnvKey k = env_key(a.keys, env);
  const EpisodeParams p = rand_episode(a.cfg, k.g, k.episode, a.keys.seed_lo, a.keys.seed_hi);
  a.out[(size_t)env * a.row_stride + w] = rand_record(a.cfg, p, k.t, w);
}

static dim3 grid_for(long long floats) { return dim3((unsigned)((floats + RAND_THREADS - 1) / RAND_THREADS)); }

void launch_perturb(hipStream_t s, const PerturbArgs& a) {
  hipLaunchKernelGGL(perturb_kernel, grid_for((long long)a.keys.n_envs * a.act_dim), dim3(RAND_THREADS), 0, s, a);
}
void launch_noise(hipStream_t s, const NoiseArgs& a) {
  hipLaunchKernelGGL(sensor_noise_kernel, grid_for((long long)a.keys.n_envs * a.dim), dim3(RAND_THREADS), 0, s, a);
}
void launch_record(hipStream_t s, const RecordArgs& a) {
  hipLaunchKernelGGL(record_kernel, grid_for((long long)a.keys.n_envs * RAND_WORDS), dim3(RAND_THREADS), 0, s, a);
}

}  // namespace mocca_rand
