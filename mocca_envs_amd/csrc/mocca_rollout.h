// mocca_rollout.h -- what a PPO trainer does between collecting a rollout and learning from it, as kernels (mocca_rollout.hip), and their
// host-side launchers.  mocca_gae / mocca_obs_stats (mocca_api_trainer.hip) check the caller's arguments, own the scratch and launch them.
//
// GAE (a2c-ppo-acktr's rollouts.compute_returns(use_gae, use_proper_time_limits=True) and the advantage normalisation of ppo.update).
// Storage [T][N] / [T + 1][N] f32, contiguous.  One IEEE f32 operation per line element, in this order, never contracted into an FMA:
//     g = f32(gamma); c = f32(gamma * lam, the product in double); s = f32(reward_scale); gae = 0
//     for t = T - 1 .. 0:
//         delta  = ((r[t] * s) + ((g * v[t + 1]) * m[t + 1])) - v[t]
//         gae    = (delta + ((c * m[t + 1]) * gae)) * bm[t + 1]
//         adv[t] = gae;  ret[t] = gae + v[t]
// Launch 1 (gae_kernel): one thread per env, GAE_BLOCK envs per workgroup; a thread also sums its T advantages and their squares in f64,
// the workgroup adds its threads' sums in a fixed order (a shuffle tree inside each wave, the waves in index order) and writes ONE pair per
// workgroup to `partials` [n_blocks][2].  No float atomics anywhere: the sum's order is a function of (T, N) alone, so two runs give the
// same bits.
// Launch 2 (moments_kernel): every workgroup adds the pairs in index order in f64 (S1, S2), forms, with B = T N,
//     mean = f32(S1 / B)        std = f32(sqrt(max(S2 - S1 S1 / B, 0) / (B - 1)))        (Bessel, as torch's .std(); NaN for B = 1)
// workgroup 0 writes moments[0..1] = mean, std, and with normalise != 0 all of them rewrite adv <- (adv - mean) / (std + f32(adv_eps)) in
// f32, the division correctly rounded.  With normalise == 0 the launch has one workgroup and only writes the moments.
//
// Running observation statistics (VecNormalize's ob_rms.update; baselines' RunningMeanStd).  state f64 [1 + 2 dim] = count, mean[dim],
// var[dim].  Rows [n_rows][row_stride] f32, the first dim floats of a row are loaded, nothing beyond them.
// Launch 1 (obs_partials_kernel): a workgroup takes a contiguous chunk of rows.  Its OBS_BLOCK threads are (sub-row, feature) with the
// feature fastest, so a wave loads along a row; a thread sums d = f64(x) - mean_old[k] and d d over its rows of the chunk in f64, the
// sub-rows of a feature are added in index order, and the workgroup writes one (sum d, sum d d) per feature: partials [n_blocks][dim][2].
// Launch 2 (obs_merge_kernel): ONE workgroup.  Thread (group, feature) adds a contiguous range of the blocks' pairs in block order, the
// groups are added in index order, and the thread of feature k merges in f64, n = n_rows:
//     bm = mean + Sd / n;  bv = Sdd / n - (Sd / n)^2;  delta = bm - mean;  tot = count + n
//     mean' = mean + delta n / tot;   var' = (var count + bv n + delta^2 count n / tot) / tot;   count' = tot
// writes the state back and mean_out[k] = f32(mean'), inv_std_out[k] = 1.0f / sqrtf(f32(var') + f32(eps)) (policy.py's f32 formula; square
// root and division correctly rounded) where the pointers are not null.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocca_ro {

constexpr int GAE_BLOCK = 256;        // envs per workgroup of the GAE kernel
constexpr int GAE_UNROLL = 8;         // steps whose loads are issued together
constexpr int NORM_BLOCK = 256;       // threads per workgroup of the moments / normalise kernel
constexpr int NORM_PER_THREAD = 4;    // advantages a thread of it rewrites per grid stride
constexpr int NORM_MAX_BLOCKS = 2048;
constexpr int OBS_BLOCK = 256;        // threads per workgroup of the statistics' first launch
constexpr int OBS_MAX_DIM = 336;      // POL_MAX_IN (mocca_policy.h)
constexpr int OBS_MAX_BLOCKS = 512;   // row chunks (pairs per feature the merge kernel adds)
constexpr int OBS_MIN_PASSES = 8;     // a chunk holds at least this many rows per thread
constexpr int OBS_MERGE_BLOCK = 1024;

struct GaeArgs {
  const float *rew, *value, *masks, *bad_masks;   // [T][N], [T + 1][N] x 3
  float *returns, *adv;                           // [T][N] or null
  double* partials;                               // [n_blocks][2]
  int n_envs, n_steps;
  float g, c, s;
};
struct MomentsArgs {
  const double* partials;
  int n_partials;
  long long count;            // B = T N
  float* adv;                 // rewritten when normalise
  float* moments;             // [2] or null
  float eps;
  int normalise;
};
struct ObsArgs {
  const float* rows;
  long long n_rows;
  int row_stride, dim;
  long long rows_per_block;
  int n_blocks;
  double* state;              // [1 + 2 dim]
  double* partials;           // [n_blocks][dim][2]
  float eps;
  float *mean_out, *inv_std_out;
};

inline int gae_blocks(int n_envs) { return (n_envs + GAE_BLOCK - 1) / GAE_BLOCK; }
// features a workgroup's threads span (a power of two up to OBS_BLOCK; dim > OBS_BLOCK: a thread takes features k and k + OBS_BLOCK)
inline int obs_span(int dim, int block) {
  int f = 1;
  while (f < dim && f < block) f *= 2;
  return f;
}
// the first launch's grid: rows per workgroup (a multiple of the sub-rows of one pass) and workgroups
inline void obs_grid(long long n_rows, int dim, long long* rows_per_block, int* n_blocks) {
  const long long sub = OBS_BLOCK / obs_span(dim, OBS_BLOCK);
  long long rpb = (n_rows + OBS_MAX_BLOCKS - 1) / OBS_MAX_BLOCKS;
  if (rpb < sub * OBS_MIN_PASSES) rpb = sub * OBS_MIN_PASSES;
  rpb = (rpb + sub - 1) / sub * sub;
  *rows_per_block = rpb;
  *n_blocks = (int)((n_rows + rpb - 1) / rpb);
}

void launch_gae(hipStream_t s, const GaeArgs& a);
void launch_moments(hipStream_t s, const MomentsArgs& a);
void launch_obs_stats(hipStream_t s, const ObsArgs& a);

}  // namespace mocca_ro
