// mocca_curriculum.hip -- the kernels of the per-env adaptive curriculum (include/mocca.h mocca_set_curriculum; the rule, the ownership
// argument and the work of one thread are mocca_curriculum.h).  One thread per env, 256 to a workgroup: a thread loads its done byte and
// leaves when it is zero, which is all but a few envs of a step.  Plain vector loads and stores, no allocation, no host read; the only
// atomics are the optional totals': the launch is capturable.
#include "mocca_curriculum.h"

namespace mocca_cur {

__global__ __launch_bounds__(CUR_THREADS) void curriculum_kernel(CurArgs a) {
  const int env = (int)blockIdx.x * CUR_THREADS + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  if (!a.done[env]) return;
  cur_thread(a.cfg, a.info[env], (uint32_t)a.env_offset + (uint32_t)env, a.task + (size_t)env * a.task_words + a.tw_episode, a.seed_lo, a.seed_hi,
             a.level + env, a.streak + env, a.hold + env, a.totals);
}

__global__ __launch_bounds__(CUR_THREADS) void curriculum_start_kernel(CurConfig c, float* level, int from_vector, int scalar, int n_envs) {
  const int env = (int)blockIdx.x * CUR_THREADS + (int)threadIdx.x;
  if (env >= n_envs) return;
  level[env] = (float)cur_start(c, from_vector ? cur_level(level[env]) : scalar);
}

__global__ __launch_bounds__(CUR_THREADS) void curriculum_get_kernel(const float* level, const int32_t* streak, const int32_t* hold, int n_envs,
                                                                     int32_t* level_out, int32_t* streak_out, int32_t* hold_out) {
  const int env = (int)blockIdx.x * CUR_THREADS + (int)threadIdx.x;
  if (env >= n_envs) return;
  if (level_out) level_out[env] = cur_level(level[env]);
  if (streak_out) streak_out[env] = streak[env];
  if (hold_out) hold_out[env] = hold[env];
}

static dim3 cur_grid(int n_envs) { return dim3((unsigned)((n_envs + CUR_THREADS - 1) / CUR_THREADS)); }

void launch_curriculum(hipStream_t s, const CurArgs& a) {
  hipLaunchKernelGGL(curriculum_kernel, cur_grid(a.n_envs), dim3(CUR_THREADS), 0, s, a);
}
void launch_curriculum_start(hipStream_t s, const CurConfig& c, float* level, int from_vector, int scalar, int n_envs) {
  hipLaunchKernelGGL(curriculum_start_kernel, cur_grid(n_envs), dim3(CUR_THREADS), 0, s, c, level, from_vector, scalar, n_envs);
}
void launch_curriculum_get(hipStream_t s, const float* level, const int32_t* streak, const int32_t* hold, int n_envs, int32_t* level_out,
                           int32_t* streak_out, int32_t* hold_out) {
  hipLaunchKernelGGL(curriculum_get_kernel, cur_grid(n_envs), dim3(CUR_THREADS), 0, s, level, streak, hold, n_envs, level_out, streak_out, hold_out);
}

}  // namespace mocca_cur
