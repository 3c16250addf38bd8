// mocca_history.hip -- the kernel of the observation-action history (include/mocca.h mocca_history; the rule, the race argument and the work
// of one thread are mocca_history.h).  A small kernel bound by memory latency over K (C + A) floats per env: one thread per output float, 256
// to a workgroup, the envs' blocks packed back to back, so that every lane but the last workgroup's tail has a float.  A thread reads its
// env's two task words itself; stores run along rows; no atomics, no allocation, no host read: the launch is capturable.
#include "mocca_history.h"

namespace mocca_hist {

// thread (env, w): word w of env's block; the threads of pair 1 also write the ring (mocca_history.h hist_thread)
__global__ __launch_bounds__(HIST_THREADS) void history_kernel(HistArgs a) {
  const int dim = hist_dim(a.cfg);
  const int i = (int)blockIdx.x * HIST_THREADS + (int)threadIdx.x;
  if (i >= a.n_envs * dim) return;
  const int env = i / dim, w = i - env * dim;
  const uint32_t* tk = a.task + (size_t)env * a.task_words;
  const size_t slots = (size_t)hist_slots(a.cfg);
  hist_thread(a.cfg, tk[a.tw_t], tk[a.tw_episode], a.rows + (size_t)env * a.row_stride, a.act ? a.act + (size_t)env * a.act_stride : nullptr,
              a.cols, a.ring + (size_t)env * slots * hist_width(a.cfg), a.tags + (size_t)env * slots * 2, a.out + (size_t)env * a.out_stride, w);
}

void launch_history(hipStream_t s, const HistArgs& a) {
  const long long floats = (long long)a.n_envs * hist_dim(a.cfg);
  hipLaunchKernelGGL(history_kernel, dim3((unsigned)((floats + HIST_THREADS - 1) / HIST_THREADS)), dim3(HIST_THREADS), 0, s, a);
}

}  // namespace mocca_hist
