// history_host.cpp -- csrc/mocca_history.h as plain C++ on the host (tests/test_history.py compiles and runs it; it is not loaded into Python).
// It runs hist_thread, the work of one GPU thread, for every (env, word) of every call, as the kernel of mocca_history.hip does -- TWICE, on
// two rings: once with the threads in ascending and once in descending order.  The header argues that no thread reads a ring word another
// thread of the same launch writes; then the order cannot matter, and the program fails (exit 7) if the two runs ever differ.
// Reads `in`:  i32 n_envs, n_calls, obs_dim, act_stride, steps, stride, n_cols, act_dim; i32 cols[n_cols]; per call: i32 have_act,
//              u32 T[n_envs], u32 E[n_envs], f32 rows[n_envs][obs_dim], f32 act[n_envs][act_stride].
// Writes `out`: per call the block, u32 [n_envs][steps * (n_cols + act_dim)].
#include <cstdio>
#include <cstring>
#include <vector>

#include "mocca_history.h"

using namespace mocca_hist;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t d[8];
  if (fread(d, 4, 8, f) != 8) return 4;
  const int n = d[0], calls = d[1], obs_dim = d[2], act_stride = d[3];
  const HistConfig c{d[4], d[5], d[6], d[7]};
  std::vector<int32_t> cols((size_t)c.n_cols + 1);
  if (fread(cols.data(), 4, (size_t)c.n_cols, f) != (size_t)c.n_cols) return 4;
  const int dim = hist_dim(c), width = hist_width(c), slots = hist_slots(c);
  std::vector<float> ring[2];
  std::vector<uint32_t> tags[2];
  for (int r = 0; r < 2; ++r) {   // as mocca_set_history leaves them
    ring[r].assign((size_t)n * slots * width, 0.0f);
    tags[r].assign((size_t)n * slots * 2, HIST_NO_T);
  }
  std::vector<uint32_t> T(n), E(n);
  std::vector<float> rows((size_t)n * obs_dim), act((size_t)n * act_stride), out[2];
  out[0].resize((size_t)n * dim); out[1].resize((size_t)n * dim);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 5;
  for (int k = 0; k < calls; ++k) {
    int32_t have_act;
    if (fread(&have_act, 4, 1, f) != 1 || fread(T.data(), 4, n, f) != (size_t)n || fread(E.data(), 4, n, f) != (size_t)n ||
        fread(rows.data(), 4, rows.size(), f) != rows.size() || fread(act.data(), 4, act.size(), f) != act.size())
      return 4;
    for (int r = 0; r < 2; ++r)
      for (int q = 0; q < n * dim; ++q) {
        const int i = r ? n * dim - 1 - q : q, env = i / dim, w = i - env * dim;
        hist_thread(c, T[env], E[env], rows.data() + (size_t)env * obs_dim, have_act ? act.data() + (size_t)env * act_stride : nullptr, cols.data(),
                    ring[r].data() + (size_t)env * slots * width, tags[r].data() + (size_t)env * slots * 2, out[r].data() + (size_t)env * dim, w);
      }
    if (std::memcmp(out[0].data(), out[1].data(), out[0].size() * 4) || std::memcmp(ring[0].data(), ring[1].data(), ring[0].size() * 4) ||
        std::memcmp(tags[0].data(), tags[1].data(), tags[0].size() * 4))
      return 7;
    if (fwrite(out[0].data(), 4, out[0].size(), g) != out[0].size()) return 6;
  }
  fclose(f);
  fclose(g);
  return 0;
}
