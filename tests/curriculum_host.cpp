// curriculum_host.cpp -- csrc/mocca_curriculum.h as plain C++ on the host (tests/test_curriculum.py compiles and runs it; it is not loaded into
// Python).  It runs cur_thread, the work of one GPU thread, for every env of every launch whose done byte is non-zero, as the kernel of
// mocca_curriculum.hip does -- TWICE, on two copies of the state: once with the threads in ascending and once in descending order.  Each
// thread owns its env and the totals are sums of whole numbers; then the order cannot matter, and the program fails (exit 7) if the two
// runs ever differ.
// Reads `in`:  i32 n_envs, n_launches, promote_at, demote_at, patience, min_level, max_level, recycle, env_offset; u32 seed_lo, seed_hi;
//              f32 level[n_envs]; per launch: u8 done[n_envs], i32 info[n_envs], u32 E[n_envs].
// Writes `out`: per launch u32 level bits[n_envs], i32 streak[n_envs], i32 hold[n_envs], f32 totals[10][4], u32 the draw word of (g, E)[n_envs].
#include <cstdio>
#include <cstring>
#include <vector>

#include "mocca_curriculum.h"

using namespace mocca_cur;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t d[9];
  uint32_t key[2];
  if (fread(d, 4, 9, f) != 9 || fread(key, 4, 2, f) != 2) return 4;
  const int n = d[0], launches = d[1], env_offset = d[8];
  const CurConfig c{d[2], d[3], d[4], d[5], d[6], d[7]};
  std::vector<float> level[2], totals[2];
  std::vector<int32_t> streak[2], hold[2];
  level[0].resize(n);
  if (fread(level[0].data(), 4, n, f) != (size_t)n) return 4;
  level[1] = level[0];
  for (int r = 0; r < 2; ++r) {   // as mocca_set_curriculum leaves them
    streak[r].assign(n, 0); hold[r].assign(n, 0); totals[r].assign(CUR_LEVELS * CUR_TOTALS, 0.0f);
  }
  std::vector<uint8_t> done(n);
  std::vector<int32_t> info(n);
  std::vector<uint32_t> E(n), draws(n);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 5;
  for (int k = 0; k < launches; ++k) {
    if (fread(done.data(), 1, n, f) != (size_t)n || fread(info.data(), 4, n, f) != (size_t)n || fread(E.data(), 4, n, f) != (size_t)n) return 4;
    for (int r = 0; r < 2; ++r)
      for (int q = 0; q < n; ++q) {
        const int env = r ? n - 1 - q : q;
        if (!done[env]) continue;
        cur_thread(c, info[env], (uint32_t)env_offset + (uint32_t)env, &E[env], key[0], key[1], &level[r][env], &streak[r][env], &hold[r][env],
                   totals[r].data());
      }
    if (std::memcmp(level[0].data(), level[1].data(), (size_t)n * 4) || std::memcmp(streak[0].data(), streak[1].data(), (size_t)n * 4) ||
        std::memcmp(hold[0].data(), hold[1].data(), (size_t)n * 4) || std::memcmp(totals[0].data(), totals[1].data(), totals[0].size() * 4))
      return 7;
    for (int env = 0; env < n; ++env) draws[env] = cur_draw((uint32_t)env_offset + (uint32_t)env, E[env], key[0], key[1]);
    if (fwrite(level[0].data(), 4, n, g) != (size_t)n || fwrite(streak[0].data(), 4, n, g) != (size_t)n || fwrite(hold[0].data(), 4, n, g) != (size_t)n ||
        fwrite(totals[0].data(), 4, totals[0].size(), g) != totals[0].size() || fwrite(draws.data(), 4, n, g) != (size_t)n)
      return 6;
  }
  fclose(f);
  fclose(g);
  return 0;
}
