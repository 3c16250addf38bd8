// randomisation_host.cpp -- csrc/mocca_randomise.h as plain C++ on the host (tests/test_randomisation.py compiles and runs it; it is not loaded
// into Python).  It composes the header's functions exactly as the three kernels of mocca_randomise.hip do, over n_eps episodes of n_steps
// steps of n_envs envs, with ONE ring that is never cleared between episodes.
// Reads `in`:  u64 seed; i32 n_envs, n_steps, n_eps, env_offset, act_dim, dim; f32 strength_lo, strength_hi; i32 delay_min, delay_max,
//              push_interval; f32 push_max; i32 planar; f32 scale[dim]; f32 rows[n_envs][dim]; f32 actions[n_eps][n_steps][n_envs][act_dim].
// Writes `out`: per (episode, step, env) 11 + act_dim + dim 32-bit words: strength, delay (i32), phase (i32), push fires (i32), dvx, dvy,
//              record[4], 0, the effective action [act_dim], the noisy row [dim].
#include <cstdio>
#include <cstring>
#include <vector>

#include "mocca_randomise.h"

using namespace mocca_rand;

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint64_t seed;
  int32_t d[6], q[3], planar;
  float sr[2], pm;
  if (fread(&seed, 8, 1, f) != 1 || fread(d, 4, 6, f) != 6 || fread(sr, 4, 2, f) != 2 || fread(q, 4, 3, f) != 3 || fread(&pm, 4, 1, f) != 1 ||
      fread(&planar, 4, 1, f) != 1)
    return 4;
  const int n = d[0], steps = d[1], eps = d[2], off = d[3], ad = d[4], dim = d[5];
  const RandConfig c{sr[0], sr[1], q[0], q[1], q[2], pm, planar};
  std::vector<float> scale(dim), rows((size_t)n * dim), act((size_t)eps * steps * n * ad);
  if (fread(scale.data(), 4, scale.size(), f) != scale.size() || fread(rows.data(), 4, rows.size(), f) != rows.size() ||
      fread(act.data(), 4, act.size(), f) != act.size())
    return 4;
  fclose(f);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  std::vector<float> ring((size_t)n * (c.delay_max + 1) * ad, 0.0f);
  std::vector<uint32_t> out;
  for (int e = 0; e < eps; ++e)
    for (int t = 0; t < steps; ++t)
      for (int env = 0; env < n; ++env) {
        const uint32_t g = (uint32_t)(off + env);
        const EpisodeParams p = rand_episode(c, g, (uint32_t)e, k0, k1);
        const bool fires = rand_push_fires(c, (uint32_t)t, p.phase);
        float dv[2] = {0.0f, 0.0f};
        if (fires) rand_push(c, g, (uint32_t)t, (uint32_t)e, k0, k1, dv);
        out.push_back(bits(p.strength)); out.push_back((uint32_t)p.delay); out.push_back((uint32_t)p.phase); out.push_back(fires ? 1u : 0u);
        out.push_back(bits(dv[0])); out.push_back(bits(dv[1]));
        for (int w = 0; w < RAND_WORDS; ++w) out.push_back(bits(rand_record(c, p, (uint32_t)t, w)));
        out.push_back(0u);
        float* rg = ring.data() + (size_t)env * (c.delay_max + 1) * ad;
        const float* a = act.data() + (((size_t)e * steps + t) * n + env) * ad;
        const int rs = rand_read_slot(c, (uint32_t)t, p.delay);
        for (int j = 0; j < ad; ++j) {
          const float v = rand_stored(p.strength, a[j]);
          rg[rand_slot(c, (uint32_t)t) * ad + j] = v;
          out.push_back(bits(rs < 0 ? 0.0f : (p.delay == 0 ? v : rg[rs * ad + j])));
        }
        for (int k = 0; k < dim; ++k) out.push_back(bits(rand_noise(rows[(size_t)env * dim + k], scale[k], k, g, (uint32_t)t, (uint32_t)e, k0, k1)));
      }
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  if (fwrite(out.data(), 4, out.size(), f) != out.size()) return 6;
  fclose(f);
  return 0;
}
