// terrain_host.cpp -- csrc/mocca_terrain.h as plain C++ on the host (tests/test_terrain_bank.py compiles and runs it; it is not loaded into
// Python).  Reads `in`: int32 rows, cols, n_peaks; f32 scale, gain; then the float32 uniforms of one field, 7 x 256 peak draws, 25 + 81
// lattice draws.  Writes `out`: the finished field, f32 [rows][cols], exactly as the kernel composes it from the header's functions.
#include <cstdio>
#include <vector>

#include "mocca_terrain.h"

using namespace mocca_terrain;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t dims[3];
  float sg[2];
  std::vector<float> u(TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS + TERRAIN_GRADS);
  if (fread(dims, 4, 3, f) != 3 || fread(sg, 4, 2, f) != 2 || fread(u.data(), 4, u.size(), f) != u.size()) return 4;
  fclose(f);
  const int rows = dims[0], cols = dims[1], n_peaks = dims[2];
  const float scale = sg[0], gain = sg[1];
  const float half0 = (float)rows / scale * 0.5f, half1 = (float)cols / scale * 0.5f;
  std::vector<float> P(TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS), G(TERRAIN_GRADS * 2);
  for (int d = 0; d < TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS; ++d) P[d] = terrain_peak_param(d / TERRAIN_MAX_PEAKS, u[d], half0, half1);
  for (int g = 0; g < TERRAIN_GRADS; ++g) terrain_gradient(u[TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS + g], &G[2 * g]);
  float corner[TERRAIN_PLATFORM * TERRAIN_PLATFORM];
  for (int c = 0; c < TERRAIN_PLATFORM * TERRAIN_PLATFORM; ++c)
    corner[c] = terrain_point(P.data(), n_peaks, G.data(), rows, cols, scale, c / TERRAIN_PLATFORM, c % TERRAIN_PLATFORM);
  const float level = terrain_level(corner);
  std::vector<float> out((size_t)rows * cols);
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j)
      out[(size_t)i * cols + j] = terrain_finish(terrain_point(P.data(), n_peaks, G.data(), rows, cols, scale, i, j), level, i, j, gain);
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  if (fwrite(out.data(), 4, out.size(), f) != out.size()) return 6;
  fclose(f);
  return 0;
}
