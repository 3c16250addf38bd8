// mocca_terrain.hip -- random height fields for the planner envs' terrain bank, generated in place on the device (include/mocca.h
// mocca_generate_heightfields; the arithmetic is mocca_terrain.h).  NOT a hot path: a trainer refreshes its terrain between rollouts.
//
// Two launches on the caller's stream, no allocation, no host read, no atomics:
//   heights: grid (blocks per field, fields), 256 threads, one thread per grid point.  Every block stages the field's 7 x 256 peak
//            parameters and 106 lattice gradients in LDS from Philox (a block's share of a field is 256 points x 256 peaks = 65 k expf; the
//            staging is 475 Philox blocks), recomputes the 25 raw heights of the corner platform (one thread each) and sums them in index
//            order on one thread -- every block of a field gets the same level bits without a grid-wide exchange --, writes its heights and
//            reduces their min / max over a fixed tree into the handle's scratch.
//   finish:  the same grid; block 0 of a field reduces the scratch to the field's [zmin, zmax], and every thread fills its point of the
//            max-pooled copies the step kernel prunes a wide sphere's search by (windows 2 .. planes; none for most robots and grids).
#include "mocca_terrain.h"

#include "mocca_philox.h"

namespace mocca_terrain {

__global__ __launch_bounds__(TERRAIN_BLOCK) void terrain_heights_kernel(TerrainArgs a) {
  __shared__ float P[TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS];
  __shared__ float G[TERRAIN_GRADS * 2];
  __shared__ float CORNER[TERRAIN_PLATFORM * TERRAIN_PLATFORM];
  __shared__ float LEVEL;
  __shared__ float LO[TERRAIN_BLOCK], HI[TERRAIN_BLOCK];
  const int t = threadIdx.x, field = a.first + (int)blockIdx.y;
  const float half0 = (float)a.rows / a.scale * 0.5f, half1 = (float)a.cols / a.scale * 0.5f;
  uint32_t w[4];
  for (int q = t; q < TERRAIN_PEAK_ARRAYS * TERRAIN_MAX_PEAKS / 4; q += TERRAIN_BLOCK) {   // draws d = 256 a + k, four to a Philox block
    philox4x32((uint32_t)q, TERRAIN_BLOCK_PEAKS, (uint32_t)field, TERRAIN_DOMAIN, a.seed_lo, a.seed_hi, w);
#pragma unroll
    for (int c = 0; c < 4; ++c) P[4 * q + c] = terrain_peak_param((4 * q + c) / TERRAIN_MAX_PEAKS, terrain_uniform(w[c]), half0, half1);
  }
  if (t < (TERRAIN_GRAD1 + 3) / 4 + (TERRAIN_GRAD2 + 3) / 4) {
    const bool second = t >= (TERRAIN_GRAD1 + 3) / 4;
    const int q = second ? t - (TERRAIN_GRAD1 + 3) / 4 : t, n = second ? TERRAIN_GRAD2 : TERRAIN_GRAD1;
    philox4x32((uint32_t)q, second ? TERRAIN_BLOCK_GRAD2 : TERRAIN_BLOCK_GRAD1, (uint32_t)field, TERRAIN_DOMAIN, a.seed_lo, a.seed_hi, w);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (4 * q + c < n) terrain_gradient(terrain_uniform(w[c]), G + 2 * ((second ? TERRAIN_GRAD1 : 0) + 4 * q + c));
  }
  __syncthreads();
  if (t < TERRAIN_PLATFORM * TERRAIN_PLATFORM)
    CORNER[t] = terrain_point(P, a.n_peaks, G, a.rows, a.cols, a.scale, t / TERRAIN_PLATFORM, t % TERRAIN_PLATFORM);
  __syncthreads();
  if (t == 0) LEVEL = terrain_level(CORNER);
  __syncthreads();
  const float level = LEVEL;
  const int cells = a.rows * a.cols, p = (int)blockIdx.x * TERRAIN_BLOCK + t;
  float lo = 3.0e38f, hi = -3.0e38f;
  if (p < cells) {
    const int i = p / a.cols, j = p % a.cols;
    const float v = terrain_finish(terrain_point(P, a.n_peaks, G, a.rows, a.cols, a.scale, i, j), level, i, j, a.gain);
    a.bank[(size_t)field * a.stride + p] = v;
    lo = hi = v;
  }
  LO[t] = lo; HI[t] = hi;
  __syncthreads();
  for (int h = TERRAIN_BLOCK / 2; h > 0; h >>= 1) {
    if (t < h) { LO[t] = fminf(LO[t], LO[t + h]); HI[t] = fmaxf(HI[t], HI[t + h]); }
    __syncthreads();
  }
  if (t == 0) {
    float* part = a.part + ((size_t)field * gridDim.x + blockIdx.x) * 2;
    part[0] = LO[0]; part[1] = HI[0];
  }
}

__global__ __launch_bounds__(TERRAIN_BLOCK) void terrain_finish_kernel(TerrainArgs a) {
  __shared__ float LO[TERRAIN_BLOCK], HI[TERRAIN_BLOCK];
  const int t = threadIdx.x, field = a.first + (int)blockIdx.y;
  if (blockIdx.x == 0) {
    const float* part = a.part + (size_t)field * gridDim.x * 2;
    float lo = 3.0e38f, hi = -3.0e38f;
    for (int b = t; b < (int)gridDim.x; b += TERRAIN_BLOCK) { lo = fminf(lo, part[2 * b]); hi = fmaxf(hi, part[2 * b + 1]); }
    LO[t] = lo; HI[t] = hi;
    __syncthreads();
    for (int h = TERRAIN_BLOCK / 2; h > 0; h >>= 1) {
      if (t < h) { LO[t] = fminf(LO[t], LO[t + h]); HI[t] = fmaxf(HI[t], HI[t + h]); }
      __syncthreads();
    }
    if (t == 0) { a.range[2 * field] = LO[0]; a.range[2 * field + 1] = HI[0]; }
  }
  const int cells = a.rows * a.cols, p = (int)blockIdx.x * TERRAIN_BLOCK + t;
  if (p >= cells) return;
  const int i = p / a.cols, j = p % a.cols;
  float* f = a.bank + (size_t)field * a.stride;
  for (int w = 2; w <= a.planes; ++w) {   // the highest point within w cells each way
    const int j0 = j - w < 0 ? 0 : j - w, j1 = j + w > a.cols - 1 ? a.cols - 1 : j + w;
    const int i0 = i - w < 0 ? 0 : i - w, i1 = i + w > a.rows - 1 ? a.rows - 1 : i + w;
    float m = -1e30f;
    for (int ii = i0; ii <= i1; ++ii)
      for (int jj = j0; jj <= j1; ++jj) m = fmaxf(m, f[(size_t)ii * a.cols + jj]);
    f[(size_t)(w - 1) * cells + p] = m;
  }
}

void launch_generate(hipStream_t s, const TerrainArgs& a) {
  const dim3 grid(terrain_blocks(a.rows, a.cols), a.count);
  hipLaunchKernelGGL(terrain_heights_kernel, grid, dim3(TERRAIN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(terrain_finish_kernel, grid, dim3(TERRAIN_BLOCK), 0, s, a);
}

}  // namespace mocca_terrain
