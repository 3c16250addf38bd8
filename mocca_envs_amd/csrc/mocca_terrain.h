// mocca_terrain.h -- the random height fields of the planner envs, drawn on the device (include/mocca.h mocca_generate_heightfields):
// HeightField.get_random_height_field (bullet_objects.py:395-441, misc_utils.py:4-58) as host_logic.random_height_field restates it, in
// f32.  The arithmetic of one grid point is ONE function for the device and the host: this header compiles as plain C++ without HIP, so a
// CPU test pins it against the f64 restatement (tests/test_terrain_bank.py).  Nothing in it is contracted into fused multiply-adds: the
// host build and the kernel differ by their expf / sinf / cosf alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MOCCA_TERRAIN_HD __host__ __device__ inline
#else
#define MOCCA_TERRAIN_HD inline
#endif
#if defined(__clang__)
#define MOCCA_TERRAIN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MOCCA_TERRAIN_NO_CONTRACT
#endif

namespace mocca_terrain {

constexpr int TERRAIN_MAX_PEAKS = 256;    // = MOCCA_HF_MAX_PEAKS; also the stride of the seven parameter arrays, whatever n_peaks is
constexpr int TERRAIN_PEAK_ARRAYS = 7;    // height, centre along axis 0, centre along axis 1, spread 0, spread 1, exponent 0, exponent 1
constexpr int TERRAIN_GRAD1 = 5 * 5;      // lattice of octave 1: (4 + 1)^2 gradients, row-major
constexpr int TERRAIN_GRAD2 = 9 * 9;      // octave 2: (8 + 1)^2
constexpr int TERRAIN_GRADS = TERRAIN_GRAD1 + TERRAIN_GRAD2;   // 106
constexpr int TERRAIN_PLATFORM = 5;       // the flat corner under the robot's start: rows 0..4 x cols 0..4
// Philox domain (counter word 3) and blocks (counter word 1) of the generator's draws
constexpr uint32_t TERRAIN_DOMAIN = 3u;
enum : uint32_t { TERRAIN_BLOCK_PEAKS = 0u, TERRAIN_BLOCK_GRAD1 = 1u, TERRAIN_BLOCK_GRAD2 = 2u };

// the uniform of a Philox word, as every draw of the device code: 24 bits
MOCCA_TERRAIN_HD float terrain_uniform(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }

// Parameter k of array a from its uniform (rng.uniform(0.1, 3), (-half, half) twice, (1, 16) twice, rng.randint(1, 6) * 2 twice): the affine
// maps in f32.  The exponents are kept as their HALVES 1 .. 5 (the even power is taken of the square).  half0 / half1: size / scale / 2.
MOCCA_TERRAIN_HD float terrain_peak_param(int a, float u, float half0, float half1) {
  MOCCA_TERRAIN_NO_CONTRACT
  switch (a) {
    case 0: return 0.1f + 2.9f * u;
    case 1: return -half0 + (2.0f * half0) * u;
    case 2: return -half1 + (2.0f * half1) * u;
    case 3: case 4: return 1.0f + 15.0f * u;
    default: { const int e = 1 + (int)(5.0f * u); return (float)(e > 5 ? 5 : e); }
  }
}
// a lattice gradient from its uniform: (cos, sin) of 2 pi u
MOCCA_TERRAIN_HD void terrain_gradient(float u, float* g) {
  MOCCA_TERRAIN_NO_CONTRACT
  const float th = 6.283185307179586f * u;
  g[0] = cosf(th); g[1] = sinf(th);
}

MOCCA_TERRAIN_HD float terrain_fade(float t) {
  MOCCA_TERRAIN_NO_CONTRACT
  return t * t * t * (t * (6.0f * t - 15.0f) + 10.0f);
}
// one Perlin layer at grid point (i, j): `res` x `res` lattice cells over rows x cols points, gradients g[(res + 1)^2][2] (misc_utils.py:4-33)
MOCCA_TERRAIN_HD float terrain_perlin(const float* g, int res, int rows, int cols, int i, int j) {
  MOCCA_TERRAIN_NO_CONTRACT
  const int per0 = rows / res, per1 = cols / res;     // grid points per lattice cell (rows and cols are multiples of 8)
  const int ci = i / per0, cj = j / per1;
  const float u = (float)(i - ci * per0) / (float)per0, v = (float)(j - cj * per1) / (float)per1;
  const float* g00 = g + 2 * (ci * (res + 1) + cj);
  const float* g10 = g00 + 2 * (res + 1);
  const float r00 = u * g00[0] + v * g00[1], r10 = (u - 1.0f) * g10[0] + v * g10[1];
  const float r01 = u * g00[2] + (v - 1.0f) * g00[3], r11 = (u - 1.0f) * g10[2] + (v - 1.0f) * g10[3];
  const float fu = terrain_fade(u), fv = terrain_fade(v);
  const float low = r00 * (1.0f - fu) + fu * r10, high = r01 * (1.0f - fu) + fu * r11;
  return 1.4142135623730951f * ((1.0f - fv) * low + fv * high);
}

// The raw height of grid point (i, j) -- row i, column j --: the peaks summed for k ascending, divided by the scale, plus the two noise
// octaves (persistence 1).  The generator's first axis is the ROW index (the reference builds its meshgrid so; its x is Bullet's y).
// peaks: [TERRAIN_PEAK_ARRAYS][TERRAIN_MAX_PEAKS]; grads: [TERRAIN_GRADS][2], octave 1 first.  What is left is the caller's: minus the level
// of the platform, times the gain.
MOCCA_TERRAIN_HD float terrain_point(const float* peaks, int n_peaks, const float* grads, int rows, int cols, float scale, int i, int j) {
  MOCCA_TERRAIN_NO_CONTRACT
  const float half0 = (float)rows / scale * 0.5f, half1 = (float)cols / scale * 0.5f;
  const float g0 = (float)i * ((2.0f * half0) / (float)(rows - 1)) + -half0;   // np.linspace: arange * step + start
  const float g1 = (float)j * ((2.0f * half1) / (float)(cols - 1)) + -half1;
  const float* P = peaks;
  constexpr int S = TERRAIN_MAX_PEAKS;
  float sum = 0.0f;
  for (int k = 0; k < n_peaks; ++k) {
    const float d0 = g0 - P[S + k], d1 = g1 - P[2 * S + k];
    const float q0 = d0 * d0, q1 = d1 * d1;
    float p0 = q0, p1 = q1;
    for (int e = (int)P[5 * S + k]; e > 1; --e) p0 = p0 * q0;
    for (int e = (int)P[6 * S + k]; e > 1; --e) p1 = p1 * q1;
    sum = sum + P[k] * expf(-(p0 / P[3 * S + k]) - p1 / P[4 * S + k]);
  }
  return sum / scale + (terrain_perlin(grads, 4, rows, cols, i, j) + terrain_perlin(grads + 2 * TERRAIN_GRAD1, 8, rows, cols, i, j));
}

// the level of the platform: the f32 sum of its 25 raw heights in index order (row-major), divided by 25
MOCCA_TERRAIN_HD float terrain_level(const float* corner) {
  MOCCA_TERRAIN_NO_CONTRACT
  float s = 0.0f;
  for (int c = 0; c < TERRAIN_PLATFORM * TERRAIN_PLATFORM; ++c) s = s + corner[c];
  return s / (float)(TERRAIN_PLATFORM * TERRAIN_PLATFORM);
}
// the finished height of point (i, j) from its raw one: the platform is flattened to the level, everything is lowered by it (the platform
// ends at exactly 0.0) and multiplied by the gain
MOCCA_TERRAIN_HD float terrain_finish(float raw, float level, int i, int j, float gain) {
  MOCCA_TERRAIN_NO_CONTRACT
  const float v = i < TERRAIN_PLATFORM && j < TERRAIN_PLATFORM ? level : raw;
  return (v - level) * gain;
}

#if defined(__HIPCC__)
// One generate call (mocca_generate_heightfields): fields first .. first + count - 1 of a bank whose field f starts at bank + f * stride --
// the heights [rows][cols], then one max-pooled copy per search window 2 .. planes (mocca_device.h sphere_heightfield) -- and whose range
// [zmin, zmax] is range[2 f], range[2 f + 1].  part: [n_fields][blocks per field][2], scratch of the range reduction, owned by the handle.
struct TerrainArgs {
  float* bank;
  float* range;
  float* part;
  size_t stride;
  int rows, cols, planes;
  float scale, gain;
  int first, count, n_peaks;
  uint32_t seed_lo, seed_hi;
};
constexpr int TERRAIN_BLOCK = 256;
inline int terrain_blocks(int rows, int cols) { return (rows * cols + TERRAIN_BLOCK - 1) / TERRAIN_BLOCK; }
void launch_generate(hipStream_t s, const TerrainArgs& a);
#endif

}  // namespace mocca_terrain
