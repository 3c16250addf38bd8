// mocca_rays.h -- the terrain geometry that the ray caster (mocca_render.hip) and the height scan (mocca_scan.hip) share: how a live plank
// of the Stepper's terrain record becomes a world-space frame, the ray / oriented-box and ray / upright-cylinder intersections, and the
// height of a height-field cell.  Device code only; one definition, two users.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mocca.h"

#ifndef DI
#define DI __device__ __forceinline__
#endif

namespace mocca_rdr {

constexpr int PLANK_WORDS = 12;                        // rotation (9, world <- plank), box centre (3)

struct SceneArgs {
  const MoccaModel* model;
  const float* dyn;        // [N][dyn_stride]
  const uint32_t* task;    // [N][MOCCA_TASK_WORDS]
  const float* terrain;    // [N][terrain_stride]
  int dyn_stride, terrain_stride, task_id;
};
struct HeightField { const float* data; int rows, cols; float scale, zmin, zmax; };   // data == nullptr: none
// The planner handle's terrain bank (mocca_set_heightfield_bank): field f at data + f * stride, its range at range[2 f], range[2 f + 1] (device
// memory: mocca_generate_heightfields writes it without telling the host); env e stands on field[e], or on field 0 where field == nullptr.
struct HeightFieldBank { const float* data; int rows, cols; float scale; const float* range; const int32_t* field; size_t stride; };
DI HeightField env_heightfield(const HeightFieldBank& b, int env) {
  if (!b.data) return HeightField{nullptr, 0, 0, 0.0f, 0.0f, 0.0f};
  const int f = b.field ? b.field[env] : 0;
  return HeightField{b.data + (size_t)f * b.stride, b.rows, b.cols, b.scale, b.range[2 * f], b.range[2 * f + 1]};
}

__host__ DI void euler_to_mat(float roll, float pitch, float yaw, float* R) {   // (on the host too: mocca_set_depth_camera's mount)
  const float cr = cosf(roll), sr = sinf(roll), cp = cosf(pitch), sp = sinf(pitch), cy = cosf(yaw), sy = sinf(yaw);
  R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
  R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
  R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

// live plank k of one env's terrain record `ter`, as the step kernel stages it (mocca_device.h stage_planks): o[0 .. 9) the rotation
// world <- plank, o[9 .. 12) the centre of the box / cylinder
DI void stage_plank(const MoccaModel* M, const float* ter, int k, float* o) {
  int row = (int)ter[6 * MOCCA_MAX_TERRAIN_STEPS + k];
  row = row < 0 ? 0 : (row > MOCCA_MAX_TERRAIN_STEPS - 1 ? MOCCA_MAX_TERRAIN_STEPS - 1 : row);
  const float* ti = ter + 6 * row;
  float Rb[9];
  euler_to_mat(ti[4], ti[5], ti[3], Rb);
  const float cz = M->plank_com_z, dz = -M->plank_half[2] - cz;
#pragma unroll
  for (int i = 0; i < 9; ++i) o[i] = Rb[i];
  o[9] = ti[0] + Rb[2] * dz; o[10] = ti[1] + Rb[5] * dz; o[11] = ti[2] + Rb[8] * dz + cz;
}

// ---- ray / primitive intersections in the plank frame.  Each returns the entry parameter (the ray starts outside), or a negative number
// for a miss. ----
DI float hit_box(const float* lo, const float* ld, const float* h, int* axis) {   // ray in the box frame
  float t0 = -1e30f, t1 = 1e30f;
  int ax = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (fabsf(ld[k]) < 1e-20f) {
      if (fabsf(lo[k]) > h[k]) return -1.0f;
    } else {
      const float inv = 1.0f / ld[k];
      float ta = (-h[k] - lo[k]) * inv, tb = (h[k] - lo[k]) * inv;
      if (ta > tb) { const float s = ta; ta = tb; tb = s; }
      if (ta > t0) { t0 = ta; ax = k; }
      t1 = fminf(t1, tb);
    }
  }
  *axis = ax;
  return t0 <= t1 ? t0 : -1.0f;
}
// upright cylinder in the plank frame: radius h[0], half height h[2]; part: 0 side, 1 cap
DI float hit_cylinder(const float* lo, const float* ld, const float* h, int* part) {
  float best = -1.0f;
  *part = 0;
  const float A = ld[0] * ld[0] + ld[1] * ld[1], B = lo[0] * ld[0] + lo[1] * ld[1], C = lo[0] * lo[0] + lo[1] * lo[1] - h[0] * h[0];
  if (A > 1e-20f) {
    const float disc = B * B - A * C;
    if (disc >= 0.0f) {
      const float t = (-B - sqrtf(disc)) / A;
      if (fabsf(lo[2] + t * ld[2]) <= h[2]) best = t;
    }
  }
  if (fabsf(ld[2]) > 1e-20f) {
    const float t = ((ld[2] < 0.0f ? h[2] : -h[2]) - lo[2]) / ld[2];   // the cap that faces the ray
    const float px = lo[0] + t * ld[0], py = lo[1] + t * ld[1];
    if (px * px + py * py <= h[0] * h[0] && (best < 0.0f || t < best)) { best = t; *part = 1; }
  }
  return best;
}

// height of cell (i, j)'s surface at cell coordinates (u, v): two triangles split from (i + 1, j) to (i, j + 1) (mocca_set_heightfield)
DI float cell_height(float h00, float h10, float h01, float h11, float u, float v) {
  return u + v <= 1.0f ? h00 + u * (h10 - h00) + v * (h01 - h00) : h11 + (1.0f - u) * (h01 - h11) + (1.0f - v) * (h10 - h11);
}

}  // namespace mocca_rdr
