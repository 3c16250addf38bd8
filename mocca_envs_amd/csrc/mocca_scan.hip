// mocca_scan.hip -- the terrain height scan (include/mocca.h mocca_height_scan): for every env, the terrain height under a fixed pattern of
// points around the robot, in its heading frame, relative to the base.  ON the training path: one asynchronous launch for all N envs, no
// host reads, no allocation, no atomics; it reads the state, task and terrain records and writes only the caller's rows.
//
// One 64-lane workgroup (one wave) per env, lanes over the points.  Lane 0 puts the base position and the heading (cos yaw, sin yaw -- from
// the quaternion as the step kernel's observation derives them, mocca_device.h quat_to_rp_heading) into LDS, lanes 32 .. 32 + n_planks the
// frames of the live planks (mocca_rays.h stage_plank, as the ray caster's scene kernel); after one barrier every lane handles points lane,
// lane + 64, ...: the rotation into the world, then a vertical ray.  The plank loop has a wave-uniform trip count and every lane reads the
// same LDS record (a broadcast); the height field needs no march under a vertical ray: the cell under the point, four loads from a table
// (64 KB for the planner envs' 128 x 128 grid) that stays in L2.  The optional observation copy and the stores run along the row: coalesced.
#include "mocca_scan.h"

#include "mocca_device.h"

namespace mocca_scan {

using namespace mocca_rdr;

__global__ __launch_bounds__(64) void scan_kernel(ScanArgs a) {
  __shared__ float POSE[8];                                  // base x, y, z, cos yaw, sin yaw
  __shared__ float PL[MOCCA_MAX_PLANKS * PLANK_WORDS];
  const int e = blockIdx.x, lane = threadIdx.x;
  const MoccaModel* M = a.scene.model;
  const int task = a.scene.task_id;
  int npl = task == MOCCA_TASK_WALKER3D_STEPPER ? M->n_planks : 0;
  npl = npl > MOCCA_MAX_PLANKS ? MOCCA_MAX_PLANKS : npl;
  if (lane == 0) {
    const float* st = a.scene.dyn + (size_t)e * a.scene.dyn_stride;
    const float q[4] = {st[3], st[4], st[5], st[6]};
    float rp[2], cy, sy;
    mocca::quat_to_rp_heading(q, rp, &cy, &sy);
    POSE[0] = st[0]; POSE[1] = st[1]; POSE[2] = st[2]; POSE[3] = cy; POSE[4] = sy;
  }
  if (lane >= 32 && lane < 32 + npl)
    stage_plank(M, a.scene.terrain + (size_t)e * a.scene.terrain_stride, lane - 32, PL + (lane - 32) * PLANK_WORDS);
  __syncthreads();

  float* row = a.out + (size_t)e * a.row_stride;
  if (a.obs) {   // the fused row: [obs | scan]
    const float* src = a.obs + (size_t)e * a.obs_dim;
    for (int k = lane; k < a.obs_dim; k += 64) row[k] = src[k];
    row += a.obs_dim;
  }

  const float bx = POSE[0], by = POSE[1], bz = POSE[2], cy = POSE[3], sy = POSE[4];
  const float zs = bz + a.z_above, tfar = a.z_above + a.max_drop;
  const bool ground = task == MOCCA_TASK_WALKER3D_CUSTOM || task == MOCCA_TASK_CASSIE;
  const bool cylinder = M->plank_shape == MOCCA_PLANK_CYLINDER;
  const float ph[3] = {M->plank_half[0], M->plank_half[1], M->plank_half[2]};
  const HeightField hf = env_heightfield(a.hf, e);
  for (int p = lane; p < a.n_points; p += 64) {
    const float px = a.points[2 * p], py = a.points[2 * p + 1];
    const float x = bx + (cy * px - sy * py), y = by + (sy * px + cy * py);
    float v = -a.max_drop;                                   // nothing below the point
    if (ground) v = 0.0f - bz;
    float best = tfar;                                       // the ray o + t (0, 0, -1), o = (x, y, zs)
#pragma unroll 1
    for (int k = 0; k < npl; ++k) {
      const float* B = PL + k * PLANK_WORDS;
      const float rel[3] = {x - B[9], y - B[10], zs - B[11]};
      float lo[3], ld[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {   // into the plank frame: R^T
        lo[c] = B[c] * rel[0] + B[3 + c] * rel[1] + B[6 + c] * rel[2];
        ld[c] = -B[6 + c];
      }
      // a start point inside the solid: the surface is at (or above) the start
      const bool inside = cylinder ? (lo[0] * lo[0] + lo[1] * lo[1] <= ph[0] * ph[0] && fabsf(lo[2]) <= ph[2])
                                   : (fabsf(lo[0]) <= ph[0] && fabsf(lo[1]) <= ph[1] && fabsf(lo[2]) <= ph[2]);
      int part = 0;
      const float t = inside ? 0.0f : (cylinder ? hit_cylinder(lo, ld, ph, &part) : hit_box(lo, ld, ph, &part));
      if (t >= 0.0f && t < best) best = t;
    }
    if (best < tfar) v = (zs - best) - bz;
    if (hf.data) {   // the cell under the point; outside the grid there is no ground
      const float gx = x * hf.scale + 0.5f * (float)(hf.cols - 1), gy = y * hf.scale + 0.5f * (float)(hf.rows - 1);
      if (gx >= 0.0f && gx <= (float)(hf.cols - 1) && gy >= 0.0f && gy <= (float)(hf.rows - 1)) {   // (false for a non-finite point)
        int i = (int)floorf(gx), j = (int)floorf(gy);
        i = i < 0 ? 0 : (i > hf.cols - 2 ? hf.cols - 2 : i);
        j = j < 0 ? 0 : (j > hf.rows - 2 ? hf.rows - 2 : j);
        const float* c = hf.data + (size_t)j * hf.cols + i;
        v = cell_height(c[0], c[1], c[hf.cols], c[hf.cols + 1], gx - (float)i, gy - (float)j) - bz;
      }
    }
    row[p] = fminf(fmaxf(v, -a.max_drop), a.z_above);
  }
}

void launch_height_scan(hipStream_t s, const ScanArgs& a, int n_envs) {
  hipLaunchKernelGGL(scan_kernel, dim3(n_envs), dim3(64), 0, s, a);
}

}  // namespace mocca_scan
