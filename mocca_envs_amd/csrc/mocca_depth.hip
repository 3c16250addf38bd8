// mocca_depth.hip -- the egocentric depth camera (include/mocca.h mocca_depth_camera): for every env, a small depth image from a pinhole
// camera that rides on one of the robot's links, cast by the ray caster's own geometry (mocca_scene.h, mocca_rays.h).  ON the training
// path: one asynchronous launch for all N envs, no host reads, no allocation, no atomics; it reads the state, task and terrain records
// and writes only the caller's rows (and, where asked, the camera records it used).
//
// One 64-lane workgroup (one wave) per env, in the shape of the height scan's kernel plus the ray caster's scene kernel.  Lane 0 walks the
// link frames into LDS -- all of them where the robot is to be seen, else only bodies 0 .. mount body (parent[b] < b: they hold the mount's
// ancestors, and a body's frame depends on its ancestors alone, so the camera record is bit for bit the same either way) -- and forms the
// camera record from the mount body's frame; lanes 32 .. 32 + n_planks stage the live planks.  After one barrier the lanes stage the
// robot's primitives from the frames (only where it is seen: a second barrier), then lane l casts pixels l, l + 64, ... and writes along
// the row: coalesced.  The primitive and plank loops have wave-uniform trip counts and every lane reads the same LDS record (a broadcast);
// the height-field march is the only divergent loop (mocca_scene.h nearest_hit: ONE routine with the ray caster).  Every trip count is an integer of the model or the grid, every index is clamped:
// a non-finite pose runs to the end and leaves finite depths in [near, far] (`far` along every ray that is not finite itself).
#include "mocca_depth.h"

#include "mocca_device.h"
#include "mocca_scene.h"

namespace mocca_depth {

using namespace mocca_rdr;

__global__ __launch_bounds__(64) void depth_kernel(DepthArgs a) {
  __shared__ float FR[MOCCA_MAX_BODIES * 15];
  __shared__ float S[MAX_PRIMS * PRIM_WORDS];
  __shared__ float PL[MOCCA_MAX_PLANKS * PLANK_WORDS];
  __shared__ float CAM[MOCCA_CAMERA_FLOATS];
  const int e = blockIdx.x, lane = threadIdx.x;
  const MoccaModel* M = a.scene.model;
  const int task = a.scene.task_id;
  const int nb = M->n_bodies > MOCCA_MAX_BODIES ? MOCCA_MAX_BODIES : M->n_bodies;
  const int body = a.body < 0 ? 0 : (a.body > nb - 1 ? nb - 1 : a.body);
  const bool see = (a.flags & MOCCA_DEPTH_SEE_ROBOT) != 0;
  int npl = task == MOCCA_TASK_WALKER3D_STEPPER ? M->n_planks : 0;
  npl = npl > MOCCA_MAX_PLANKS ? MOCCA_MAX_PLANKS : npl;
  if (lane == 0) {
    const float* st = a.scene.dyn + (size_t)e * a.scene.dyn_stride;
    walk_frames(M, st, FR, see ? nb : body + 1);
    const float* Rb = FR + 15 * body;
    float Rm[9];   // the mount frame: the body's, or R_z(yaw) of the base's heading as the height scan has it
    if (a.flags & MOCCA_DEPTH_STABILISED) {
      const float q[4] = {st[3], st[4], st[5], st[6]};
      float rp[2], cy, sy;
      mocca::quat_to_rp_heading(q, rp, &cy, &sy);
      Rm[0] = cy; Rm[1] = -sy; Rm[2] = 0.0f; Rm[3] = sy; Rm[4] = cy; Rm[5] = 0.0f; Rm[6] = 0.0f; Rm[7] = 0.0f; Rm[8] = 1.0f;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rm[k] = Rb[k];
    }
    const float fl[3] = {a.axes[0], a.axes[3], a.axes[6]}, ul[3] = {a.axes[2], a.axes[5], a.axes[8]};
    const float off[3] = {a.offset[0], a.offset[1], a.offset[2]};
    float f[3], u[3], eo[3];
    matvec3(Rm, fl, f);
    matvec3(Rm, ul, u);
    matvec3(Rb, off, eo);
#pragma unroll
    for (int k = 0; k < 3; ++k) { CAM[k] = Rb[9 + k] + eo[k]; CAM[6 + k] = u[k]; CAM[9 + k] = f[k]; }
    CAM[3] = f[1] * u[2] - f[2] * u[1]; CAM[4] = f[2] * u[0] - f[0] * u[2]; CAM[5] = f[0] * u[1] - f[1] * u[0];   // right = forward x up
    CAM[12] = a.tan_half_fov; CAM[13] = (float)a.width / (float)a.height; CAM[14] = a.near; CAM[15] = a.far;
  }
  if (lane >= 32 && lane < 32 + npl)
    stage_plank(M, a.scene.terrain + (size_t)e * a.scene.terrain_stride, lane - 32, PL + (lane - 32) * PLANK_WORDS);
  __syncthreads();
  int n_prims = 0;
  if (see) {   // wave-uniform
    n_prims = stage_robot(M, FR, lane, S, nullptr);
    n_prims = n_prims > MAX_PRIMS - 1 ? MAX_PRIMS - 1 : n_prims;
    __syncthreads();
  }

  float* row = a.out + (size_t)e * a.row_stride;
  if (a.obs) {   // the fused row: [obs | depth]
    const float* src = a.obs + (size_t)e * a.obs_dim;
    for (int k = lane; k < a.obs_dim; k += 64) row[k] = src[k];
    row += a.obs_dim;
  }
  if (a.cameras && lane < MOCCA_CAMERA_FLOATS) a.cameras[(size_t)e * MOCCA_CAMERA_FLOATS + lane] = CAM[lane];

  const bool ground = task == MOCCA_TASK_WALKER3D_CUSTOM || task == MOCCA_TASK_CASSIE;
  const bool cylinder = M->plank_shape == MOCCA_PLANK_CYLINDER;
  const float ph[3] = {M->plank_half[0], M->plank_half[1], M->plank_half[2]};
  const HeightField hf = env_heightfield(a.hf, e);
  const float tnear = CAM[14], tfar = CAM[15];
  const float o[3] = {CAM[0], CAM[1], CAM[2]};
  const int width = a.width < 1 ? 1 : a.width;
  int n_pix = width * a.height;
  n_pix = n_pix > MOCCA_DEPTH_MAX_PIXELS ? MOCCA_DEPTH_MAX_PIXELS : n_pix;
  for (int p = lane; p < n_pix; p += 64) {
    // pixel centres, as mocca_render: column px, row py (row 0 on top) looks through ((px + 1/2) / W, (py + 1/2) / H) of the image plane
    const int py = p / width, px = p - py * width;
    const float sx = (2.0f * ((float)px + 0.5f) / (float)a.width - 1.0f) * CAM[12] * CAM[13];
    const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)a.height) * CAM[12];
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = CAM[9 + k] + sx * CAM[3 + k] + sy * CAM[6 + k];
    row[p] = nearest_hit<false>(S, n_prims, PL, npl, cylinder, ph, ground, hf, o, d, tnear, tfar, nullptr);   // mocca_render's ray, depth only
  }
}

void launch_depth_camera(hipStream_t s, const DepthArgs& a, int n_envs) {
  hipLaunchKernelGGL(depth_kernel, dim3(n_envs), dim3(64), 0, s, a);
}

}  // namespace mocca_depth
