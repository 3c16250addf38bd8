// mocca_render.hip -- where the robot's links are, and a ray caster over one env's scene (include/mocca.h mocca_get_link_frames, mocca_render).
//
// Three kernels, none of them on the training path (the walk, the robot's primitives and the ray / primitive intersections live in
// mocca_scene.h and mocca_rays.h, shared with the depth camera and the height scan, which are):
//   link_frames_kernel   one thread per env walks the tree root to leaves (parent[b] < b) in the oracle's order of operations
//                        and writes R, origin, COM per body.
//   scene_kernel         one wave per view: the same walk into LDS, then lane g turns geom g into a world-space record; (a model whose geoms are all
//                        points: its skeleton); the live planks and the walk target follow.  The walk is a serial chain of up to 22 joints: it runs once per view here, not once per tile.
//   raycast_kernel       one thread per pixel, a 16 x 16 tile per workgroup.  The workgroup copies the view's scene (< 2 KB) into LDS; every
//                        lane then loops over the primitives with a wave-uniform trip count, all lanes reading the same LDS address
//                        (a broadcast, no bank conflict).  The height-field march is the only divergent loop.
#include "mocca_render.h"

namespace mocca_rdr {

#define DI __device__ __forceinline__

// ---- colours (cosmetic; stated once in include/mocca.h) ----
__constant__ float PALETTE[8][3] = {{0.85f, 0.55f, 0.20f}, {0.25f, 0.55f, 0.85f}, {0.35f, 0.75f, 0.40f}, {0.80f, 0.35f, 0.35f},
                                    {0.65f, 0.45f, 0.80f}, {0.90f, 0.80f, 0.30f}, {0.30f, 0.75f, 0.75f}, {0.70f, 0.70f, 0.70f}};
__constant__ float BG[3] = {0.53f, 0.71f, 0.90f};
__constant__ float GROUND_A[3] = {0.80f, 0.80f, 0.78f}, GROUND_B[3] = {0.55f, 0.58f, 0.60f};
__constant__ float PLANK_RGB[3] = {0.72f, 0.53f, 0.33f}, TARGET_RGB[3] = {0.90f, 0.15f, 0.15f};
__constant__ float HF_LOW[3] = {0.30f, 0.50f, 0.25f}, HF_HIGH[3] = {0.85f, 0.80f, 0.65f};
__constant__ float LIGHT[3] = {0.36f, -0.48f, 0.80f};   // unit vector towards the light
constexpr float AMBIENT = 0.35f;

__global__ __launch_bounds__(64) void link_frames_kernel(SceneArgs a, int n, float* frames) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  const MoccaModel* M = a.model;
  walk_frames(M, a.dyn + (size_t)e * a.dyn_stride, frames + (size_t)e * M->n_bodies * 15, M->n_bodies);
}

// one wave per view
__global__ __launch_bounds__(64) void scene_kernel(SceneArgs a, const int32_t* env_ids, int n_envs, float* scenes) {
  __shared__ float fr[MOCCA_MAX_BODIES * 15];
  const int view = blockIdx.x, lane = threadIdx.x;
  int e = env_ids[view];
  e = e < 0 ? 0 : (e > n_envs - 1 ? n_envs - 1 : e);   // (mocca_render has refused ids out of range; the clamp keeps the loads in bounds regardless)
  const MoccaModel* M = a.model;
  float* out = scenes + (size_t)view * SCENE_WORDS;
  if (lane == 0) walk_frames(M, a.dyn + (size_t)e * a.dyn_stride, fr, M->n_bodies);
  __syncthreads();
  const bool target = a.task_id != MOCCA_TASK_CASSIE;   // the walkers' VSphere; Cassie's target lies 1 km ahead and is not drawn
  const int nrobot = stage_robot(M, fr, lane, out, PALETTE);   // the geoms, or the skeleton (mocca_scene.h)
  if (lane == 63 && target) {
    const uint32_t* tk = a.task + (size_t)e * MOCCA_TASK_WORDS;
    float* o = out + nrobot * PRIM_WORDS;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = o[4 + k] = __uint_as_float(tk[MOCCA_TW_WALK_TARGET_X + k]); o[8 + k] = TARGET_RGB[k]; }
    o[3] = 0.15f;   // VSphere(radius=0.15)
    o[7] = __int_as_float((int)MOCCA_RENDER_ID_TARGET);
    o[11] = __int_as_float(0);
  }
  const int npl = a.task_id == MOCCA_TASK_WALKER3D_STEPPER ? M->n_planks : 0;
  if (lane >= 32 && lane < 32 + npl) {   // the live planks, as the step kernel stages them (mocca_device.h stage_planks)
    const int k = lane - 32;
    stage_plank(M, a.terrain + (size_t)e * a.terrain_stride, k, out + MAX_PRIMS * PRIM_WORDS + k * PLANK_WORDS);
  }
  if (lane == 62) {
    float* o = out + MAX_PRIMS * PRIM_WORDS + MOCCA_MAX_PLANKS * PLANK_WORDS;
    o[0] = __int_as_float(nrobot + (target ? 1 : 0)); o[1] = __int_as_float(npl); o[2] = 0.0f; o[3] = 0.0f;
  }
}

__global__ __launch_bounds__(TILE * TILE) void raycast_kernel(const float* scenes, const float* cameras, int width, int height, int task_id,
                                                              int plank_shape, float ph0, float ph1, float ph2, HeightFieldBank bank,
                                                              const int32_t* env_ids, uint8_t* rgb, float* depth, int32_t* idout) {
  __shared__ float S[SCENE_WORDS];
  __shared__ float CAM[MOCCA_CAMERA_FLOATS];
  const int view = blockIdx.z, tid = threadIdx.y * TILE + threadIdx.x;
  const HeightField hf = env_heightfield(bank, bank.data ? env_ids[view] : 0);   // the grid and range of the view's env
  const float* sc = scenes + (size_t)view * SCENE_WORDS;
  for (int k = tid; k < SCENE_WORDS; k += TILE * TILE) S[k] = sc[k];
  if (tid < MOCCA_CAMERA_FLOATS) CAM[tid] = cameras[(size_t)view * MOCCA_CAMERA_FLOATS + tid];
  __syncthreads();
  const int px = blockIdx.x * TILE + threadIdx.x, py = blockIdx.y * TILE + threadIdx.y;
  if (px >= width || py >= height) return;
  const int n_prims = __float_as_int(S[MAX_PRIMS * PRIM_WORDS + MOCCA_MAX_PLANKS * PLANK_WORDS]);
  const int n_planks = __float_as_int(S[MAX_PRIMS * PRIM_WORDS + MOCCA_MAX_PLANKS * PLANK_WORDS + 1]);
  const float tnear = CAM[14], tfar = CAM[15];
  // pixel centres: column px, row py (row 0 on top) looks through ((px + 1/2) / W, (py + 1/2) / H) of the image plane
  const float sx = (2.0f * ((float)px + 0.5f) / (float)width - 1.0f) * CAM[12] * CAM[13];
  const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)height) * CAM[12];
  const float o[3] = {CAM[0], CAM[1], CAM[2]};
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = CAM[9 + k] + sx * CAM[3 + k] + sy * CAM[6 + k];

  // the nearest surface, its id and its normal: one routine with the depth camera (mocca_scene.h nearest_hit)
  const float ph[3] = {ph0, ph1, ph2};
  RayHit hit;
  const float best = nearest_hit<true>(S, n_prims, S + MAX_PRIMS * PRIM_WORDS, n_planks, plank_shape == MOCCA_PLANK_CYLINDER, ph,
                                       task_id == MOCCA_TASK_WALKER3D_CUSTOM || task_id == MOCCA_TASK_CASSIE, hf, o, d, tnear, tfar, &hit);
  const int id = hit.id, bestk = hit.bestk;
  const float nrm[3] = {hit.nrm[0], hit.nrm[1], hit.nrm[2]};

  const size_t pix = ((size_t)view * height + py) * width + px;
  if (depth) depth[pix] = best;
  if (idout) idout[pix] = id;
  if (rgb) {
    float col[3] = {BG[0], BG[1], BG[2]};
    float shade = 1.0f;
    if (id != MOCCA_RENDER_ID_NONE) {
      const float hp[3] = {o[0] + best * d[0], o[1] + best * d[1], o[2] + best * d[2]};
      if (bestk >= 0) { col[0] = S[bestk * PRIM_WORDS + 8]; col[1] = S[bestk * PRIM_WORDS + 9]; col[2] = S[bestk * PRIM_WORDS + 10]; }
      else if (id == MOCCA_RENDER_ID_GROUND) {
        const bool odd = (((int)floorf(hp[0]) + (int)floorf(hp[1])) & 1) != 0;   // 1 m squares
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = odd ? GROUND_B[k] : GROUND_A[k];
      } else if (id == MOCCA_RENDER_ID_HEIGHTFIELD) {
        const float span = hf.zmax - hf.zmin;
        float w = span > 0.0f ? (hp[2] - hf.zmin) / span : 0.0f;
        w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = HF_LOW[k] + w * (HF_HIGH[k] - HF_LOW[k]);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = PLANK_RGB[k];
      }
      const float nl = nrm[0] * LIGHT[0] + nrm[1] * LIGHT[1] + nrm[2] * LIGHT[2];
      shade = AMBIENT + (1.0f - AMBIENT) * fmaxf(nl, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = col[k] * shade * 255.0f + 0.5f;
      rgb[3 * pix + k] = (uint8_t)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
    }
  }
}

void launch_link_frames(hipStream_t s, const SceneArgs& a, int n, float* frames) {
  hipLaunchKernelGGL(link_frames_kernel, dim3((n + 63) / 64), dim3(64), 0, s, a, n, frames);
}
void launch_scene(hipStream_t s, const SceneArgs& a, const int32_t* env_ids, int n_envs, int n_views, float* scenes) {
  hipLaunchKernelGGL(scene_kernel, dim3(n_views), dim3(64), 0, s, a, env_ids, n_envs, scenes);
}
void launch_raycast(hipStream_t s, const float* scenes, const float* cameras, int n_views, int width, int height, int task_id, int plank_shape,
                    const float* plank_half, HeightFieldBank bank, const int32_t* env_ids, uint8_t* rgb, float* depth, int32_t* id) {
  const dim3 grid((width + TILE - 1) / TILE, (height + TILE - 1) / TILE, n_views);
  hipLaunchKernelGGL(raycast_kernel, grid, dim3(TILE, TILE), 0, s, scenes, cameras, width, height, task_id, plank_shape, plank_half[0],
                     plank_half[1], plank_half[2], bank, env_ids, rgb, depth, id);
}

}  // namespace mocca_rdr
