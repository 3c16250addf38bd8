// mocca_render.h -- launchers of mocca_render.hip (link frames, scene assembly, ray caster), called by the C ABI in mocca_api_sensors.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mocca.h"
#include "mocca_scene.h"

namespace mocca_rdr {

constexpr int TILE = 16;                               // a 16 x 16 pixel tile per workgroup: four waves
// one view's scene as the assembly kernel leaves it: [MAX_PRIMS][PRIM_WORDS] then [MOCCA_MAX_PLANKS][PLANK_WORDS] then {n_prims, n_planks, 0, 0}
constexpr int SCENE_WORDS = MAX_PRIMS * PRIM_WORDS + MOCCA_MAX_PLANKS * PLANK_WORDS + 4;
static_assert(SCENE_WORDS * 4 <= 2048, "the scene of one env stays under 2 KB of LDS");

// frames [n][n_bodies][15] of the handle's n envs
void launch_link_frames(hipStream_t s, const SceneArgs& a, int n, float* frames);
// scenes [n_views][SCENE_WORDS] of the listed envs (ids are clamped to 0 .. n_envs - 1)
void launch_scene(hipStream_t s, const SceneArgs& a, const int32_t* env_ids, int n_envs, int n_views, float* scenes);
// (bank.data != nullptr: view v sees the grid of env env_ids[v])
void launch_raycast(hipStream_t s, const float* scenes, const float* cameras, int n_views, int width, int height, int task_id, int plank_shape,
                    const float* plank_half, HeightFieldBank bank, const int32_t* env_ids, uint8_t* rgb, float* depth, int32_t* id);

}  // namespace mocca_rdr
