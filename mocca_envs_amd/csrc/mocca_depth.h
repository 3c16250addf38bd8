// mocca_depth.h -- launcher of mocca_depth.hip (the egocentric depth camera), called by the C ABI in mocca_api_sensors.hip (include/mocca.h mocca_depth_camera).
#pragma once
#include "mocca_rays.h"

namespace mocca_depth {

struct DepthArgs {
  mocca_rdr::SceneArgs scene;      // the handle's records; read only
  mocca_rdr::HeightFieldBank hf;   // planner task: the bank, env e on its own grid; data == nullptr otherwise
  int body;                        // the link the camera rides on, 0 .. n_bodies - 1 (clamped again in the kernel)
  float offset[3];                 // the eye in the body's frame
  float axes[9];                   // euler_to_mat(roll, pitch, yaw) of the mount: column 0 forward, column 2 up
  int width, height, flags;        // MOCCA_DEPTH_*; 1 <= width * height <= MOCCA_DEPTH_MAX_PIXELS
  float tan_half_fov, near, far;
  float* out;                      // row e at out + e * row_stride: [obs (obs_dim) | depth (width * height)]
  int row_stride;
  const float* obs;                // [n_envs][obs_dim] copied in front of the image, or nullptr (then obs_dim = 0)
  int obs_dim;
  float* cameras;                  // [n_envs][MOCCA_CAMERA_FLOATS]: the records the rays were cast from, or nullptr
};

// one 64-lane workgroup per env, asynchronous on `s`
void launch_depth_camera(hipStream_t s, const DepthArgs& a, int n_envs);

}  // namespace mocca_depth
