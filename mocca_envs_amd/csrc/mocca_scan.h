// mocca_scan.h -- launcher of mocca_scan.hip (the terrain height scan), called by the C ABI in mocca_api_sensors.hip (include/mocca.h mocca_height_scan).
#pragma once
#include "mocca_rays.h"

namespace mocca_scan {

struct ScanArgs {
  mocca_rdr::SceneArgs scene;      // the handle's records; read only
  mocca_rdr::HeightFieldBank hf;   // planner task: the bank, env e on its own grid; data == nullptr otherwise
  const float* points;             // [n_points][2] in the heading frame, device memory owned by the handle
  int n_points;
  float z_above, max_drop;
  float* out;                      // row e at out + e * row_stride: [obs (obs_dim) | scan (n_points)]
  int row_stride;
  const float* obs;                // [n_envs][obs_dim] copied in front of the scan, or nullptr (then obs_dim = 0)
  int obs_dim;
};

// one 64-lane workgroup per env, asynchronous on `s`
void launch_height_scan(hipStream_t s, const ScanArgs& a, int n_envs);

}  // namespace mocca_scan
