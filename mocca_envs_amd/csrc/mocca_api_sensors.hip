// mocca_api_sensors.hip -- the C ABI of what a trainer reads of the envs beside the observation (include/mocca.h): link frames and the ray
// caster (mocca_render.h), the terrain height scan (mocca_scan.h), the depth camera (mocca_depth.h), the observation-action history
// (mocca_history.h), and domain randomisation with its sensor noise (mocca_randomise.h).  Host code only: see mocca_handle.h.
#include "mocca_handle.h"

extern "C" {

int mocca_get_link_frames(mocca_handle h, float* frames_dev, void* stream) {
  ENTRY(h, "mocca_get_link_frames");
  if (!frames_dev) return c.null_arg("frames_dev");
  DeviceGuard guard(h->device);
  mocca_rdr::launch_link_frames((hipStream_t)stream, scene_args(h), h->n_envs, frames_dev);
  return c.launched();
}

int mocca_render(mocca_handle h, const int32_t* env_ids_dev, int n_views, const float* cameras_dev, int width, int height, uint8_t* rgb_dev,
                 float* depth_dev, int32_t* id_dev, void* stream) try {
  ENTRY(h, "mocca_render");
  if (!env_ids_dev || !cameras_dev) return c.null_arg("env_ids_dev and cameras_dev");
  if (n_views < 1 || n_views > 65535) return c.bad("n_views must be 1 .. 65535");
  if (width < 1 || height < 1 || width > MOCCA_RENDER_MAX_SIZE || height > MOCCA_RENDER_MAX_SIZE)
    return c.bad("width and height must be 1 .. " + std::to_string(MOCCA_RENDER_MAX_SIZE));
  if (need_heightfield(c, "mocca_render: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> ids((size_t)n_views);
  HIP_TRY(c, hipMemcpyAsync(ids.data(), env_ids_dev, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (int v = 0; v < n_views; ++v)
    if (ids[v] < 0 || ids[v] >= h->n_envs)
      return c.bad("env index " + std::to_string(ids[v]) + " (view " + std::to_string(v) + ") is outside 0 .. " + std::to_string(h->n_envs - 1));
  if (n_views > h->scenes_cap) {   // grow: an earlier render in flight may still read the old scenes
    DevBuf<float> scenes;
    if (int rc = commit_ready(c, scenes.alloc((size_t)n_views * mocca_rdr::SCENE_WORDS, false))) return rc;
    h->d_scenes.swap(scenes);
    h->scenes_cap = n_views;
  }
  if (int rc = flush_pending(c, s)) return rc;
  mocca_rdr::launch_scene(s, scene_args(h), env_ids_dev, h->n_envs, n_views, h->d_scenes);
  HIP_TRY(c, hipGetLastError());
  mocca_rdr::launch_raycast(s, h->d_scenes, cameras_dev, n_views, width, height, h->task_id, h->model.plank_shape, h->model.plank_half,
                            heightfield_record(h), env_ids_dev, rgb_dev, depth_dev, id_dev);
  return c.launched();
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_render")); }

int mocca_set_height_scan(mocca_handle h, const float* points_host, int n_points, double z_above, double max_drop) {
  ENTRY(h, "mocca_set_height_scan");
  DeviceGuard guard(h->device);
  if (!points_host) {   // detach
    if (int rc = commit_ready(c)) return rc;
    h->d_scan_pts.reset(); h->scan_n = 0;
    return MOCCA_OK;
  }
  if (n_points < 1 || n_points > MOCCA_SCAN_MAX_POINTS) return c.bad("n_points must be 1 .. " + std::to_string(MOCCA_SCAN_MAX_POINTS));
  if (!std::isfinite(z_above) || !std::isfinite(max_drop) || z_above < 0.0 || !(max_drop > 0.0)) return c.bad("needs a finite z_above >= 0 and max_drop > 0");
  for (int k = 0; k < 2 * n_points; ++k)
    if (!std::isfinite(points_host[k])) return c.bad("point " + std::to_string(k / 2) + " is not finite");
  DevBuf<float> pts;
  hipError_t e = pts.alloc((size_t)n_points * 2, false);
  if (e == hipSuccess) e = hipMemcpy(pts, points_host, (size_t)n_points * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(c, e)) return rc;
  h->d_scan_pts.swap(pts);
  h->scan_n = n_points; h->scan_above = (float)z_above; h->scan_drop = (float)max_drop;
  return MOCCA_OK;
}

int mocca_scan_dim(mocca_handle h) { return h ? h->scan_n : Call(h, "mocca_scan_dim").null_handle(); }

int mocca_height_scan(mocca_handle h, float* out_dev, int row_stride, const float* obs_dev, void* stream) {
  ENTRY(h, "mocca_height_scan");
  if (!h->d_scan_pts) return c.bad("no scan pattern (mocca_set_height_scan)");
  if (!out_dev) return c.null_arg("out_dev");
  const int width = h->scan_n + (obs_dev ? h->obs_dim : 0);
  if (row_stride < width)
    return c.small_stride("row_stride", row_stride, "the row (" + std::to_string(width) + " floats)");
  if (need_heightfield(c, "mocca_height_scan: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  mocca_scan::ScanArgs a{};
  a.scene = scene_args(h);
  a.hf = heightfield_record(h);
  a.points = h->d_scan_pts; a.n_points = h->scan_n; a.z_above = h->scan_above; a.max_drop = h->scan_drop;
  a.out = out_dev; a.row_stride = row_stride; a.obs = obs_dev; a.obs_dim = obs_dev ? h->obs_dim : 0;
  mocca_scan::launch_height_scan((hipStream_t)stream, a, h->n_envs);
  return c.launched();
}

int mocca_set_depth_camera(mocca_handle h, int body, const float* mount_host, int width, int height, double fov_y, double near, double far, int flags) {
  ENTRY(h, "mocca_set_depth_camera");
  if (!mount_host) {   // detach
    h->depth_on = false;
    return MOCCA_OK;
  }
  if (body < 0 || body >= h->model.n_bodies) return c.bad("body " + std::to_string(body) + " is outside 0 .. " + std::to_string(h->model.n_bodies - 1));
  if (width < 1 || width > 64 || height < 1 || height > 64 || width * height > MOCCA_DEPTH_MAX_PIXELS)
    return c.bad("width and height must be 1 .. 64 and their product at most " + std::to_string(MOCCA_DEPTH_MAX_PIXELS));
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(mount_host[k])) return c.bad("mount entry " + std::to_string(k) + " is not finite");
  if (!(fov_y > 0.0 && fov_y < 3.14159265358979323846)) return c.bad("fov_y must lie in (0, pi) radians");
  if (!std::isfinite(near) || !std::isfinite(far) || !(near > 0.0) || !(far > near)) return c.bad("needs finite 0 < near < far");
  if (flags & ~(MOCCA_DEPTH_STABILISED | MOCCA_DEPTH_SEE_ROBOT)) return c.bad("unknown flag bits " + std::to_string(flags & ~(MOCCA_DEPTH_STABILISED | MOCCA_DEPTH_SEE_ROBOT)));
  mocca_depth::DepthArgs a{};
  a.body = body; a.width = width; a.height = height; a.flags = flags;
  for (int k = 0; k < 3; ++k) a.offset[k] = mount_host[k];
  mocca_rdr::euler_to_mat(mount_host[3], mount_host[4], mount_host[5], a.axes);
  a.tan_half_fov = (float)std::tan(0.5 * fov_y); a.near = (float)near; a.far = (float)far;
  if (!std::isfinite(a.tan_half_fov) || !(a.near > 0.0f) || !(a.far > a.near)) return c.bad("fov_y, near and far must stay distinct and finite in float32");
  h->depth = a; h->depth_on = true;
  return MOCCA_OK;
}

int mocca_depth_dim(mocca_handle h) { return h ? (h->depth_on ? h->depth.width * h->depth.height : 0) : Call(h, "mocca_depth_dim").null_handle(); }

int mocca_depth_camera(mocca_handle h, float* out_dev, int row_stride, const float* obs_dev, float* cameras_dev, void* stream) {
  ENTRY(h, "mocca_depth_camera");
  if (!h->depth_on) return c.bad("no camera (mocca_set_depth_camera)");
  if (!out_dev) return c.null_arg("out_dev");
  const int width = h->depth.width * h->depth.height + (obs_dev ? h->obs_dim : 0);
  if (row_stride < width)
    return c.small_stride("row_stride", row_stride, "the row (" + std::to_string(width) + " floats)");
  if (need_heightfield(c, "mocca_depth_camera: ", "first") != MOCCA_OK) return MOCCA_E_ARG;
  DeviceGuard guard(h->device);
  mocca_depth::DepthArgs a = h->depth;
  a.scene = scene_args(h);
  a.hf = heightfield_record(h);
  a.out = out_dev; a.row_stride = row_stride; a.obs = obs_dev; a.obs_dim = obs_dev ? h->obs_dim : 0; a.cameras = cameras_dev;
  mocca_depth::launch_depth_camera((hipStream_t)stream, a, h->n_envs);
  return c.launched();
}

// ---- the observation-action history (mocca_history.h) ----
int mocca_set_history(mocca_handle h, const int32_t* cols_host, int n_cols, int act_dim, int steps, int stride) {
  ENTRY(h, "mocca_set_history");
  DeviceGuard guard(h->device);
  if (steps == 0) {   // detach
    if (int rc = commit_ready(c)) return rc;
    h->hist_cfg = mocca_hist::HistConfig{}; h->d_hist_cols.reset(); h->d_hist_ring.reset(); h->d_hist_tags.reset();
    return MOCCA_OK;
  }
  if (steps < 1 || steps > MOCCA_HIST_MAX_STEPS) return c.bad("steps must be 1 .. " + std::to_string(MOCCA_HIST_MAX_STEPS) + " (0 detaches)");
  if (stride < 1 || stride > MOCCA_HIST_MAX_STRIDE) return c.bad("stride must be 1 .. " + std::to_string(MOCCA_HIST_MAX_STRIDE));
  if (act_dim < 0 || act_dim > mocca_hist::HIST_MAX_ACT) return c.bad("act_dim must be 0 .. " + std::to_string(mocca_hist::HIST_MAX_ACT));
  if (n_cols < 0 || n_cols > h->obs_dim || (n_cols > 0 && !cols_host))
    return c.bad("n_cols must be 0 .. obs_dim (" + std::to_string(h->obs_dim) + "), with that many columns");
  if (n_cols + act_dim == 0) return c.bad("a frame needs at least one observation column or one action entry");
  std::vector<char> seen((size_t)h->obs_dim, 0);
  for (int k = 0; k < n_cols; ++k) {
    const int col = cols_host[k];
    if (col < 0 || col >= h->obs_dim) return c.bad("column " + std::to_string(col) + " is outside 0 .. " + std::to_string(h->obs_dim - 1));
    if (seen[col]) return c.bad("column " + std::to_string(col) + " is repeated");
    seen[col] = 1;
  }
  const mocca_hist::HistConfig cfg{steps, stride, n_cols, act_dim};
  if (mocca_hist::hist_dim(cfg) > MOCCA_HIST_MAX_DIM)
    return c.bad("the block has steps x (n_cols + act_dim) = " + std::to_string(mocca_hist::hist_dim(cfg)) + " floats, at most " +
                  std::to_string(MOCCA_HIST_MAX_DIM));
  const size_t n_slots = (size_t)h->n_envs * mocca_hist::hist_slots(cfg);
  if ((size_t)h->n_envs * mocca_hist::hist_dim(cfg) >= ((size_t)1 << 31)) return c.bad("n_envs x the block width must stay below 2^31");
  DevBuf<int32_t> cols;
  DevBuf<float> ring;
  DevBuf<uint32_t> tags;
  hipError_t e = cols.alloc((size_t)(n_cols > 0 ? n_cols : 1), true);
  if (e == hipSuccess && n_cols > 0) e = hipMemcpy(cols, cols_host, (size_t)n_cols * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ring.alloc(n_slots * mocca_hist::hist_width(cfg), true);
  if (e == hipSuccess) e = tags.alloc(n_slots * 2, false);
  if (e == hipSuccess) e = hipMemset(tags, 0xFF, n_slots * 2 * sizeof(uint32_t));   // every tag word HIST_NO_T: a frame no episode holds
  if (int rc = commit_ready(c, e)) return rc;
  h->d_hist_cols.swap(cols); h->d_hist_ring.swap(ring); h->d_hist_tags.swap(tags);
  h->hist_cfg = cfg;
  return MOCCA_OK;
}

int mocca_history_dim(mocca_handle h) {
  ENTRY(h, "mocca_history_dim");
  if (h->hist_cfg.steps == 0) return c.needs("a history", "mocca_set_history");
  return mocca_hist::hist_dim(h->hist_cfg);
}

int mocca_history(mocca_handle h, const float* rows_dev, int row_stride, const float* act_dev, int act_stride, float* out_dev, int out_stride,
                  void* stream) {
  ENTRY(h, "mocca_history");
  const mocca_hist::HistConfig& cfg = h->hist_cfg;
  if (cfg.steps == 0) return c.needs("a history", "mocca_set_history");
  if (!rows_dev || !out_dev) return c.null_arg("rows_dev or out_dev", " is NULL");
  if (row_stride < h->obs_dim) return c.bad("row_stride must be at least obs_dim (" + std::to_string(h->obs_dim) + ")");
  if (out_stride < mocca_hist::hist_dim(cfg))
    return c.bad("out_stride must be at least the block width (" + std::to_string(mocca_hist::hist_dim(cfg)) + ")");
  if (act_dev && act_stride < cfg.act_dim)
    return c.bad("act_stride must be at least the history's act_dim (" + std::to_string(cfg.act_dim) + ")");
  DeviceGuard guard(h->device);
  mocca_hist::HistArgs a{cfg, h->d_task, MOCCA_TASK_WORDS, MOCCA_TW_T, MOCCA_TW_EPISODE, h->n_envs, h->d_hist_cols, h->d_hist_ring, h->d_hist_tags,
                         rows_dev, act_dev, out_dev, row_stride, act_stride, out_stride};
  mocca_hist::launch_history((hipStream_t)stream, a);
  return c.launched();
}

// ---- domain randomisation (mocca_randomise.h) ----
int mocca_set_randomisation(mocca_handle h, const mocca_randomisation* cfg) {
  ENTRY(h, "mocca_set_randomisation");
  DeviceGuard guard(h->device);
  if (!cfg) {   // detach: the next step reads the caller's actions again
    if (int rc = commit_ready(c)) return rc;
    h->rand_on = false; h->d_rand_eff.reset(); h->d_rand_ring.reset();
    return MOCCA_OK;
  }
  const float lo = (float)cfg->strength_lo, hi = (float)cfg->strength_hi, pm = (float)cfg->push_max;
  if (!(lo > 0.0f) || !(hi <= 1.0f) || !(lo <= hi)) return c.bad("the strength range must satisfy 0 < strength_lo <= strength_hi <= 1");
  if (h->task_id == MOCCA_TASK_CASSIE && (lo != 1.0f || hi != 1.0f))
    return c.bad("MOCCA_TASK_CASSIE takes the strength range [1, 1] alone: its action is a PD target, not a torque");
  if (cfg->delay_min < 0 || cfg->delay_max < cfg->delay_min || cfg->delay_max > MOCCA_RAND_MAX_DELAY)
    return c.bad("the delays must satisfy 0 <= delay_min <= delay_max <= " + std::to_string(MOCCA_RAND_MAX_DELAY));
  if (!std::isfinite(pm) || pm < 0.0f) return c.bad("push_max must be finite and not negative");
  if (cfg->push_interval < 0 || cfg->push_interval > mocca_rand::RAND_MAX_INTERVAL)
    return c.bad("push_interval must be 0 (no pushes) .. " + std::to_string(mocca_rand::RAND_MAX_INTERVAL));
  const int ad = mocca_act_dim(h);
  const size_t n_eff = (size_t)h->n_envs * ad, n_ring = n_eff * (cfg->delay_max + 1);
  if (n_eff >= ((size_t)1 << 31) || (long long)h->env_offset + h->n_envs > (1ll << 32) || h->env_offset < 0)
    return c.bad("n_envs x act_dim must stay below 2^31 and the global env ids below 2^32");
  DevBuf<float> eff, ring;
  hipError_t e = eff.alloc(n_eff, true);
  if (e == hipSuccess) e = ring.alloc(n_ring, true);
  if (int rc = commit_ready(c, e)) return rc;
  h->d_rand_eff.swap(eff); h->d_rand_ring.swap(ring);
  h->rand_cfg = mocca_rand::RandConfig{lo, hi, cfg->delay_min, cfg->delay_max, cfg->push_interval, pm, h->planar};
  h->rand_on = true;
  return MOCCA_OK;
}

int mocca_get_effective_action(mocca_handle h, float* out_dev, void* stream) {
  ENTRY(h, "mocca_get_effective_action");
  if (!h->rand_on) return c.needs("a randomisation", "mocca_set_randomisation");
  if (!out_dev) return c.null_arg("out_dev", " is NULL");
  DeviceGuard guard(h->device);
  HIP_TRY(c, hipMemcpyAsync(out_dev, h->d_rand_eff, (size_t)h->n_envs * mocca_act_dim(h) * sizeof(float), hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
  return MOCCA_OK;
}

int mocca_set_sensor_noise(mocca_handle h, const float* scale_host, int dim) {
  ENTRY(h, "mocca_set_sensor_noise");
  DeviceGuard guard(h->device);
  if (!scale_host) {
    if (int rc = commit_ready(c)) return rc;
    h->d_noise_scale.reset();
    return MOCCA_OK;
  }
  if (dim != h->obs_dim) return c.bad("dim must be obs_dim (" + std::to_string(h->obs_dim) + ")");
  for (int k = 0; k < dim; ++k)
    if (!std::isfinite(scale_host[k]) || scale_host[k] < 0.0f)
      return c.bad("scale " + std::to_string(k) + " must be finite and not negative");
  if ((size_t)h->n_envs * dim >= ((size_t)1 << 31)) return c.bad("n_envs x dim must stay below 2^31");
  DevBuf<float> sc;
  hipError_t e = sc.alloc(dim, false);
  if (e == hipSuccess) e = hipMemcpy(sc, scale_host, (size_t)dim * sizeof(float), hipMemcpyHostToDevice);
  if (int rc = commit_ready(c, e)) return rc;
  h->d_noise_scale.swap(sc);
  return MOCCA_OK;
}

int mocca_sensor_noise(mocca_handle h, const float* rows_dev, int in_stride, float* out_dev, int out_stride, void* stream) {
  ENTRY(h, "mocca_sensor_noise");
  if (!h->d_noise_scale) return c.needs("the scales", "mocca_set_sensor_noise");
  if (!rows_dev || !out_dev) return c.null_arg("rows_dev or out_dev", " is NULL");
  if (in_stride < h->obs_dim || out_stride < h->obs_dim)
    return c.bad("in_stride and out_stride must be at least obs_dim (" + std::to_string(h->obs_dim) + ")");
  DeviceGuard guard(h->device);
  mocca_rand::NoiseArgs a{rand_keys(h), h->d_noise_scale, rows_dev, out_dev, in_stride, out_stride, h->obs_dim};
  mocca_rand::launch_noise((hipStream_t)stream, a);
  return c.launched();
}

int mocca_randomisation_record(mocca_handle h, float* out_dev, int row_stride, void* stream) {
  ENTRY(h, "mocca_randomisation_record");
  if (!h->rand_on) return c.needs("a randomisation", "mocca_set_randomisation");
  if (!out_dev) return c.null_arg("out_dev", " is NULL");
  if (row_stride < MOCCA_RAND_WORDS)
    return c.bad("row_stride must be at least MOCCA_RAND_WORDS (" + std::to_string(MOCCA_RAND_WORDS) + ")");
  DeviceGuard guard(h->device);
  mocca_rand::RecordArgs a{rand_keys(h), h->rand_cfg, out_dev, row_stride};
  mocca_rand::launch_record((hipStream_t)stream, a);
  return c.launched();
}

}  // extern "C"
