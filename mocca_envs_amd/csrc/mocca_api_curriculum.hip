// mocca_api_curriculum.hip -- the C ABI of the per-env adaptive curriculum of the Stepper envs (include/mocca.h mocca_set_curriculum ..
// mocca_curriculum_apply; the rule: mocca_curriculum.h).  The launch behind the step kernel is launch_step's (mocca_api.hip), with the
// arguments built here.  Host code only: see mocca_handle.h.
#include "mocca_handle.h"

mocca_cur::CurArgs curriculum_args(mocca_handle h, const uint8_t* done_dev, const int32_t* info_dev) {
  return mocca_cur::CurArgs{h->cur_cfg, h->d_task, MOCCA_TASK_WORDS, MOCCA_TW_EPISODE, h->env_offset, h->n_envs, (uint32_t)h->seed, (uint32_t)(h->seed >> 32),
                            done_dev, info_dev, h->d_pvec[0], h->d_cur_streak, h->d_cur_hold, h->cur_totals};
}

extern "C" {

int mocca_set_curriculum(mocca_handle h, const mocca_curriculum* cfg, float* level_totals_dev) {
  ENTRY(h, "mocca_set_curriculum");
  DeviceGuard guard(h->device);
  if (!cfg) {   // detach: the levels stay where they are, in the vector; the scalar MOCCA_PARAM_CURRICULUM is taken again
    if (int rc = commit_ready(c)) return rc;
    h->cur_on = false; h->cur_totals = nullptr;
    h->d_cur_streak.reset(); h->d_cur_hold.reset(); h->d_cur_info.reset();
    return MOCCA_OK;
  }
  if (h->task_id != MOCCA_TASK_WALKER3D_STEPPER) return c.bad("only MOCCA_TASK_WALKER3D_STEPPER has curriculum levels");
  if (cfg->demote_at >= cfg->promote_at) return c.bad("demote_at must be smaller than promote_at");
  if (cfg->patience < 1 || cfg->patience > MOCCA_CUR_MAX_PATIENCE) return c.bad("patience must be 1 .. " + std::to_string(MOCCA_CUR_MAX_PATIENCE));
  if (cfg->min_level < 0 || cfg->max_level < cfg->min_level || cfg->max_level > MOCCA_CUR_MAX_LEVEL)
    return c.bad("the levels must satisfy 0 <= min_level <= max_level <= " + std::to_string(MOCCA_CUR_MAX_LEVEL));
  if (cfg->recycle != 0 && cfg->recycle != 1) return c.bad("recycle must be 0 or 1");
  if ((long long)h->env_offset + h->n_envs > (1ll << 32) || h->env_offset < 0) return c.bad("the global env ids must stay below 2^32");
  const mocca_cur::CurConfig cur{cfg->promote_at, cfg->demote_at, cfg->patience, cfg->min_level, cfg->max_level, cfg->recycle};
  const size_t n = (size_t)h->n_envs;
  DevBuf<float> vec;
  DevBuf<int32_t> streak, hold, info;
  hipError_t e = streak.alloc(n, true);
  if (e == hipSuccess) e = hold.alloc(n, true);
  if (e == hipSuccess) e = info.alloc(n, true);
  if (e == hipSuccess && !h->d_pvec[0]) e = vec.alloc(n, false);
  if (e == hipSuccess) {   // the starting levels: the vector's where it is on, else the scalar level, clamped into the band
    mocca_cur::launch_curriculum_start(nullptr, cur, vec ? vec.get() : h->d_pvec[0].get(), h->pvec_on[0] ? 1 : 0, h->curriculum, h->n_envs);
    e = hipGetLastError();
  }
  if (int rc = commit_ready(c, e)) return rc;
  if (vec) h->d_pvec[0].swap(vec);
  h->d_cur_streak.swap(streak); h->d_cur_hold.swap(hold); h->d_cur_info.swap(info);
  h->pvec_on[0] = true;
  h->cur_cfg = cur; h->cur_totals = level_totals_dev; h->cur_on = true;
  return MOCCA_OK;
}

int mocca_get_curriculum(mocca_handle h, int32_t* level_dev, int32_t* streak_dev, int32_t* hold_dev, void* stream) {
  ENTRY(h, "mocca_get_curriculum");
  if (!h->cur_on) return c.needs("a curriculum", "mocca_set_curriculum");
  DeviceGuard guard(h->device);
  mocca_cur::launch_curriculum_get((hipStream_t)stream, h->d_pvec[0], h->d_cur_streak, h->d_cur_hold, h->n_envs, level_dev, streak_dev, hold_dev);
  return c.launched();
}

int mocca_curriculum_apply(mocca_handle h, const uint8_t* done_dev, const int32_t* info_dev, void* stream) {
  ENTRY(h, "mocca_curriculum_apply");
  if (!h->cur_on) return c.needs("a curriculum", "mocca_set_curriculum");
  if (!done_dev || !info_dev) return c.null_arg("done_dev or info_dev", " is NULL");
  DeviceGuard guard(h->device);
  mocca_cur::launch_curriculum((hipStream_t)stream, curriculum_args(h, done_dev, info_dev));
  return c.launched();
}

}  // extern "C"
