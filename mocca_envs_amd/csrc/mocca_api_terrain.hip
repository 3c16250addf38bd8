// mocca_api_terrain.hip -- the C ABI of the planner envs' terrain bank (include/mocca.h): the height fields, their generation on the device
// (mocca_terrain.h) and the field each env stands on.  Host code only: the handle and what crosses units are in mocca_handle.h.
#include "mocca_handle.h"

extern "C" {

// Attach a terrain bank (mocca_set_heightfield: a bank of one).  heights_host == nullptr: a bank of zeros.
static int attach_bank(const Call& c, const float* heights_host, int n_fields, int rows, int cols, double scale) {
  const mocca_handle h = c.h;
  if (rows < 2 || cols < 2 || !(scale > 0.0)) return c.bad("needs at least 2 x 2 heights and a positive scale");
  // Search window of every terrain contact slot: a sphere of reach rho = radius + margin around a centre that is at most half a cell from
  // its nearest grid point touches only cells within W = ceil(rho scale + 1/2) of that point (1e-6: a reach of exactly half a cell is W = 1).
  // W - 1 travels in bits 30..31 of the slot record; a grid so fine that a sphere spans more than 4 cells each way is refused.
  int wmax = 1;
  uint32_t wbits[MOCCA_MAX_SLOTS];
  for (int sl = 0; sl < h->model.n_slots; ++sl) {
    uint32_t ids; std::memcpy(&ids, &h->model.slot_tab[sl][2], 4);
    const double reach = (double)h->model.slot_tab[sl][0] + (double)((ids >> 17) & 0xFFu) / 8192.0;
    int w = (int)std::ceil(reach * scale + 0.5 - 1e-6);
    if (w < 1) w = 1;
    if (w > 4 && ((ids >> 25) & 1u)) return c.bad("the grid is too fine for this robot (a contact sphere would span more than 4 cells each way)");
    if (w > 4) w = 4;
    wbits[sl] = (ids & 0x3FFFFFFFu) | ((uint32_t)(w - 1) << 30);
    if (((ids >> 25) & 1u) && w > wmax) wmax = w;
  }
  const size_t cells = (size_t)rows * cols, stride = cells * wmax;
  if (stride > ((size_t)1 << 26) || stride * n_fields > ((size_t)1 << 30)) return c.bad("the bank is larger than 2^30 heights (pooled copies included)");
  DeviceGuard guard(h->device);
  // every field: the heights, followed by one max-pooled copy per window 2 .. wmax (copy k: the highest point within k + 1 cells of each grid
  // point): what a wide sphere's search is pruned by with one load.  Beside the bank, each field's range.
  std::vector<float> host, range((size_t)n_fields * 2, 0.0f);
  if (heights_host) {
    host.resize(stride * n_fields);
    for (int f = 0; f < n_fields; ++f) {
      const float* in = heights_host + cells * f;
      float* field = host.data() + stride * f;
      std::memcpy(field, in, cells * sizeof(float));
      for (int w = 2; w <= wmax; ++w) {
        float* out = field + cells * (w - 1);
        for (int j = 0; j < rows; ++j)
          for (int i = 0; i < cols; ++i) {
            float m = -1e30f;
            for (int jj = (j - w < 0 ? 0 : j - w); jj <= (j + w > rows - 1 ? rows - 1 : j + w); ++jj)
              for (int ii = (i - w < 0 ? 0 : i - w); ii <= (i + w > cols - 1 ? cols - 1 : i + w); ++ii)
                m = in[(size_t)jj * cols + ii] > m ? in[(size_t)jj * cols + ii] : m;
            out[(size_t)j * cols + i] = m;
          }
      }
      float zmin = in[0], zmax = in[0];
      for (size_t k = 1; k < cells; ++k) {
        zmin = in[k] < zmin ? in[k] : zmin;
        zmax = in[k] > zmax ? in[k] : zmax;
      }
      range[2 * (size_t)f] = zmin; range[2 * (size_t)f + 1] = zmax;
    }
  }
  // the window bits go into a COPY of the model; the handle's host image takes them only once the device has them
  auto next = std::make_unique<MoccaModel>(h->model);
  for (int sl = 0; sl < next->n_slots; ++sl) std::memcpy(&next->slot_tab[sl][2], &wbits[sl], 4);
  DevBuf<float> hf, rng, part;
  DevBuf<int32_t> field;
  hipError_t e = hf.alloc(stride * n_fields, !heights_host);
  if (e == hipSuccess && heights_host) e = hipMemcpy(hf, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = rng.alloc(range.size(), false);
  if (e == hipSuccess) e = hipMemcpy(rng, range.data(), range.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = part.alloc((size_t)n_fields * mocca_terrain::terrain_blocks(rows, cols) * 2, true);
  if (e == hipSuccess) e = field.alloc((size_t)h->n_envs, true);
  if (int rc = commit_ready(c, e)) return rc;   // no launch in flight still reads the old bank or the old slot records
  // the device model is rewritten in place: the last step that can fail, and one that fails leaves host and device records as they were
  if ((e = hipMemcpy(h->d_model, next.get(), sizeof(MoccaModel), hipMemcpyHostToDevice)) != hipSuccess) return c.hip("hipMemcpy(model)", e);
  h->model = *next;
  h->d_hf.swap(hf); h->d_hf_range.swap(rng); h->d_hf_part.swap(part); h->d_hf_field.swap(field);
  h->hf_rows = rows; h->hf_cols = cols; h->hf_scale = (float)scale;
  h->hf_n_fields = n_fields; h->hf_planes = wmax; h->hf_redraw = 0;
  return MOCCA_OK;
}

int mocca_set_heightfield(mocca_handle h, const float* heights_host, int rows, int cols, double scale) try {
  ENTRY(h, "mocca_set_heightfield");
  if (!heights_host) return c.bad("needs at least 2 x 2 heights and a positive scale");
  return attach_bank(c, heights_host, 1, rows, cols, scale);
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_set_heightfield")); }

int mocca_set_heightfield_bank(mocca_handle h, const float* heights_host, int n_fields, int rows, int cols, double scale) try {
  ENTRY(h, "mocca_set_heightfield_bank");
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER) return c.bad("only the planner task (Walker3DPlannerEnv, MikePlannerEnv) stands on height fields");
  if (!heights_host && n_fields == 0) {   // detach
    DeviceGuard guard(h->device);
    if (int rc = commit_ready(c)) return rc;
    h->d_hf.reset(); h->d_hf_range.reset(); h->d_hf_part.reset(); h->d_hf_field.reset();
    h->hf_rows = h->hf_cols = h->hf_n_fields = h->hf_redraw = 0; h->hf_planes = 1; h->hf_scale = 0.0f;
    return MOCCA_OK;
  }
  if (n_fields < 1 || n_fields > MOCCA_HF_MAX_FIELDS) return c.bad("n_fields must be 1 .. " + std::to_string(MOCCA_HF_MAX_FIELDS));
  return attach_bank(c, heights_host, n_fields, rows, cols, scale);
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_set_heightfield_bank")); }

// what the bank calls below share: a planner handle with a bank, and fields first .. first + count - 1 inside it
static int need_bank(const Call& c, int first, int count) {
  const mocca_handle h = c.h;
  if (h->task_id != MOCCA_TASK_WALKER3D_PLANNER || !h->d_hf) return c.bad("no terrain bank (mocca_set_heightfield_bank)");
  if (first < 0 || count < 1 || first > h->hf_n_fields - count)
    return c.bad("fields " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) + " are not inside the bank of " + std::to_string(h->hf_n_fields));
  return MOCCA_OK;
}

int mocca_generate_heightfields(mocca_handle h, int first, int count, uint64_t seed, int n_peaks, double gain, void* stream) try {
  ENTRY(h, "mocca_generate_heightfields");
  if (int rc = need_bank(c, first, count)) return rc;
  if ((h->hf_rows & 7) || (h->hf_cols & 7)) return c.bad("rows and cols must be multiples of 8 (the noise lattices of 4 and 8 cells divide them)");
  if (n_peaks < 1 || n_peaks > MOCCA_HF_MAX_PEAKS) return c.bad("n_peaks must be 1 .. " + std::to_string(MOCCA_HF_MAX_PEAKS));
  if (!std::isfinite(gain) || !(gain > 0.0)) return c.bad("gain must be finite and > 0");
  DeviceGuard guard(h->device);
  mocca_terrain::TerrainArgs a{};
  a.bank = h->d_hf; a.range = h->d_hf_range; a.part = h->d_hf_part;
  a.rows = h->hf_rows; a.cols = h->hf_cols; a.planes = h->hf_planes; a.stride = (size_t)h->hf_planes * h->hf_rows * h->hf_cols;
  a.scale = h->hf_scale; a.gain = (float)gain;
  a.first = first; a.count = count; a.n_peaks = n_peaks;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  mocca_terrain::launch_generate((hipStream_t)stream, a);
  return c.launched();
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_generate_heightfields")); }

int mocca_set_env_fields(mocca_handle h, const int32_t* field_dev, int redraw_at_reset, void* stream) try {
  ENTRY(h, "mocca_set_env_fields");
  if (int rc = need_bank(c, 0, 1)) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)h->n_envs * sizeof(int32_t);
  if (field_dev) {
    std::vector<int32_t> ids((size_t)h->n_envs);
    HIP_TRY(c, hipMemcpyAsync(ids.data(), field_dev, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (int e = 0; e < h->n_envs; ++e)
      if (ids[e] < 0 || ids[e] >= h->hf_n_fields)
        return c.bad("field " + std::to_string(ids[e]) + " (env " + std::to_string(e) + ") is outside 0 .. " + std::to_string(h->hf_n_fields - 1));
    HIP_TRY(c, hipMemcpyAsync(h->d_hf_field, field_dev, bytes, hipMemcpyDeviceToDevice, s));
  } else {
    HIP_TRY(c, hipMemsetAsync(h->d_hf_field, 0, bytes, s));
  }
  h->hf_redraw = redraw_at_reset != 0;
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_set_env_fields")); }

int mocca_get_env_fields(mocca_handle h, int32_t* field_dev, void* stream) try {
  ENTRY(h, "mocca_get_env_fields");
  if (!field_dev) return c.null_arg("field_dev");
  if (int rc = need_bank(c, 0, 1)) return rc;
  DeviceGuard guard(h->device);
  HIP_TRY(c, hipMemcpyAsync(field_dev, h->d_hf_field, (size_t)h->n_envs * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_get_env_fields")); }

int mocca_get_heightfields(mocca_handle h, int first, int count, float* out_dev, void* stream) try {
  ENTRY(h, "mocca_get_heightfields");
  if (!out_dev) return c.null_arg("out_dev");
  if (int rc = need_bank(c, first, count)) return rc;
  DeviceGuard guard(h->device);
  const size_t cells = (size_t)h->hf_rows * h->hf_cols, w = cells * sizeof(float);   // the heights of each field, without its pooled copies
  const float* src = h->d_hf.get() + cells * h->hf_planes * first;
  if (h->hf_planes == 1) HIP_TRY(c, hipMemcpyAsync(out_dev, src, w * count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  else
    for (int f = 0; f < count; ++f)
      HIP_TRY(c, hipMemcpyAsync(out_dev + cells * f, src + cells * h->hf_planes * f, w, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MOCCA_OK;
} catch (const std::bad_alloc&) { return out_of_host_memory(Call(h, "mocca_get_heightfields")); }

}  // extern "C"
