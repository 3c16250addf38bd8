// mocca_mlp.h -- what the three MFMA MLP kernels share (controller_kernel, policy_kernel, ppo_rows_kernel): the layer loop, the activation
// of the two forward-only kernels and the input stage's normalisation.  Device code only; the layer table and the fragment order of the
// weights: mocca_controller.h.
//
// Summation: an output is the sum of FOUR partial sums, one accumulator per MFMA j of a 16-wide k-group (the k with k mod 4 = j), each in
// ascending k, added as (p0 + p1) + (p2 + p3) ahead of the epilogue.  The order does not depend on the batch: same inputs -> same bits.
// Nothing below multiplies into an add, so the includer's fp-contract setting does not reach these functions.
#pragma once
#include <hip/hip_runtime.h>

#include "mocca_controller.h"

namespace mocca_mlp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NP = 4;   // partial sums per output
constexpr int NT = 4;   // output tiles per wave: 16 tiles of 16 rows (width 256) over 4 waves

// the forward-only kernels' activation (ppo_rows_kernel has its own, rounded once: its stored activations feed dW)
__device__ __forceinline__ float activate(float x, int act) {
  switch (act) {
    case mocca_ctrl::CTRL_ACT_RELU: return fmaxf(x, 0.0f);
    case mocca_ctrl::CTRL_ACT_TANH: return tanhf(x);
    case mocca_ctrl::CTRL_ACT_SOFTSIGN: return x / (1.0f + fabsf(x));
    default: return x;
  }
}

// the input stage's line: f32, in this operation order (mocca_policy.h: Image)
__device__ __forceinline__ float normalise(float v, float mean, float inv_std, float clip) {
  return fminf(fmaxf((v - mean) * inv_std, -clip), clip);
}

// out[o][col] = sum_k W[o][k] Xin[col][k] for the 16 columns of the workgroup (four waves): Xin in LDS, STRIDE floats per column; W in
// fragment order [n_ot][nkg][64][4], streamed from L2.  The 16-row output tiles are dealt to the waves round robin (wave w: tiles w, w + 4,
// w + 8, w + 12), so no weight is read twice by a workgroup; the B operand is one ds_read_b128 that serves four MFMAs and every tile of the
// wave.  epi(o, sum) receives rows o .. o + 3 of column `col` (lane & 15), sum = (p0 + p1) + (p2 + p3).
template <int STRIDE, class Epi>
__device__ __forceinline__ void mfma_layer(const f32x4* W, int nkg, int n_ot, const float* Xin, int wave, int lane, Epi epi) {
  const int col = lane & 15, quad = lane >> 4;
  const int nt_w = wave < n_ot ? (n_ot - wave + 3) >> 2 : 0;   // output tiles of this wave (wave-uniform)
  if (nt_w == 0) return;
  f32x4 acc[NT][NP];   // [..][j]: the partial sum fed by MFMA j of every k-group
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[t][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // weight fragments of this wave's tiles at k-group kg (tiles past the wave's last re-read that one: loaded, never multiplied)
  const f32x4* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ot = wave + 4 * (t < nt_w ? t : nt_w - 1);
    wp[t] = W + (size_t)ot * nkg * 64 + lane;
  }
  // the weights come from L2 (hundreds of cycles): the fragments of k-groups kg + 1 and kg + 2 are in flight while kg multiplies
  f32x4 w0[NT], w1[NT], w2[NT];
  auto load = [&](f32x4 (&w)[NT], int kg) {
    const int kc = kg < nkg ? kg : nkg - 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = wp[t][(size_t)kc * 64];
  };
  auto multiply = [&](const f32x4 (&w)[NT], int kg) {
    const f32x4 b = *(const f32x4*)&Xin[col * STRIDE + kg * 16 + quad * 4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt_w) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][j], b[j], acc[t][j], 0, 0, 0);
      }
  };
  // three k-groups per trip: the three fragment sets rotate by name, not by register moves
  load(w0, 0); load(w1, 1);
#pragma unroll 1
  for (int kg = 0; kg < nkg; kg += 3) {
    load(w2, kg + 2); multiply(w0, kg);
    if (kg + 1 >= nkg) break;
    load(w0, kg + 3); multiply(w1, kg + 1);
    if (kg + 2 >= nkg) break;
    load(w1, kg + 4); multiply(w2, kg + 2);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt_w) epi((wave + 4 * t) * 16 + quad * 4, (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]));
}

}  // namespace mocca_mlp
