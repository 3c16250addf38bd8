// mocca_ppo.hip -- PPO's minibatch loss and its gradient with respect to every parameter of the Gaussian actor-critic, plain (mocca_ppo_grad),
// mirror-symmetric (mocca_ppo_grad_sym), plain with the mirror-symmetry loss added (mocca_ppo_grad_mirror) or plain on mirror-duplicated
// rows (mocca_ppo_grad_dup), on the device.  What each launch does, the scratch and the transposed weight copy: mocca_ppo.h.
// The loss and the per-row formulas: include/mocca.h.
//
// Arithmetic: the policy kernel's (mocca_policy.hip), on the layer loop both share (mocca_mlp.h: mfma_layer, the epilogue a parameter): the
// forward adds the bias, activates and also stores the output to scratch; the backward (the same loop over the transposed copy) stores dA
// to LDS only.  The forward's activation is this file's own, activate_once: tanh rounded once, where the policy kernel's is tanhf.
#include <hip/hip_runtime.h>

#include "mocca_mlp.h"
#include "mocca_ppo.h"

// every f32 / f64 operation written below is that IEEE operation: a * b + c stays two roundings (include/mocca.h names each of them)
#pragma clang fp contract(off)

namespace mocca_ppo {

using namespace mocca_ctrl;   // CL_*, CTRL_ACT_*
using namespace mocca_pol;
using mocca_mlp::f32x4;
using mocca_mlp::mfma_layer;
using mocca_mlp::NP;

constexpr int LDS_STRIDE = POL_MAX_IN + 4;   // the policy kernel's LDS row
constexpr int TILE = POL_TILE;
static_assert(TILE == 16, "one 16-row MFMA sub-tile per workgroup");
static_assert(2 * PPO_SYM_TILE == TILE, "the symmetric instance: column c the row as given, column PPO_SYM_TILE + c its mirror image");

// NOT mocca_mlp::activate (tanhf), and named apart from it so that neither can stand in for the other
__device__ __forceinline__ float activate_once(float x, int act) {
  switch (act) {
    case CTRL_ACT_RELU: return fmaxf(x, 0.0f);
    case CTRL_ACT_TANH: return (float)tanh((double)x);   // rounded once: the stored activations feed dW, and tanhf's 2 ulp showed in small nets
    case CTRL_ACT_SOFTSIGN: return x / (1.0f + fabsf(x));
    default: return x;
  }
}
// the activation's derivative, from its INPUT x: where the unit saturates, 1 - y y and (1 - |y|)^2 cancel and carry the rounding of y
// magnified by 1 / (1 - |y|); from x the derivative keeps a few ulp of relative error at any x
__device__ __forceinline__ float activate_slope(float x, int act) {
  switch (act) {
    case CTRL_ACT_RELU: return x > 0.0f ? 1.0f : 0.0f;
    case CTRL_ACT_TANH: { const float e = expf(-2.0f * fabsf(x)), d = 1.0f + e; return (4.0f * e) / (d * d); }   // sech^2 x
    case CTRL_ACT_SOFTSIGN: { const float u = 1.0f / (1.0f + fabsf(x)); return u * u; }
    default: return 1.0f;
  }
}

// MODE (header: Symmetric policy, Mirror loss, Duplicated rows).  PPO_SYM, PPO_MIRROR and PPO_DUP (SYM below): the 16 MFMA columns are PPO_SYM_TILE = 8 minibatch rows x
// {as given, mirrored} -- policy_kernel<true>'s layout: column c is row row0 + c, column 8 + c its mirror image -- and column e's activations
// live in scratch row 16 * tile + e.  The plain instance has one column per row and scratch row = minibatch row.
// PPO_SYM's head stage symmetrises mean, log_std and value over the two columns; PPO_MIRROR's leaves the policy the as-given column's and
// adds the mirror term over the actor's two columns, and its critic's mirrored columns are not live.  PPO_DUP's runs the plain per-row lines
// on each of the 16 columns by itself: a mirrored column is one more sample, with the action mirrored too.
// PPO_DISTIL (header: Distillation): the plain instance -- one column per row, its staging, layer loop and backward -- with the regression head stage.
// PPO_PRIV (header: Privileged critic): the plain instance with the critic's workgroups staging the critic's own rows, to A0c.
template <int MODE>
__global__ __launch_bounds__(256, 2) void ppo_rows_kernel(PpoArgs a) {
  __shared__ __attribute__((aligned(16))) float X[2][TILE * LDS_STRIDE];
  constexpr bool DISTIL = MODE == PPO_DISTIL; // the regression head stage on the plain layout
  constexpr bool PRIV = MODE == PPO_PRIV;     // the critic's own staging on the plain layout (header: Privileged critic)
  constexpr bool SYM = MODE != PPO_PLAIN && !DISTIL && !PRIV;   // the two-column layout
  constexpr bool NET = MODE == PPO_SYM;       // the symmetric network's head stage
  constexpr bool ML = MODE == PPO_MIRROR;     // the mirror loss's head stage
  constexpr bool DUP = MODE == PPO_DUP;       // duplicated rows: the plain head stage, one lane per COLUMN
  constexpr bool PAIR = NET || ML;            // a head lane owns a row's two columns
  constexpr int ROWS = SYM ? PPO_SYM_TILE : TILE;   // minibatch rows of a workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS, srow0 = blockIdx.x * TILE, net = blockIdx.y;
  const int col = lane & 15;
  const int B = a.n_rows;

  // input: the policy kernel's staging, the rows gathered through idx; the normalised tile also goes to A0.  SYM: column e >= ROWS is the
  // mirror image of row e - ROWS, formed from the RAW row through in_perm / in_sign and normalised by k
  // PRIV: a second copy of the loop, not one loop over parameters -- folded into one lambda the two made the compiler move instructions in all
  // five existing instances, which are held to the instruction streams they had (profiles/kernel_resources_priv_critic.md)
  if (PRIV && net == 1) {   // the critic's own rows and statistics, the tile to A0c: the loop below, field for field
    const bool norm = a.params[a.flags_off] != 0.0f;
    const float *mu = a.params + a.critic_mean_off, *is = a.params + a.critic_inv_std_off;
    float* A0c = a.scratch + a.a0c_off;
    for (int i = tid; i < TILE * a.critic_in_pad; i += 256) {
      const int e = i / a.critic_in_pad, k = i - e * a.critic_in_pad, row = row0 + e;
      float v = 0.0f;
      if (row < B && k < a.critic_in_dim) {
        const long long src = a.idx ? (long long)a.idx[row] : row;
        v = a.critic_obs[(size_t)src * a.critic_stride + k];
        if (norm) v = fminf(fmaxf((v - mu[k]) * is[k], -a.norm_clip), a.norm_clip);
      }
      X[0][e * LDS_STRIDE + k] = v;
      A0c[(size_t)(srow0 + e) * a.critic_in_pad + k] = v;
    }
  } else {
    const bool norm = a.params[a.flags_off] != 0.0f;
    const float *mu = a.params + a.mean_off, *is = a.params + a.inv_std_off;
    float* A0 = a.scratch + a.a0_off;
    for (int i = tid; i < TILE * a.in_pad; i += 256) {
      const int e = i / a.in_pad, k = i - e * a.in_pad, row = row0 + (SYM ? e & (ROWS - 1) : e);
      float v = 0.0f;
      if (row < B && k < a.in_dim) {
        const long long src = a.idx ? (long long)a.idx[row] : row;
        if (SYM && e >= ROWS) v = a.obs[(size_t)src * a.obs_stride + a.in_perm[k]] * a.in_sign[k];
        else v = a.obs[(size_t)src * a.obs_stride + k];
        if (norm) v = fminf(fmaxf((v - mu[k]) * is[k], -a.norm_clip), a.norm_clip);
      }
      X[0][e * LDS_STRIDE + k] = v;
      if (net == 0) A0[(size_t)(srow0 + e) * a.in_pad + k] = v;
    }
  }
  __syncthreads();

  const int first = net == 0 ? 0 : a.n_actor, count = net == 0 ? a.n_actor : a.n_critic;
  // this lane's MFMA column is a row of the minibatch (SYM: or its mirror image; ML: the critic has no use for the mirror image)
  const bool live = row0 + (SYM ? col & (ROWS - 1) : col) < B && !(ML && net == 1 && col >= ROWS);
  int cur = 0;
#pragma unroll 1
  for (int li = 0; li < count; ++li) {
    const int32_t* lr = a.layers + (size_t)(first + li) * CTRL_LAYER_WORDS;
    const int out_pad = lr[CL_OUT_PAD], act = lr[CL_ACT];
    const float* Bias = a.params + lr[CL_B_OFF];
    float* Xout = X[cur ^ 1];
    float* Y = a.scratch + a.a_off[first + li] + (size_t)(srow0 + col) * out_pad;
    float* S = a.scratch + a.dz_off[first + li] + (size_t)(srow0 + col) * out_pad;
    mfma_layer<LDS_STRIDE>((const f32x4*)(a.params + lr[CL_W_OFF]), lr[CL_IN_PAD] >> 4, out_pad >> 4, X[cur], wave, lane, [&](int o, f32x4 sum) {
      const f32x4 bias = *(const f32x4*)(Bias + o);
      f32x4 y, slope;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = sum[r] + bias[r];
        y[r] = activate_once(x, act);
        slope[r] = live ? activate_slope(x, act) : 0.0f;
      }
      *(f32x4*)(S + o) = slope;   // act'(x) waits in dZ's place until the backward multiplies it by dA
      *(f32x4*)&Xout[col * LDS_STRIDE + o] = y;
      *(f32x4*)(Y + o) = live ? y : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    });
    __syncthreads();
    cur ^= 1;
  }

  // head stage: one lane per row -> the row's loss terms (R) and dL/dhead, the backward's first dA, in the other LDS buffer.  PAIR: the
  // row's lane reads the heads of its two columns and writes dA for both; R's terms go to the as-given column's scratch row, the lane of
  // the mirrored column zeroes that column's R row.  ML: the critic's lane reads its as-given column alone and hands the mirrored one zeros.
  // DUP: one lane per column, each a sample of its own -- a mirrored column's lane reads the action through act_perm / act_sign and the
  // row's own old_logp, adv, returns and old_value --, dA and R's terms go to the lane's own column and scratch row
  if (tid < TILE) {
    const int row = row0 + (SYM ? tid & (ROWS - 1) : tid);
    float* R = a.scratch + a.r_off + (size_t)(srow0 + tid) * PPO_ROW_COLS;
    const int head_pad = (a.layers + (size_t)(first + count - 1) * CTRL_LAYER_WORDS)[CL_OUT_PAD];
    if (PAIR && tid >= ROWS) {
      for (int j = 0; j < PPO_ROW_COLS; ++j)
        if ((j == PPO_COL_VLOSS) == (net == 1)) R[j] = 0.0f;
    } else {
      const int mcol = PAIR ? ROWS + tid : tid;   // PAIR: the row's mirrored column
      const bool twin = DUP && tid >= ROWS;       // DUP: this lane's sample is a mirror image
      const float *head = &X[cur][tid * LDS_STRIDE], *mirror = &X[cur][mcol * LDS_STRIDE];
      float *dA = &X[cur ^ 1][tid * LDS_STRIDE], *dAm = &X[cur ^ 1][mcol * LDS_STRIDE];
      const long long src = row < B ? (a.idx ? (long long)a.idx[row] : row) : 0;
      if constexpr (DISTIL) {   // include/mocca.h, mocca_distill_grad: one f32 operation per line of it, in that order; action is the target
        if (net == 1) {         // row, returns the value target or null
          float dv = 0.0f, vloss = 0.0f;
          if (row < B && a.returns) {
            const float e = head[0] - a.returns[src];
            const float l = e * e;
            vloss = 0.5f * l;
            dv = a.value_coef * e;
            dv = dv * a.inv_b;
          }
          R[PPO_COL_VLOSS] = vloss;
          for (int j = 0; j < head_pad; ++j) dA[j] = j == 0 ? dv : 0.0f;
        } else {
          const int A = a.act_dim;
          const float ia = 1.0f / (float)A;
          double m64 = 0.0;   // the row's sum of d_j^2, the terms f32
          for (int j = 0; j < head_pad || j < POL_MAX_ACTION; ++j) {
            float dmu = 0.0f;
            if (row < B && j < A) {
              const float d = head[j] - a.action[(size_t)src * A + j];
              const float q = d * d;
              m64 += (double)q;
              float u = d * a.inv_b;
              u = u * ia;
              dmu = u * a.mirror_k2;
            }
            if (j < head_pad) dA[j] = dmu;
            if (j < POL_MAX_ACTION) R[j] = 0.0f;   // log_std takes no gradient
          }
          R[PPO_COL_SURR] = 0.0f; R[PPO_COL_DLOGP] = 0.0f; R[PPO_COL_CLIPPED] = 0.0f;
          R[PPO_COL_MIRROR] = (float)m64 * ia;   // the row's distillation term (stats[7])
          for (int j = PPO_COL_MIRROR + 1; j < PPO_ROW_COLS; ++j) R[j] = 0.0f;
        }
      } else if (net == 1) {
        float dv = 0.0f, vloss = 0.0f;
        if (row < B) {   // include/mocca.h: one f32 operation per line of it, in that order
          const float v = NET ? 0.5f * (head[0] + mirror[0]) : head[0], ret = a.returns[src];
          const float e = v - ret;
          float l = e * e;
          dv = e;
          if (a.value_clip) {
            const float vo = a.old_value[src];
            const float dl = v - vo;
            const float dc = fminf(fmaxf(dl, -a.clip), a.clip);
            const float vc = vo + dc;
            const float e2 = vc - ret;
            const float l2 = e2 * e2;
            // where the clamp passes, vc is v and both terms are the same function of v: a tie, the unclipped term is used
            if ((dl < -a.clip || dl > a.clip) && l2 > l) {
              l = l2;
              dv = 0.0f;
            }
          }
          vloss = 0.5f * l;
          dv = a.value_coef * dv;
          dv = dv * a.inv_b;
          if (NET) dv = 0.5f * dv;   // dL/dv1 = dL/dv2
        }
        R[PPO_COL_VLOSS] = vloss;
        for (int j = 0; j < head_pad; ++j) {
          dA[j] = j == 0 ? dv : 0.0f;
          if (PAIR) dAm[j] = NET && j == 0 ? dv : 0.0f;
        }
      } else {
        const float* log_std = a.params + a.log_std_off;
        const int A = a.act_dim;
        // the Gaussian of action j: its mean (returned) and log_std.  NET: the symmetrised ones of mocca_policy.h, one f32 operation each
        auto gaussian = [&](int j, float* ls) {
          if (NET) {
            const int pj = a.act_perm[j];
            const float mm = mirror[pj] * a.act_sign[j];
            *ls = 0.5f * (log_std[j] + log_std[pj]);
            return 0.5f * (head[j] + mm);
          }
          *ls = log_std[j];
          return head[j];
        };
        // the sample's action j.  DUP, a mirrored column: (M_a a)[j], one f32 operation, exact
        auto action = [&](int j) {
          if (DUP && twin) return a.action[(size_t)src * A + a.act_perm[j]] * a.act_sign[j];
          return a.action[(size_t)src * A + j];
        };
        float g = 0.0f, surr = 0.0f, dlogp = 0.0f, clipped = 0.0f;
        if (row < B) {
          double lp64 = 0.0;   // the terms are f32, their sum is f64: 21 terms of size ~1 in f32 would leave ~1e-6 in the ratio
          for (int j = 0; j < A; ++j) {
            float ls;
            const float mu = gaussian(j, &ls);
            const float s = expf(ls);
            const float d = action(j) - mu;
            const float z = d / s;
            lp64 += (double)((-0.5f * z) * z - ls - 0.91893853320467274178f);
          }
          const float olp = a.old_logp[src], adv = a.adv[src];
          const float dl = (float)(lp64 - (double)olp);
          const float r = expf(dl);
          const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
          const float s1 = r * adv;
          const float rc = fminf(fmaxf(r, lo), hi);
          const float s2 = rc * adv;
          surr = fminf(s1, s2);
          dlogp = -dl;
          clipped = r > hi || r < lo ? 1.0f : 0.0f;
          const bool inactive = (adv > 0.0f && r > hi) || (adv < 0.0f && r < lo);
          if (!inactive) {
            g = adv * r;
            g = g * a.inv_b;
            g = -g;
          }
        }
        if (PAIR)   // every act_perm[j] below is written once more (a bijection of 0 .. A - 1); the padding stays 0
          for (int j = 0; j < head_pad; ++j) dAm[j] = 0.0f;
        const float ia = 1.0f / (float)A;
        double m64 = 0.0;   // ML: the row's sum of d_j^2, the terms f32
        for (int j = 0; j < head_pad || j < POL_MAX_ACTION; ++j) {
          float dmu = 0.0f, dls = 0.0f;
          if (row < B && j < A) {
            float ls;
            const float mu = gaussian(j, &ls);
            const float s = expf(ls);
            const float d = action(j) - mu;
            const float z = d / s;
            const float w = z / s;
            dmu = g * w;
            const float q = z * z - 1.0f;
            dls = g * q;
            if (NET) {   // dL/df1[j] = h, dL/df2[pj] = h * act_sign[j]
              dmu = 0.5f * dmu;
              dAm[a.act_perm[j]] = dmu * a.act_sign[j];
            }
            if (ML) {   // include/mocca.h: the mirror term's lines, one f32 operation each
              const int pj = a.act_perm[j];
              const float sg = a.act_sign[j];
              const float mm = mirror[pj] * sg;
              const float dm = head[j] - mm;
              const float qm = dm * dm;
              m64 += (double)qm;
              float u = dm * a.inv_b;
              u = u * ia;
              u = u * a.mirror_k2;
              dmu = dmu + u;
              const float um = u * sg;
              dAm[pj] = -um;
            }
          }
          if (j < head_pad) dA[j] = dmu;
          if (j < POL_MAX_ACTION) R[j] = dls;
        }
        R[PPO_COL_SURR] = surr; R[PPO_COL_DLOGP] = dlogp; R[PPO_COL_CLIPPED] = clipped;
        R[PPO_COL_MIRROR] = ML ? (float)m64 * ia : DUP && twin ? dlogp : 0.0f;   // DUP: old_logp - logp of the twins alone (stats[7])
        for (int j = PPO_COL_MIRROR + 1; j < PPO_ROW_COLS; ++j) R[j] = 0.0f;
      }
    }
  }
  __syncthreads();   // also orders this workgroup's stores of Y ahead of the loads below
  cur ^= 1;

  // backward, from the head down: X[cur] holds dA_l
#pragma unroll 1
  for (int li = count - 1; li >= 0; --li) {
    const int32_t* lr = a.layers + (size_t)(first + li) * CTRL_LAYER_WORDS;
    const int out_pad = lr[CL_OUT_PAD];
    float* dZ = a.scratch + a.dz_off[first + li] + (size_t)srow0 * out_pad;
    float* Xd = X[cur];
    for (int i = tid; i < TILE * out_pad; i += 256) {
      const int e = i / out_pad, o = i - e * out_pad;
      const float dz = Xd[e * LDS_STRIDE + o] * dZ[i];   // dZ holds act'(x) from the forward
      Xd[e * LDS_STRIDE + o] = dz;
      dZ[i] = dz;
    }
    if (li == 0) break;
    __syncthreads();
    float* Xout = X[cur ^ 1];
    mfma_layer<LDS_STRIDE>((const f32x4*)(a.params + a.wt_off[first + li]), out_pad >> 4, lr[CL_IN_PAD] >> 4, Xd, wave, lane,
               [&](int o, f32x4 sum) { *(f32x4*)&Xout[col * LDS_STRIDE + o] = sum; });
    __syncthreads();
    cur ^= 1;
  }
}

// launch 2 (header): blockIdx.x the tile -- per layer of the table its n_ot x n_kt weight tiles, then its n_ot bias tiles; after the layers
// the PPO_ROW_COLS / 16 column tiles of R --, blockIdx.y the row chunk; one wave
__global__ __launch_bounds__(64) void ppo_wgrad_kernel(PpoArgs a) {
  const int lane = threadIdx.x, col = lane & 15, quad = lane >> 4;
  const int chunk = blockIdx.y;
  const int r_begin = chunk * a.chunk_rows, r_end = min(r_begin + a.chunk_rows, a.b_pad);
  float* P = a.scratch + a.p_off + (size_t)chunk * a.p_floats;
  int t = blockIdx.x;
  const int n_layers = a.n_actor + a.n_critic;
  const float* M = nullptr;   // a column tile: 16 columns of M [b_pad][m_stride] from column m_col, summed to P[m_dst ..]
  int m_stride = 0, m_col = 0, m_dst = 0;
  bool found = false;
  for (int gl = 0; gl < n_layers && !found; ++gl) {
    const int32_t* lr = a.layers + (size_t)gl * CTRL_LAYER_WORDS;
    const int in_pad = lr[CL_IN_PAD], out_pad = lr[CL_OUT_PAD], n_kt = in_pad >> 4, n_ot = out_pad >> 4;
    const float* dZ = a.scratch + a.dz_off[gl];
    if (t < n_ot * n_kt) {
      const int ot = t / n_kt, kt = t - ot * n_kt;
      const bool first = gl == 0 || gl == a.n_actor;
      const float* Ap = a.scratch + (first ? (gl == 0 ? a.a0_off : a.a0c_off) : a.a_off[gl - 1]);   // the layer's input [b_pad][in_pad]; a0c_off: A0, PPO_PRIV: A0c
      const float* pz = dZ + (size_t)(r_begin + quad) * out_pad + 16 * ot + col;
      const float* pa = Ap + (size_t)(r_begin + quad) * in_pad + 16 * kt + col;
      f32x4 acc[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int r = r_begin; r < r_end; r += 16) {
        float z[NP], x[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) { z[j] = pz[(size_t)(4 * j) * out_pad]; x[j] = pa[(size_t)(4 * j) * in_pad]; }
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(z[j], x[j], acc[j], 0, 0, 0);
        pz += (size_t)16 * out_pad; pa += (size_t)16 * in_pad;
      }
      const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
      float* dst = P + lr[CL_W_OFF] + (size_t)(16 * ot + 4 * quad) * in_pad + 16 * kt + col;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dst[(size_t)rr * in_pad] = sum[rr];
      return;
    }
    t -= n_ot * n_kt;
    if (t < n_ot) { M = dZ; m_stride = out_pad; m_col = 16 * t; m_dst = lr[CL_B_OFF] + 16 * t; found = true; }
    else t -= n_ot;
  }
  if (!found) {
    if (t >= PPO_ROW_COLS / 16) return;
    M = a.scratch + a.r_off; m_stride = PPO_ROW_COLS; m_col = 16 * t; m_dst = a.log_std_off + 16 * t;
  }
  double s = 0.0;
  const float* p = M + (size_t)(r_begin + quad) * m_stride + m_col + col;
  for (int r = r_begin; r < r_end; r += 4) { s += (double)*p; p += (size_t)4 * m_stride; }
  s += __shfl_xor(s, 16);   // (q0 + q1), (q2 + q3)
  s += __shfl_xor(s, 32);   // (q0 + q1) + (q2 + q3): the same bits in all four quads
  if (quad == 0) P[m_dst + col] = (float)s;
}

// launch 3 (header): thread i forms grad[i]
__global__ __launch_bounds__(PPO_REDUCE_BLOCK) void ppo_reduce_kernel(PpoArgs a) {
  __shared__ double sq[PPO_REDUCE_BLOCK];
  const int tid = threadIdx.x, i = blockIdx.x * PPO_REDUCE_BLOCK + tid;
  double g2 = 0.0;
  if (i < a.n_head) {
    const int n_layers = a.n_actor + a.n_critic;
    int pos = 0, src = -1;
    for (int gl = 0; gl < n_layers; ++gl) {
      const int32_t* lr = a.layers + (size_t)gl * CTRL_LAYER_WORDS;
      const int in = lr[CL_IN], out = lr[CL_OUT], n_w = in * out;
      if (i < pos + n_w) { const int o = (i - pos) / in, k = (i - pos) - o * in; src = lr[CL_W_OFF] + o * lr[CL_IN_PAD] + k; break; }
      if (i < pos + n_w + out) { src = lr[CL_B_OFF] + (i - pos - n_w); break; }
      pos += n_w + out;
    }
    const bool is_log_std = src < 0;
    if (is_log_std) src = a.log_std_off + (i - pos);
    const float* P = a.scratch + a.p_off + src;
    float g = P[0];
    for (int c = 1; c < a.n_chunks; ++c) g += P[(size_t)c * a.p_floats];
    if (is_log_std && a.mode == PPO_SYM) {   // the symmetrised log_std: 0.5f * (T[j] + T[act_perm[j]])
      const float* Pm = a.scratch + a.p_off + a.log_std_off + a.act_perm[i - pos];
      float gm = Pm[0];
      for (int c = 1; c < a.n_chunks; ++c) gm += Pm[(size_t)c * a.p_floats];
      g = 0.5f * (g + gm);
    }
    if (is_log_std) g = g - a.entropy_coef;   // dH / dlog_std_j = 1 (act_perm is a bijection)
    a.grad[i] = g;
    g2 = (double)g * (double)g;
  }
  sq[tid] = g2;
  __syncthreads();
  for (int s = PPO_REDUCE_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) sq[tid] += sq[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.sq_part[blockIdx.x] = sq[0];
}

// launch 4 (header): one workgroup
__global__ __launch_bounds__(PPO_REDUCE_BLOCK) void ppo_stats_kernel(PpoArgs a) {
  __shared__ double sq[PPO_REDUCE_BLOCK];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int b = tid; b < a.n_reduce_blocks; b += PPO_REDUCE_BLOCK) s += a.sq_part[b];
  sq[tid] = s;
  __syncthreads();
  for (int h = PPO_REDUCE_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) sq[tid] += sq[tid + h];
    __syncthreads();
  }
  if (tid != 0 || !a.stats) return;
  float sum[5];   // the columns 32 .. 35 of R over all rows, and 36 for the mirror loss and the duplicated rows: the chunks' sums in chunk order
  sum[4] = 0.0f;
  for (int k = 0; k < (a.mode >= PPO_MIRROR ? 5 : 4); ++k) {
    const float* P = a.scratch + a.p_off + a.log_std_off + PPO_COL_SURR + k;
    float v = P[0];
    for (int c = 1; c < a.n_chunks; ++c) v += P[(size_t)c * a.p_floats];
    sum[k] = v;
  }
  const float* log_std = a.params + a.log_std_off;
  double h = 0.0;   // the entropy: summed in f64, j ascending, rounded once; PPO_SYM: of the symmetrised log_std (f32, as the head stage forms it)
  for (int j = 0; j < a.act_dim; ++j) {
    const float ls = a.mode == PPO_SYM ? 0.5f * (log_std[j] + log_std[a.act_perm[j]]) : log_std[j];
    h += ((double)ls + 0.5) + 0.91893853320467274178;
  }
  a.stats[0] = sum[0] * a.inv_b;
  a.stats[1] = sum[1] * a.inv_b;
  a.stats[2] = (float)h;
  a.stats[3] = sum[2] * a.inv_b;
  a.stats[4] = sum[3] / (float)a.n_samples;   // a count over B (PPO_DUP: 2 B), correctly rounded
  a.stats[5] = (float)sq[0];
  a.stats[6] = 0.0f;
  a.stats[7] = sum[4] * a.inv_b;   // PPO_MIRROR: L_m, the rows' terms already carry the 1 / A; PPO_DUP: the twins' share of stats[3]; PPO_DISTIL: L_d; else 0
}

void launch_ppo(hipStream_t s, const PpoArgs& a) {
  if (a.mode == PPO_SYM) hipLaunchKernelGGL(ppo_rows_kernel<PPO_SYM>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  else if (a.mode == PPO_MIRROR) hipLaunchKernelGGL(ppo_rows_kernel<PPO_MIRROR>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  else if (a.mode == PPO_DUP) hipLaunchKernelGGL(ppo_rows_kernel<PPO_DUP>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  else if (a.mode == PPO_DISTIL) hipLaunchKernelGGL(ppo_rows_kernel<PPO_DISTIL>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  else if (a.mode == PPO_PRIV) hipLaunchKernelGGL(ppo_rows_kernel<PPO_PRIV>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(ppo_rows_kernel<PPO_PLAIN>, dim3(a.b_pad / TILE, 2), dim3(256), 0, s, a);
  hipLaunchKernelGGL(ppo_wgrad_kernel, dim3(a.n_tiles, a.n_chunks), dim3(64), 0, s, a);
  hipLaunchKernelGGL(ppo_reduce_kernel, dim3(a.n_reduce_blocks), dim3(PPO_REDUCE_BLOCK), 0, s, a);
  hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(PPO_REDUCE_BLOCK), 0, s, a);
}

}  // namespace mocca_ppo
