// mocca_optim.h -- what follows the gradient in a PPO update, as kernels (mocca_optim.hip): clip_grad_norm_ and Adam's step on the flat parameter
// tensor of mocca_update_policy, and the epoch's shuffle.  mocca_adam_step / mocca_ppo_update (mocca_api_trainer.hip) check the caller's arguments, own
// the scratch and launch them between mocca_ppo.h's four launches and the repack of mocca_policy.h.  The contract: include/mocca.h.
// mocca_distill_update is the same loop (mocca_api_trainer.hip: update_loop) around mocca_distill_grad: same kernels, same scratch, same shuffle.
//
// Layout.  params [n_floats] f32 is mocca_update_policy's flat tensor; its first n_params floats are trainable.  grad [>= n_params] f32 in the
// same order.  moments f32 [2][n_head]: m at 0, v at n_head (n_head: the tensor's length without mean / inv_std), caller-owned.  clock f64 [4]:
// {t, beta1^t, beta2^t, skipped steps}, caller-owned, fresh {0, 1, 1, 0}.  Scratch (f64 words, owned by the handle, one buffer):
//   rec     [4]                     AdamRecord: what launch A hands launch B
//   G       [ceil(n_head / 2)]      mocca_ppo_update's gradient, f32 [n_head]
//   perm    [R]                     mocca_ppo_update's permutation of the epoch, i64
//
// Launch A (adam_norm_kernel): ONE workgroup of 256.  S = sum f64(g[i])^2 over i < n_params: thread tid adds i = tid, tid + 256, .. ascending,
// then ppo_stats_kernel's tree (sq[tid] += sq[tid + h], h = 128 .. 1).  Thread 0, in f64: nrm = sqrt(S); coef = max_grad_norm > 0 ?
// min(1, max_grad_norm / (nrm + 1e-6)) : 1, rounded once to f32.  S not finite: rec.skip = 1, clock[3] += 1, nothing else changes.  Otherwise
// t += 1, p1 = p1 * beta1, p2 = p2 * beta2 (running products: no pow), and rec = {coef, ss = f32(lr / (1 - p1)), bc = f32(sqrt(1 - p2)),
// b2 = f32(beta2), w1 = f32(1 - beta1), w2 = f32(1 - beta2), e = f32(eps), skip = 0}.  stats (a row of mocca_ppo_grad's statistics or null):
// stats[6] = coef, 0 on a skipped step.  The stream orders A before B: no atomics, no race on the clock.
// Launch B (adam_apply_kernel): one thread per trainable float; returns at once on rec.skip.  Each line ONE IEEE f32 operation, never contracted,
// square root and division correctly rounded:
//     g = grad[i] * coef
//     d = g - m;  d = d * w1;  m = m + d
//     v = v * b2;  q = g * g;  q = q * w2;  v = v + q
//     s = sqrtf(v);  s = s / bc;  s = s + e
//     u = m / s;  u = ss * u;  p = p - u
// Launch C is mocca_policy.h's repack of params, as mocca_update_policy runs it.
// lr, the betas, eps and max_grad_norm are kernel arguments: a captured call has them baked in; the clock is on the device and advances on replay.
//
// Shuffle (shuffle_kernel): one thread per entry b < R of perm, closed form, integers only.  w = max(2, bit_length(R - 1)) rounded up to even,
// half = w / 2, mask = 2^half - 1.  One pass maps x = (L << half) | Rr through six Feistel rounds (L, Rr) <- (Rr, L ^ (F & mask)),
// F = philox4x32(c0 = Rr, c1 = round, c2 = t mod 2^32, c3 = t >> 32, k0 = seed mod 2^32, k1 = seed >> 32)[0]; entry b starts at x = b and takes
// passes until x < R (cycle walking: the pass is a bijection of 0 .. 2^w - 1, so the walk returns below R and the result is a bijection of
// 0 .. R - 1).  t is clock[0] as the kernel reads it: a replayed graph shuffles anew, a fresh clock with the same seed repeats a run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocca_optim {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_REC_WORDS = 4;         // f64 words of the scratch ahead of G
constexpr int FEISTEL_ROUNDS = 6;

struct AdamRecord {
  float coef, ss, bc, b2, w1, w2, e;
  int skip;
};
static_assert(sizeof(AdamRecord) <= OPT_REC_WORDS * sizeof(double), "the record has OPT_REC_WORDS f64 words of the scratch");

struct AdamArgs {
  float* params;
  const float* grad;
  int n_params;
  float *m, *v;                          // [n_head] each; the first n_params are touched
  double* clock;                         // [4]
  AdamRecord* rec;
  double lr, beta1, beta2, eps, max_grad_norm;
  float* stats;                          // [8] or null: launch A writes [6]
};

struct ShuffleArgs {
  int64_t* perm;                         // [n]
  int n;                                 // R
  int half;
  uint32_t mask, seed_lo, seed_hi;
  const double* clock;
};

// half of the Feistel word for n entries (header: Shuffle)
inline int shuffle_half(long long n) {
  int w = 0;
  for (long long x = n - 1; x > 0; x >>= 1) ++w;
  if (w < 2) w = 2;
  return (w + 1) / 2;
}

void launch_adam(hipStream_t s, const AdamArgs& a);        // launches A and B
void launch_shuffle(hipStream_t s, const ShuffleArgs& a);

}  // namespace mocca_optim
