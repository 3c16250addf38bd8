"""Checker for mocca_adam_step / mocca_ppo_update (include/mocca.h; mocca_envs_amd/csrc/mocca_optim.hip): the epoch's permutation in numpy
integers, launch A (the gradient's norm, the clip coefficient, the clock) in float64 and launch B (Adam's step) in float32, operation by
operation and sum by sum in the kernels' order.  A device run must give these bits.

`how` names a deliberate mistake (MUTATIONS); the tests show that their comparisons reject each."""
import numpy as np

MUTATIONS = ("no_bias_correction",     # ss = lr and bc = 1: Adam without its bias correction
             "coef_after_moments",     # the moments see the raw gradient; the clip scales only the step's m
             "five_rounds")            # the Feistel network with five rounds
BLOCK = 256
FRESH_CLOCK = (0.0, 1.0, 1.0, 0.0)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, np.uint64)


def philox4x32_first(c0, c1, c2, c3, k0, k1):
    """word 0 of Philox4x32-10 (mocca_philox.h); counters and keys: uint32 values, arrays that broadcast"""
    c0, c1, c2, c3, k0, k1 = (_u64(c) & _U32 for c in (c0, c1, c2, c3, k0, k1))
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _U32, (p0 >> s32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0


def feistel_half(n):
    w = max(2, int(n - 1).bit_length())
    return (w + 1) // 2


def feistel_pass(x, half, t, seed, rounds=6):
    """one pass of the network over the uint64 array x: a bijection of 0 .. 4^half - 1; t and seed: uint64 values that broadcast with x"""
    half64, mask, s32 = np.uint64(half), np.uint64((1 << half) - 1), np.uint64(32)
    t, seed = _u64(t), _u64(seed)
    left, right = x >> half64, x & mask
    for r in range(rounds):
        f = philox4x32_first(right, np.uint64(r), t & _U32, t >> s32, seed & _U32, seed >> s32)
        left, right = right, left ^ (f & mask)
    return (left << half64) | right


def permutation(n, t, seed, how=None):
    """int64 [n]: entry b starts at x = b and takes passes until x < n.  t and seed: integers, or arrays [k, 1] for k permutations [k, n]"""
    half, rounds = feistel_half(n), 5 if how == "five_rounds" else 6
    t, seed = _u64(t), _u64(seed)
    x = np.broadcast_to(np.arange(n, dtype=np.uint64), np.broadcast(t, seed, np.empty(n)).shape)
    t, seed = np.broadcast_to(t, x.shape), np.broadcast_to(seed, x.shape)
    x = feistel_pass(x, half, t, seed, rounds)
    while True:
        out = x >= np.uint64(n)
        if not out.any():
            return x.astype(np.int64)
        x[out] = feistel_pass(x[out], half, t[out], seed[out], rounds)


def sum_of_squares(g):
    """launch A's S: thread tid adds f64(g[i])^2 for i = tid, tid + 256, .. ascending, then the tree sq[tid] += sq[tid + h], h = 128 .. 1"""
    g = np.asarray(g, np.float32).astype(np.float64)
    pad = np.zeros((g.size + BLOCK - 1) // BLOCK * BLOCK)
    pad[:g.size] = g * g
    sq = np.zeros(BLOCK)
    with np.errstate(invalid="ignore", over="ignore"):
        for row in pad.reshape(-1, BLOCK):      # a padded entry adds +0.0: it changes no bit
            sq = sq + row
        h = BLOCK // 2
        while h:
            sq[:h] = sq[:h] + sq[h:2 * h]
            h //= 2
    return sq[0]


def clip_coef(grad, max_grad_norm=0.5):
    """launch A's clip coefficient for the float32 gradient `grad` (all of it): float32; 0.0 where the step is skipped"""
    S = sum_of_squares(grad)
    if not np.isfinite(S):
        return np.float32(0.0)
    return np.float32(min(1.0, max_grad_norm / (np.sqrt(np.float64(S)) + 1e-6))) if max_grad_norm > 0 else np.float32(1.0)


def adam_step(params, grad, m, v, clock, n_params=None, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, how=None):
    """one mocca_adam_step on float32 arrays params / m / v [>= n_params] and a float64 clock [4] -> (params, m, v, clock, coef), all new;
    coef is the clip coefficient applied, 0.0 on a skipped step"""
    f32 = np.float32
    p, m, v, clock = (np.array(x, dtype=d) for x, d in ((params, f32), (m, f32), (v, f32), (clock, np.float64)))
    n = p.size if n_params is None else int(n_params)
    g = np.asarray(grad, f32)[:n]
    if not np.isfinite(sum_of_squares(g)):
        clock[3] += 1.0
        return p, m, v, clock, f32(0.0)
    coef = clip_coef(g, max_grad_norm)
    clock[0] += 1.0
    clock[1] = clock[1] * beta1
    clock[2] = clock[2] * beta2
    ss, bc = f32(lr / (1.0 - clock[1])), f32(np.sqrt(1.0 - clock[2]))
    if how == "no_bias_correction":
        ss, bc = f32(lr), f32(1.0)
    b2, w1, w2, e = f32(beta2), f32(1.0 - beta1), f32(1.0 - beta2), f32(eps)
    mm, vv, pp = m[:n], v[:n], p[:n]
    gc = g * coef
    gm = g if how == "coef_after_moments" else gc
    d = gm - mm
    d = d * w1
    mm = mm + d
    vv = vv * b2
    q = gm * gm
    q = q * w2
    vv = vv + q
    s = np.sqrt(vv)
    s = s / bc
    s = s + e
    u = (mm * coef if how == "coef_after_moments" else mm) / s
    u = ss * u
    pp = pp - u
    m[:n], v[:n], p[:n] = mm, vv, pp
    assert mm.dtype == f32 and vv.dtype == f32 and pp.dtype == f32
    return p, m, v, clock, coef


def gradients(n, seed, hi=10.0):
    """float32 [n]: |g| log-uniform in 1e-8 .. hi (<= 10), random signs, one entry in sixteen exactly 0: g * g stays a normal float"""
    rng = np.random.default_rng(seed)
    g = np.exp(rng.uniform(np.log(1e-8), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 1 / 16] = 0.0
    return g.astype(np.float32)
