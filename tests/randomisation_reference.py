"""Numpy restatement of the domain randomisation (mocca_envs_amd/csrc/mocca_randomise.h, include/mocca.h mocca_set_randomisation): the
keying, the episode parameters, the strength / latency ring, the pushes, the sensor noise and the record, BIT FOR BIT.

Every draw is Philox4x32-10 (policy_reference.philox4x32) under the key (seed low, seed high) with the counter (g, c1, E, domain + 256 b).
Every fmaf is evaluated exactly -- the product and the sum in float64 with round-to-odd where the sum is inexact -- and rounded ONCE to
float32; every other operation is a single float32 operation.

`mutate=` switches ONE rule to a plausible wrong reading; the CPU test shows that the comparison against the header rejects each of them.
"""
import numpy as np

from policy_reference import philox4x32

RAND_WORDS, MAX_DELAY, MAX_INTERVAL = 4, 7, 65536
DOMAIN_PLANT, DOMAIN_NOISE, BLOCK = 4, 5, 256
MUTATIONS = ("domain", "ring_off_by_one", "push_at_zero", "planar_dvy", "noise_block")


class Config:
    def __init__(self, strength=(1.0, 1.0), latency=(0, 0), push=(0, 0.0), planar=False):
        self.lo, self.hi = np.float32(strength[0]), np.float32(strength[1])
        self.dmin, self.dmax = int(latency[0]), int(latency[1])
        self.interval, self.push_max = int(push[0]), np.float32(push[1])
        self.planar = bool(planar)


def _key(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def _words(seed, g, c1, episode, c3):
    """Philox words [len(g), 4] of the counters (g, c1, episode, c3); every argument an integer or an array over the envs"""
    g = np.asarray(g, np.int64)
    c = np.zeros((g.size, 4), np.uint64)
    for i, v in enumerate((g, c1, episode, c3)):
        c[:, i] = (np.broadcast_to(np.asarray(v, np.int64), g.shape).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return philox4x32(c, _key(seed))


def uniform(w):
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def signed(w):
    return np.float32(2.0) * uniform(w) - np.float32(1.0)       # exact


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays: the product of two float32 is exact in float64; the sum is rounded to odd where it is inexact
    (TwoSum finds the error), so that the one rounding to float32 that follows is the correctly rounded result"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    inexact = (err != 0.0) & np.isfinite(s)
    even = (s.view(np.int64) & 1) == 0
    s = np.where(inexact & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def episode_params(seed, g, episode, cfg, mutate=None):
    """-> strength f32 [n], delay i64 [n], phase i64 [n]"""
    w = _words(seed, g, 0, episode, (DOMAIN_PLANT + 1 if mutate == "domain" else DOMAIN_PLANT))
    strength = fma32(uniform(w[:, 0]), cfg.hi - cfg.lo, np.broadcast_to(cfg.lo, w[:, 0].shape))
    delay = cfg.dmin + (w[:, 1] >> np.uint32(8)).astype(np.int64) % (cfg.dmax - cfg.dmin + 1)
    phase = (w[:, 2] >> np.uint32(8)).astype(np.int64) % cfg.interval if cfg.interval > 0 else np.zeros(w.shape[0], np.int64)
    return strength, delay, phase


def clip(a):
    a = np.asarray(a, np.float32)
    return np.where(a < -1, np.float32(-1), np.where(a > 1, np.float32(1), a)).astype(np.float32)      # a NaN passes through


def push(seed, g, t, episode, cfg, phase, mutate=None):
    """-> fires bool [n], dv f32 [n, 2] (zeros where no push fires)"""
    t = np.broadcast_to(np.asarray(t, np.int64), np.asarray(g).shape)
    if cfg.interval <= 0:
        return np.zeros(t.shape, bool), np.zeros(t.shape + (2,), np.float32)
    fires = ((t > 0) | (mutate == "push_at_zero")) & ((t + phase) % cfg.interval == 0)
    w = _words(seed, g, t, episode, DOMAIN_PLANT + BLOCK)
    dv = np.stack([cfg.push_max * signed(w[:, 0]), cfg.push_max * signed(w[:, 1])], -1).astype(np.float32)
    if cfg.planar and mutate != "planar_dvy":
        dv[:, 1] = 0.0
    dv[~fires] = 0.0
    return fires, dv


def until_push(t, phase, cfg):
    t = np.asarray(t, np.int64)
    if cfg.interval <= 0:
        return np.full(t.shape, -1, np.int64)
    t0 = np.maximum(t, 1)
    r = (t0 + phase) % cfg.interval
    return t0 - t + np.where(r != 0, cfg.interval - r, 0)


def record(seed, g, t, episode, cfg):
    """[n, 4] f32: strength, delay, steps until the next push (or -1), 0"""
    strength, delay, phase = episode_params(seed, g, episode, cfg)
    t = np.broadcast_to(np.asarray(t, np.int64), strength.shape)
    return np.stack([strength, delay.astype(np.float32), until_push(t, phase, cfg).astype(np.float32), np.zeros_like(strength)], -1)


def noise(seed, g, t, episode, rows, scale, mutate=None):
    """rows [n, >= dim] -> the noisy [n, dim], dim = len(scale)"""
    scale = np.asarray(scale, np.float32)
    g = np.asarray(g, np.int64)
    dim = scale.size
    out = np.empty((g.size, dim), np.float32)
    for b in range((dim + 3) // 4):
        for k in range(4 * b, min(dim, 4 * b + 4)):
            blk = (k % 4) if mutate == "noise_block" else b
            w = _words(seed, g, t, episode, DOMAIN_NOISE + BLOCK * blk)
            out[:, k] = fma32(np.broadcast_to(scale[k], (g.size,)), signed(w[:, k % 4]), rows[:, k])
    return out


class Plant:
    """The perturb kernel's state across steps: the ring [n, delay_max + 1, act_dim], never cleared"""

    def __init__(self, seed, g, cfg, act_dim, mutate=None):
        self.seed, self.g, self.cfg, self.mutate = seed, np.asarray(g, np.int64), cfg, mutate
        self.ring = np.zeros((self.g.size, cfg.dmax + 1, act_dim), np.float32)

    def step(self, actions, t, episode):
        """actions [n, act_dim], the envs' counters t and episode AT LAUNCH -> (effective action [n, act_dim], fires [n], dv [n, 2])"""
        cfg, n = self.cfg, self.g.size
        t = np.broadcast_to(np.asarray(t, np.int64), (n,))
        strength, delay, phase = episode_params(self.seed, self.g, episode, cfg, self.mutate)
        v = (strength[:, None] * clip(actions)).astype(np.float32)
        idx = np.arange(n)
        self.ring[idx, t % (cfg.dmax + 1)] = v
        src = t - delay - (1 if self.mutate == "ring_off_by_one" else 0)
        eff = self.ring[idx, src % (cfg.dmax + 1)].copy()
        eff[t < delay] = 0.0
        fires, dv = push(self.seed, self.g, t, episode, cfg, phase, self.mutate)
        return eff, fires, dv
