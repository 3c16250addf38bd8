"""Checker for the device policy (mocca_envs_amd/csrc/mocca_policy.hip): an independent numpy float64 forward (normalisation, nets, sample,
log-probability, value), a numpy restatement of the in-kernel noise (Philox keying and Box-Muller of csrc/mocca_policy.h), a seeded factory
of random policies, and mutations -- policies that differ from the right one the way a kernel bug would.

A policy here is a SimpleNamespace(actor, critic, log_std, obs_mean, inv_std, clip): layer lists [(W[out][in], b[out], activation)] as in
controller_reference, float32 arrays; obs_mean / inv_std None = no normalisation."""
from types import SimpleNamespace

import numpy as np

from controller_reference import act64, error_units, net64, triple  # noqa: F401  (re-exported for the tests)
from ppo_reference import normalise64  # noqa: F401

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
NOISE_SEED = 2024            # the seed of the noise-moment tests, CPU and GPU (test_policy.py checks that the reference holds both bounds at it)
SHAPES = {
    "ppo": (([256, 256], ["tanh", "tanh", "identity"]), ([256, 256], ["tanh", "tanh", "identity"])),
    "small": (([16], ["tanh", "identity"]), ([16], ["softsign", "identity"])),
    # 8 layers of mixed widths and activations: controller_reference.SHAPES["deep8"]
    "deep8": (([32, 64, 16, 128, 48, 256, 80], ["relu", "tanh", "softsign", "identity", "relu", "softsign", "tanh", "tanh"]),
              ([16, 256, 32, 32, 112, 64, 16], ["softsign", "relu", "relu", "tanh", "identity", "relu", "softsign", "identity"])),
}
DIMS = ((36, 10), (52, 21), (65, 21), (142, 21))     # (in_dim, act_dim); the last is run with in_stride > in_dim


def random_policy(kind="ppo", in_dim=52, act_dim=21, norm=True, seed=0):
    """Weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2), log_std ~ U(-1.5, 0); observation statistics: mean ~ N(0, 1), var ~ U(0.05, 4) --
    with raw inputs ~ N(0, 3^2) (plausible_inputs) a few percent of the normalised values reach the clip at 5."""
    rng = np.random.default_rng([seed, sorted(SHAPES).index(kind), in_dim, act_dim])

    def net(hidden, acts, out):
        dims, layers = [in_dim] + list(hidden) + [out], []
        for i, act in enumerate(acts):
            layers.append((rng.normal(0, 1 / np.sqrt(dims[i]), (dims[i + 1], dims[i])).astype(np.float32),
                           rng.normal(0, 0.1, dims[i + 1]).astype(np.float32), act))
        return layers

    (ah, aa), (ch, ca) = SHAPES[kind]
    p = SimpleNamespace(actor=net(ah, aa, act_dim), critic=net(ch, ca, 1), log_std=rng.uniform(-1.5, 0.0, act_dim).astype(np.float32),
                        obs_mean=None, inv_std=None, clip=5.0)
    mean, var = rng.normal(0, 1, in_dim).astype(np.float32), rng.uniform(0.05, 4.0, in_dim).astype(np.float32)
    if norm:
        p.obs_mean, p.inv_std = mean, (np.float32(1) / np.sqrt(var + np.float32(1e-8))).astype(np.float32)
    return p


def plausible_inputs(n, in_dim, seed=0):
    return np.random.default_rng([seed, 77]).normal(0, 3.0, (n, in_dim)).astype(np.float32)


def forward64(p, x):
    """-> (mean [B, A], value [B]) in float64"""
    z = normalise64(p, x)
    return net64(p.actor, z), net64(p.critic, z)[..., 0]


def sample64(mean, log_std, eps):
    """-> (action, logp) in float64 from a given mean: action = mean + exp(log_std) eps, logp = sum_j (-eps^2 / 2 - log_std - log(2 pi) / 2)"""
    mean, ls, eps = np.asarray(mean, np.float64), np.asarray(log_std, np.float64), np.asarray(eps, np.float64)
    return mean + np.exp(ls) * eps, (-0.5 * eps * eps - ls - HALF_LOG_2PI).sum(-1)


def sample32(mean, log_std, eps):
    """the same in float32, term by term in ascending j: the yardstick of the sample's rounding error"""
    mean, ls, eps = np.asarray(mean, np.float32), np.asarray(log_std, np.float32), np.asarray(eps, np.float32)
    lp = np.zeros(mean.shape[:-1], np.float32)
    for j in range(mean.shape[-1]):
        lp = lp + (np.float32(-0.5) * eps[..., j] * eps[..., j] - ls[j] - np.float32(HALF_LOG_2PI))
    return mean + np.exp(ls) * eps, lp


def torch32(p, x):
    """-> (mean, value): torch CPU float32 on the same inputs -- the yardstick of the nets' rounding error"""
    import torch
    x = torch.from_numpy(np.asarray(x, np.float32))
    if p.obs_mean is not None:
        x = ((x - torch.from_numpy(p.obs_mean)) * torch.from_numpy(p.inv_std)).clamp(-p.clip, p.clip)

    def net(layers, h):
        for w, b, act in layers:
            h = torch.nn.functional.linear(h, torch.from_numpy(w), torch.from_numpy(b))
            h = {"relu": torch.relu, "tanh": torch.tanh, "softsign": torch.nn.functional.softsign, "identity": lambda v: v}[act](h)
        return h

    return net(p.actor, x).numpy(), net(p.critic, x)[..., 0].numpy()


# ---- the in-kernel noise ----
def philox4x32(c, key):
    """Philox4x32-10: counters uint32 [..., 4], key (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(c[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, -1).astype(np.uint32)


def noise(seed, env_ids, t, episode, act_dim, dtype=np.float64):
    """eps [len(env_ids), act_dim] of csrc/mocca_policy.h: block p of env e has the counter (16 e + p, t[e], episode[e], 1) under the key
    (seed low, seed high); words 0, 1 -> u1 = ((w0 >> 8) + 1) / 2^24, u2 = (w1 >> 8) / 2^24; r = sqrt(-2 log u1); eps[2 p] = r cos(2 pi u2),
    eps[2 p + 1] = r sin(2 pi u2).  dtype float64: exact uniforms, float64 functions; float32: every operation in float32, as the kernel."""
    env_ids = np.asarray(env_ids, np.uint64)
    n, blocks = env_ids.size, (act_dim + 1) // 2
    c = np.zeros((n, blocks, 4), np.uint64)
    c[..., 0] = (np.uint64(16) * env_ids[:, None] + np.arange(blocks, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
    c[..., 1] = (np.asarray(t, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))[:, None]
    c[..., 2] = (np.asarray(episode, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))[:, None]
    c[..., 3] = 1
    w = philox4x32(c, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    f = dtype
    u1 = ((w[..., 0] >> 8) + 1).astype(f) * f(1.0 / 16777216.0)
    u2 = (w[..., 1] >> 8).astype(f) * f(1.0 / 16777216.0)
    r = np.sqrt(f(-2.0) * np.log(u1))
    th = (f(6.28318530717958647692) * u2).astype(f)
    z = np.stack([r * np.cos(th), r * np.sin(th)], -1).astype(f).reshape(n, 2 * blocks)
    return z[:, :act_dim]


# ---- mutations ----
MUTATIONS = ("no_norm", "no_clip", "activation", "log_std_sign", "logp_no_log_std")


def mutated(p, how):
    """A policy / sampler that is wrong the way a kernel bug would be.  The first three change mean and value (forward64), the last two the
    sample (sample64_mutated)."""
    q = SimpleNamespace(**vars(p))
    if how == "no_norm":
        q.obs_mean = q.inv_std = None
    elif how == "no_clip":
        q.clip = np.inf
    elif how == "activation":
        swap = {"relu": "softsign", "softsign": "relu", "tanh": "softsign"}
        q.actor = [(w, b, swap.get(a, a)) for w, b, a in p.actor]
        q.critic = [(w, b, swap.get(a, a)) for w, b, a in p.critic]
    elif how not in MUTATIONS:
        raise ValueError(how)
    return q


def sample64_mutated(mean, log_std, eps, how):
    ls = np.asarray(log_std, np.float64)
    if how == "log_std_sign":
        return sample64(mean, -ls, eps)
    if how == "logp_no_log_std":
        a, lp = sample64(mean, ls, eps)
        return a, lp + ls.sum()
    raise ValueError(how)
