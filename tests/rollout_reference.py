"""Numpy restatements of what mocca_gae / mocca_obs_stats compute (include/mocca.h), shared by test_rollout.py and test_gpu_rollout.py.

`gae_f32` is the kernel's contract operation by operation in float32; `gae_f64` the same recurrence in float64 (for the closed forms);
`moments_f64` / `obs_stats_f64` are the plain two-pass float64 definitions, NOT the kernel's shifted sums: an independent route to the
same numbers.  `torch_gae_loop` is the loop of tools/ppo_demo.py, restated on whatever device its tensors live on."""
import numpy as np

U64 = 2.0 ** -53      # unit roundoff of float64


def _gae(rew, value, masks, bad_masks, g, c, s, dt):
    rew, value, masks, bad_masks = (np.asarray(x, dt).reshape(x.shape[0], -1) for x in (rew, value, masks, bad_masks))
    T, N = rew.shape
    adv, ret = np.zeros((T, N), dt), np.zeros((T, N), dt)
    gae = np.zeros(N, dt)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            delta = ((rew[t] * s) + ((g * value[t + 1]) * masks[t + 1])) - value[t]
            gae = (delta + ((c * masks[t + 1]) * gae)) * bad_masks[t + 1]
            adv[t] = gae
            ret[t] = gae + value[t]
    return adv, ret


def gae_f32(rew, value, masks, bad_masks, gamma, lam, reward_scale=1.0):
    """-> (adv, ret) float32 [T, N]: every operation one float32 operation, in the contract's order"""
    return _gae(rew, value, masks, bad_masks, np.float32(gamma), np.float32(float(gamma) * float(lam)), np.float32(reward_scale), np.float32)


def gae_f64(rew, value, masks, bad_masks, gamma, lam, reward_scale=1.0):
    return _gae(rew, value, masks, bad_masks, np.float64(gamma), np.float64(float(gamma) * float(lam)), np.float64(reward_scale), np.float64)


def moments_f64(adv):
    """(mean, std with Bessel's correction) of all entries, two passes in float64"""
    a = np.asarray(adv, np.float64).reshape(-1)
    mean = a.sum() / a.size
    return mean, np.sqrt(((a - mean) ** 2).sum() / (a.size - 1))


def normalise_f32(adv, moments, adv_eps):
    """the kernel's float32 formula from given float32 moments"""
    m = np.asarray(moments, np.float32)
    return (np.asarray(adv, np.float32) - m[0]) / (m[1] + np.float32(adv_eps))


def obs_stats_f64(state, rows, dim):
    """Chan's merge of [count, mean[dim], var[dim]] with the UNSHIFTED two-pass batch moments of rows[:, :dim], float64"""
    state = np.asarray(state, np.float64)
    x = np.asarray(rows).reshape(-1, np.shape(rows)[-1])[:, :dim].astype(np.float64)
    n = x.shape[0]
    count, mean, var = state[0], state[1:1 + dim], state[1 + dim:]
    bm = x.sum(0) / n
    bv = ((x - bm) ** 2).sum(0) / n
    delta, tot = bm - mean, count + n
    return np.concatenate([[tot], mean + delta * n / tot, (var * count + bv * n + delta * delta * count * n / tot) / tot])


def obs_stats_bound(state, rows, dim):
    """the standard bound of recursive summation for the sums the merge is built on, with d = x - the running mean BEFORE the update:
    n u mean|d| on the mean, n u mean(d^2) on the variance, each times 4 for the merge arithmetic -> (bound_mean[dim], bound_var[dim])"""
    state = np.asarray(state, np.float64)
    x = np.asarray(rows).reshape(-1, np.shape(rows)[-1])[:, :dim].astype(np.float64)
    n = x.shape[0]
    d = x - state[1:1 + dim]
    return 4.0 * n * U64 * np.abs(d).mean(0), 4.0 * n * U64 * (d * d).mean(0)


def obs_rows(rng, n_rows, dim, stride, batch):
    """float32 [n_rows, stride] test rows: feature k < dim - 1 is scale_k (0.5 + batch + N(0, 1)) with scale_k log-spaced over 1e-3 .. 1e2
    (so the running mean moves by about a standard deviation from batch to batch); with dim >= 2 the last feature is the constant 0 (a dead
    observation slot: its variance shrinks towards 0 and inv_std towards 1 / sqrt(eps)); floats beyond dim are NaN"""
    x = np.full((n_rows, stride), np.nan, np.float32)
    live = dim - 1 if dim >= 2 else dim
    scale = np.logspace(-3.0, 2.0, live) if live > 1 else np.array([1.0])
    x[:, :live] = (scale * (0.5 + batch + rng.standard_normal((n_rows, live)))).astype(np.float32)
    if dim >= 2:
        x[:, dim - 1] = 0.0
    return x


def torch_gae_loop(S, T, N, gamma, lam, reward_scale):
    """tools/ppo_demo.py's GAE loop over storage S (tensors [T(+1), N, 1]) -> (adv, ret) before normalisation, tensors [T, N, 1]"""
    import torch
    dev = S["reward"].device
    adv = torch.zeros(T, N, 1, device=dev)
    gae = torch.zeros(N, 1, device=dev)
    rew = S["reward"] * reward_scale
    for t in reversed(range(T)):
        delta = rew[t] + gamma * S["value"][t + 1] * S["masks"][t + 1] - S["value"][t]
        gae = (delta + gamma * lam * S["masks"][t + 1] * gae) * S["bad_masks"][t + 1]
        adv[t] = gae
    ret = adv + S["value"][:T]
    return adv, ret


def storage(rng, T, N, masks="iid"):
    """random rollout storage as float32 numpy [T(+1), N]: rewards, values, masks (`masks`: "ones", "zeros", "all_zeros" or "iid": P(0) = 0.1, and
    bad_masks zero at a random 3 % of positions, some of them where masks is 0 too)"""
    rew = rng.standard_normal((T, N)).astype(np.float32)
    value = (2.0 * rng.standard_normal((T + 1, N))).astype(np.float32)
    if masks == "ones":
        m, bm = np.ones((T + 1, N), np.float32), np.ones((T + 1, N), np.float32)
    elif masks == "zeros":        # every step ends an episode; nothing is a time limit
        m, bm = np.zeros((T + 1, N), np.float32), np.ones((T + 1, N), np.float32)
    elif masks == "all_zeros":    # ... and every end is a time limit: all advantages are 0
        m, bm = np.zeros((T + 1, N), np.float32), np.zeros((T + 1, N), np.float32)
    else:
        m = (rng.random((T + 1, N)) >= 0.1).astype(np.float32)
        bm = (rng.random((T + 1, N)) >= 0.03).astype(np.float32)
        if T * N >= 16:      # at least one position where both are 0
            t, e = 1 + int(rng.integers(T)), int(rng.integers(N))
            m[t, e] = 0.0; bm[t, e] = 0.0
    return rew, value, m, bm
