"""Checker for mocca_distill_grad (include/mocca.h; mocca_envs_amd/csrc/mocca_ppo.hip, PPO_DISTIL): the regression loss stated in torch on
the CPU and differentiated by autograd -- at float64 the reference, at float32 the yardstick --, the header's per-row lines in float64
numpy, a seeded factory of stored rows whose targets are a second net's outputs plus noise, the GPU test's acceptance rule as a function,
and the mutations that rule must refuse.  Policies and the parity helpers are tests/ppo_reference.py's."""
from types import SimpleNamespace

import numpy as np

import ppo_reference as R
from ppo_reference import gather  # noqa: F401  (re-exported for the tests)

HALF_LOG_2PI = R.HALF_LOG_2PI
MUTATIONS = ("no_inv_a", "no_factor_2", "flipped_sign", "rolled_targets", "value_leaks_into_actor", "entropy_on_log_std")


def make_storage(name, p, n_rows, seed=0):
    """`n_rows` stored rows for policy `p` = make_policy(name, ..): obs ~ N(0, 3^2); target = the actor mean of a differently seeded net of
    the same shape (seed + 100) plus N(0, 0.1^2) noise, value_target its value plus noise; nets with a relu keep rows whose f64 pre-activations all
    lie RELU_MARGIN away from 0, as ppo_reference.make_storage does.  -> dict of float32 arrays obs [R, in_dim], target [R, A],
    value_target [R]"""
    rng = np.random.default_rng([seed, n_rows, 11])
    in_dim, act_dim = p.actor[0][0].shape[1], p.log_std.size
    relu = any(act == "relu" for _, _, act in p.actor + p.critic)
    obs = rng.normal(0, 3.0, (2 * n_rows + 64 if relu else n_rows, in_dim)).astype(np.float32)
    if relu:
        probe = dict(obs=obs, target=np.zeros((obs.shape[0], act_dim)), value_target=np.zeros(obs.shape[0]))
        pre = loss_autograd(p, probe).pre
        keep = np.all([np.all(np.abs(z) > R.RELU_MARGIN, axis=1) for z in pre], axis=0)
        obs = obs[keep][:n_rows]
        assert obs.shape[0] == n_rows, "too few candidate rows"
    labeller = R.make_policy(name, norm=p.obs_mean is not None, seed=seed + 100)
    x = R.normalise64(labeller, obs)
    mu, v = R._forward64(labeller.actor, x)[-1], R._forward64(labeller.critic, x)[-1][:, 0]
    return dict(obs=obs, target=(mu + rng.normal(0, 0.1, mu.shape)).astype(np.float32),
                value_target=(v + rng.normal(0, 0.1, v.shape)).astype(np.float32))


def loss_autograd(p, batch, dtype="float64", distill_coef=1.0, value_coef=0.5, use_value=True, mutation=None):
    """`distill_coef * (mean - target).pow(2).mean() + value_coef * 0.5 * (v - vt).pow(2).mean()` (the second term only with `use_value`) in
    torch on the CPU at `dtype`, differentiated by autograd.  `batch`: obs [B, in_dim] (raw), target [B, A], value_target [B], already
    gathered.  `mutation`: one of MUTATIONS, a deliberately wrong loss (the negative controls).
    -> SimpleNamespace(grad flat [n_head], stats [8] as mocca_distill_grad lays them out, pre: every layer's pre-activations)"""
    import torch
    dt = getattr(torch, dtype)
    t = lambda x: torch.tensor(np.asarray(x), dtype=dt)
    leaves, pre = [], []

    def net(layers, x):
        for w, b, act in layers:
            w, b = t(w).requires_grad_(), t(b).requires_grad_()
            leaves.extend([w, b])
            z = x @ w.T + b
            pre.append(z.detach().numpy())
            x = R._activate(torch, z, act)
        return x

    x = t(batch["obs"])
    if p.obs_mean is not None:
        x = torch.clamp((x - t(p.obs_mean)) * t(p.inv_std), -p.clip, p.clip)
    mu, v = net(p.actor, x), net(p.critic, x)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    target = t(batch["target"])
    if mutation == "rolled_targets":
        target = torch.roll(target, 1, dims=1)
    l_d = (mu - target).pow(2).mean()
    if mutation == "no_inv_a":
        l_d = (mu - target).pow(2).sum(-1).mean()
    if mutation == "no_factor_2":
        l_d = 0.5 * l_d
    if mutation == "flipped_sign":
        l_d = -l_d
    l_v = 0.5 * (v - t(batch["value_target"])).pow(2).mean() if use_value else torch.zeros((), dtype=dt)
    loss = distill_coef * l_d + value_coef * l_v
    if mutation == "value_leaks_into_actor":
        loss = loss + value_coef * 0.5 * (mu[:, 0] - t(batch["value_target"])).pow(2).mean()
    entropy = (log_std + 0.5 + HALF_LOG_2PI).sum()
    if mutation == "entropy_on_log_std":
        loss = loss - 0.01 * entropy
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = np.concatenate([(torch.zeros_like(leaf) if g is None else g).numpy().reshape(-1) for g, leaf in zip(grads, leaves)])
    stats = np.array([0.0, l_v.item(), entropy.item(), 0.0, 0.0, float((grad.astype(np.float64) ** 2).sum()), 0.0, l_d.item()])
    return SimpleNamespace(grad=grad, stats=stats, pre=pre)


def grad_by_hand(p, batch, distill_coef=1.0, value_coef=0.5, use_value=True):
    """the per-row lines of include/mocca.h (mocca_distill_grad) in float64 numpy -> the flat gradient"""
    f = lambda k: np.asarray(batch[k], np.float64)
    x = R.normalise64(p, f("obs"))
    n, a = x.shape[0], p.log_std.size
    za, zc = [], []
    ya, yc = R._forward64(p.actor, x, za), R._forward64(p.critic, x, zc)
    ib, ia, k2 = 1.0 / n, 1.0 / a, 2.0 * distill_coef
    d = ya[-1] - f("target")
    d_mu = d * ib * ia * k2
    d_v = np.zeros((n, 1))
    if use_value:
        d_v = (value_coef * (yc[-1][:, 0] - f("value_target")) * ib)[:, None]
    parts = R._backward64(p.actor, ya, za, d_mu) + R._backward64(p.critic, yc, zc, d_v) + [np.zeros(a)]
    return np.concatenate([np.asarray(q).reshape(-1) for q in parts])


def zero_tensors(p, want64):
    """[(start, stop)] of the parameter tensors whose float64 gradient is identically zero (log_std always; the critic's without value targets)"""
    return [(a, b) for a, b in R.tensor_slices(p) if not np.any(want64[a:b])]


def pooled_errors(p, got, want64):
    """the parity rule's errors (ppo_reference.tensor_errors) over the tensors whose f64 gradient is NOT identically zero"""
    out = []
    for a, b in R.tensor_slices(p):
        scale = np.abs(want64[a:b]).max()
        if scale > 0:
            out.append(np.abs(np.asarray(got[a:b], np.float64) - want64[a:b]) / scale)
    return np.concatenate(out)


def zero_bits_ok(p, got, want64):
    """every tensor whose f64 gradient is identically zero is all +0.0f bits in `got` (float32)"""
    got = np.asarray(got, np.float32)
    return all(not got[a:b].view(np.uint32).any() for a, b in zero_tensors(p, want64))


def accepts(p, got, f32, want64):
    """the GPU test's rule for one configuration: `got` (float32 flat gradient) stays within 3 x the float32-autograd gradient `f32` against
    the float64 gradient `want64` at the median, the 99th percentile and the maximum of the pooled per-tensor errors, and the tensors
    whose f64 gradient is identically zero are all +0.0f bits"""
    return zero_bits_ok(p, got, want64) and R.within(R.triple(pooled_errors(p, got, want64)), R.triple(pooled_errors(p, f32, want64)))
