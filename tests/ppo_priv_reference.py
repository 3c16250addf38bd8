"""Checker for PPO with a privileged critic (include/mocca.h mocca_set_policy_priv / mocca_ppo_grad_priv): the loss of ppo_reference with the
critic on rows and statistics of its own, stated in torch on the CPU and differentiated by autograd -- at float64 the reference, at float32
the yardstick --, the three ways an implementation can cross the two nets' inputs (MUTATIONS), a seeded factory of asymmetric policies with
the two plain policies each side's bits are compared with, and storage whose rows sit away from every discrete tie of the loss.

A policy here is ppo_reference's SimpleNamespace with critic_obs_mean / critic_inv_std added; the critic's first layer takes critic_in_dim."""
from types import SimpleNamespace

import numpy as np

import ppo_reference as R

MUTATIONS = ("critic_on_actor_rows", "critic_with_actor_statistics", "critic_first_dw_from_actor_input")
# (in_dim, critic_in_dim) of the GPU tests: both orders at one k-group, across k-groups with both paddings odd, the camera student's 244 beside
# its [obs | scan] critic, and the LDS row's bound
DIMS = ((5, 9), (9, 5), (65, 95), (244, 95), (36, 336))


def _net(rng, in_dim, hidden, acts, out):
    dims, layers = [in_dim] + list(hidden) + [out], []
    for i, act in enumerate(list(acts) + ["identity"]):
        layers.append((rng.normal(0, 1 / np.sqrt(dims[i]), (dims[i + 1], dims[i])).astype(np.float32),
                       rng.normal(0, 0.1, dims[i + 1]).astype(np.float32), act))
    return layers


def _stats(rng, dim):
    mean, var = rng.normal(0, 1, dim).astype(np.float32), rng.uniform(0.05, 4.0, dim).astype(np.float32)
    return mean, (np.float32(1) / np.sqrt(var + np.float32(1e-8))).astype(np.float32)


def make_policy(name, in_dim=None, critic_in_dim=None, norm=True, seed=0, act_dim=None):
    """The hidden layers, activations and act_dim of ppo_reference.NETS[name] (`act_dim`: another, a planner env's 15-number plan); the actor
    takes in_dim (None: the net's own), the critic critic_in_dim.  Weights and statistics as ppo_reference.make_policy draws them."""
    own, net_act_dim, hidden, acts = R.NETS[name]
    act_dim = net_act_dim if act_dim is None else act_dim
    in_dim = own if in_dim is None else in_dim
    rng = np.random.default_rng([seed, sorted(R.NETS).index(name), in_dim, critic_in_dim])
    p = SimpleNamespace(actor=_net(rng, in_dim, hidden, acts, act_dim), critic=_net(rng, critic_in_dim, hidden, acts, 1),
                        log_std=rng.uniform(-1.0, 0.2, act_dim).astype(np.float32), obs_mean=None, inv_std=None, critic_obs_mean=None,
                        critic_inv_std=None, clip=5.0, in_dim=in_dim, critic_in_dim=critic_in_dim, name=name)
    a, c = _stats(rng, in_dim), _stats(rng, critic_in_dim)
    if norm:
        (p.obs_mean, p.inv_std), (p.critic_obs_mean, p.critic_inv_std) = a, c
    return p


def actor_side(p, seed=7):
    """the PLAIN policy whose actor, log_std and statistics are p's (its critic, on the actor's rows, is drawn here)"""
    _, _, hidden, acts = R.NETS[p.name]
    rng = np.random.default_rng([seed, p.in_dim, 0])
    return SimpleNamespace(actor=p.actor, critic=_net(rng, p.in_dim, hidden, acts, 1), log_std=p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std,
                           clip=p.clip)


def critic_side(p, seed=7):
    """the PLAIN policy of in_dim = critic_in_dim whose critic and statistics are p's critic's (its actor, on the critic's rows, is drawn
    here; log_std is p's)"""
    _, act_dim, hidden, acts = R.NETS[p.name]
    rng = np.random.default_rng([seed, p.critic_in_dim, 1])
    return SimpleNamespace(actor=_net(rng, p.critic_in_dim, hidden, acts, act_dim), critic=p.critic, log_std=p.log_std, obs_mean=p.critic_obs_mean,
                           inv_std=p.critic_inv_std, clip=p.clip)


def device_policy(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip,
                        critic_obs_mean=p.critic_obs_mean, critic_inv_std=p.critic_inv_std)


def tensor_slices(p):
    return R.tensor_slices(p)


def actor_slices(p):
    """[(start, stop)] of the actor's tensors and log_std in flat_params' order"""
    s = R.tensor_slices(p)
    return s[:2 * len(p.actor)] + s[-1:]


def critic_slices(p):
    return R.critic_slices(p)


def make_storage(p, n_rows, seed=0):
    """Rollout storage for the asymmetric policy p, each side away from the loss's ties by ppo_reference.make_storage's construction: the
    actor's fields (obs, action, old_logp, adv) are those of actor_side(p)'s storage, the critic's (critic_obs, returns, old_value) those of
    critic_side(p)'s.  -> (storage with critic_obs [R, critic_in_dim], the actor side's storage, the critic side's storage)"""
    st_a, st_c = R.make_storage(actor_side(p), n_rows, seed=seed), R.make_storage(critic_side(p), n_rows, seed=seed + 100)
    st = dict(obs=st_a["obs"], critic_obs=st_c["obs"], action=st_a["action"], old_logp=st_a["old_logp"], adv=st_a["adv"],
              returns=st_c["returns"], old_value=st_c["old_value"])
    return st, st_a, st_c


def _fit(x, dim):
    """the first `dim` columns of x, zeros where x is narrower: what a crossed implementation would read"""
    out = np.zeros(x.shape[:-1] + (dim,), x.dtype)
    k = min(dim, x.shape[-1])
    out[..., :k] = x[..., :k]
    return out


def loss_autograd(p, batch, dtype="float64", clip=R.CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False, mutate=None, separately=False):
    """ppo_reference.loss_autograd with the critic on batch["critic_obs"] [B, critic_in_dim] under critic_obs_mean / critic_inv_std.
    `mutate`: one of MUTATIONS.  `separately`: the actor's and log_std's gradient from L_pi - entropy_coef H alone and the critic's from
    value_coef L_v alone, two backward passes -- the loss separates, so this is the same gradient.
    -> SimpleNamespace(grad flat [n_head], stats [6], logp [B], value [B])"""
    import torch
    dt = getattr(torch, dtype)
    t = lambda x: torch.tensor(np.asarray(x), dtype=dt)
    leaves, firsts = [], []

    def net(layers, x):
        for i, (w, b, act) in enumerate(layers):
            w, b = t(w).requires_grad_(), t(b).requires_grad_()
            leaves.extend([w, b])
            z = x @ w.T + b
            if i == 0:
                firsts.append(z)
            x = R._activate(torch, z, act)
        return x

    def normalised(x, mean, inv_std):
        return x if mean is None else torch.clamp((x - t(mean)) * t(inv_std), -p.clip, p.clip)

    x_a = normalised(t(batch["obs"]), p.obs_mean, p.inv_std)
    rows_c, mean_c, inv_c = batch["critic_obs"], p.critic_obs_mean, p.critic_inv_std
    if mutate == "critic_on_actor_rows":
        rows_c = _fit(np.asarray(batch["obs"]), p.critic_in_dim)
    elif mutate == "critic_with_actor_statistics" and p.obs_mean is not None:
        mean_c, inv_c = _fit(p.obs_mean, p.critic_in_dim), _fit(p.inv_std, p.critic_in_dim)
    elif mutate not in (None, "critic_with_actor_statistics", "critic_first_dw_from_actor_input"):
        raise ValueError(mutate)
    x_c = normalised(t(rows_c), mean_c, inv_c)
    mu, v = net(p.actor, x_a), net(p.critic, x_c)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    z = (t(batch["action"]) - mu) / torch.exp(log_std)
    logp = (-0.5 * z * z - log_std - R.HALF_LOG_2PI).sum(-1)
    old_logp, adv, ret = t(batch["old_logp"]), t(batch["adv"]), t(batch["returns"])
    r = torch.exp(logp - old_logp)
    surr = torch.min(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    l_v = (v - ret) ** 2
    if value_clip:
        v_old = t(batch["old_value"])
        l_v = torch.max(l_v, (v_old + torch.clamp(v - v_old, -clip, clip) - ret) ** 2)
    l_v = 0.5 * l_v.mean()
    entropy = (log_std + 0.5 + R.HALF_LOG_2PI).sum()
    l_actor, l_critic = -surr.mean() - entropy_coef * entropy, value_coef * l_v
    n_a = 2 * len(p.actor)
    wanted = leaves + [firsts[1]]
    if separately:
        g_a = torch.autograd.grad(l_actor, leaves[:n_a] + leaves[-1:], retain_graph=True)
        g_c = torch.autograd.grad(l_critic, leaves[n_a:-1] + [firsts[1]])
        grads = list(g_a[:-1]) + list(g_c[:-1]) + [g_a[-1], g_c[-1]]
    else:
        grads = list(torch.autograd.grad(l_actor + l_critic, wanted))
    if mutate == "critic_first_dw_from_actor_input":      # dW = dZ^T A0 with A0 the ACTOR's normalised tile where the critic's belongs
        grads[n_a] = grads[-1].T @ t(_fit(x_a.detach().numpy(), p.critic_in_dim))
    grad = np.concatenate([g.numpy().reshape(-1) for g in grads[:-1]])
    lo, hi = t(1.0) - t(clip), t(1.0) + t(clip)
    clipped = ((r > hi) | (r < lo)).to(dt).mean()
    stats = np.array([surr.mean().item(), l_v.item(), entropy.item(), (old_logp - logp).mean().item(), clipped.item(),
                      float((grad.astype(np.float64) ** 2).sum())])
    return SimpleNamespace(grad=grad, stats=stats, logp=logp.detach().numpy(), value=v.detach().numpy())


def side_errors(slices, got, want64):
    """ppo_reference.tensor_errors over `slices` alone"""
    out = []
    for a, b in slices:
        scale = np.abs(want64[a:b]).max()
        out.append(np.abs(np.asarray(got[a:b], np.float64) - want64[a:b]) / (scale if scale > 0 else 1.0))
    return np.concatenate(out)


def forward64(p, obs, critic_obs):
    """-> (mean [N, A], value [N]) in float64"""
    x_a = R.normalise64(p, obs)
    x_c = np.asarray(critic_obs, np.float64)
    if p.critic_obs_mean is not None:
        x_c = np.clip((x_c - np.asarray(p.critic_obs_mean, np.float64)) * np.asarray(p.critic_inv_std, np.float64), -p.clip, p.clip)
    return R._forward64(p.actor, x_a)[-1], R._forward64(p.critic, x_c)[-1][:, 0]
