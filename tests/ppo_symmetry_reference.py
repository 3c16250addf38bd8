"""Checker for mocca_ppo_grad_sym (include/mocca.h; mocca_envs_amd/csrc/mocca_ppo.h: Symmetric policy), built on ppo_reference and
policy_symmetry_reference: PPO's minibatch loss of the mirror-symmetric policy

    mu = 1/2 (f(n(s)) + M_a f(n(M_o s)))     ls[j] = 1/2 (log_std[j] + log_std[act_perm[j]])     v = 1/2 (V(n(s)) + V(n(M_o s)))

stated in torch on the CPU and differentiated by autograd -- at float64 the reference, at float32 the yardstick --, the same gradient from
the header's by-hand formulas in float64 numpy, a seeded factory of rollout storage away from every discrete tie of the loss, and mutations:
definitions that differ from the right one the way a kernel bug would, in the forward (policy_symmetry_reference.MUTATIONS) or in the
backward alone (BACKWARD_MUTATIONS: the forward values, and so the loss and the statistics, are the right ones).

A policy is ppo_reference's SimpleNamespace; tables are (in_perm, in_sign, act_perm, act_sign)."""
from types import SimpleNamespace

import numpy as np

import policy_symmetry_reference as S
import ppo_reference as R
from policy_symmetry_reference import MUTATIONS, mirror, random_tables  # noqa: F401  (re-exported for the tests)
from ppo_reference import CLIP, HALF_LOG_2PI, RATIOS, RELU_MARGIN

BACKWARD_MUTATIONS = ("mirror_detached",   # f2 and v2 are constants: the mirrored pass gets no gradient
                      "back_no_sign",      # dL/df2[pj] = h, without act_sign[j]
                      "back_no_perm",      # dL/df2[j] = h act_sign[j]: routed to j, not to act_perm[j]
                      "log_std_half")      # only T[j] reaches log_std[j]: 1/2 T[j] in place of 1/2 (T[j] + T[pj])


def identity_tables(in_dim, act_dim):
    return (np.arange(in_dim, dtype=np.int32), np.ones(in_dim, np.float32), np.arange(act_dim, dtype=np.int32), np.ones(act_dim, np.float32))


def loss_autograd_sym(p, tables, batch, dtype="float64", clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False, how=None):
    """ppo_reference.loss_autograd for the symmetric policy: the loss of include/mocca.h mocca_ppo_grad_sym in torch on the CPU at `dtype`,
    differentiated by autograd.  `how`: None, one of MUTATIONS (the forward differs) or of BACKWARD_MUTATIONS (only the gradient differs).
    -> SimpleNamespace(grad flat [n_head], stats [6], logp [B], value [B], pre: every layer's pre-activations, of both passes)"""
    import torch
    if how not in (None,) + MUTATIONS + BACKWARD_MUTATIONS:
        raise ValueError(how)
    dt = getattr(torch, dtype)
    t = lambda x: torch.tensor(np.asarray(x), dtype=dt)
    in_perm, in_sign, act_perm, act_sign = tables
    if how == "no_sign":
        in_sign, act_sign = np.ones_like(in_sign), np.ones_like(act_sign)
    elif how == "no_perm":
        in_perm, act_perm = np.arange(len(in_perm)), np.arange(len(act_perm))
    in_perm, act_perm = torch.tensor(np.asarray(in_perm, np.int64)), torch.tensor(np.asarray(act_perm, np.int64))
    in_sign, act_sign = t(in_sign), t(act_sign)
    pre = []
    nets = []
    for layers in (p.actor, p.critic):      # leaves in flat_params' order: the actor's layers, then the critic's
        nets.append([(t(w).requires_grad_(), t(b).requires_grad_(), act) for w, b, act in layers])
    leaves = [q for net in nets for w, b, _ in net for q in (w, b)]

    def run(net, x):
        for w, b, act in net:
            z = x @ w.T + b
            pre.append(z.detach().numpy())
            x = R._activate(torch, z, act)
        return x

    def normalise(x):
        return x if p.obs_mean is None else torch.clamp((x - t(p.obs_mean)) * t(p.inv_std), -p.clip, p.clip)

    x = t(batch["obs"])
    x1 = normalise(x)
    x2 = x1[:, in_perm] * in_sign if how == "mirror_after_norm" else normalise(x[:, in_perm] * in_sign)
    f1, f2, v1, v2 = run(nets[0], x1), run(nets[0], x2), run(nets[1], x1)[:, 0], run(nets[1], x2)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    half = 1.0 if how == "no_half" else 0.5
    mm = f2[:, act_perm] * act_sign
    if how == "mirror_detached":
        mm, v2 = mm.detach(), v2.detach()
    elif how == "back_no_sign":
        mm = mm.detach() + (f2[:, act_perm] - f2[:, act_perm].detach())
    elif how == "back_no_perm":
        mm = mm.detach() + (f2 * act_sign - (f2 * act_sign).detach())
    mu, v = half * (f1 + mm), half * (v1 + v2)
    ls = 0.5 * (log_std + log_std[act_perm])
    ls_p = 0.5 * (log_std + log_std[act_perm].detach()) if how == "log_std_half" else ls      # what logp differentiates
    z = (t(batch["action"]) - mu) / torch.exp(ls_p)
    logp = (-0.5 * z * z - ls_p - HALF_LOG_2PI).sum(-1)
    old_logp, adv, ret = t(batch["old_logp"]), t(batch["adv"]), t(batch["returns"])
    r = torch.exp(logp - old_logp)
    surr = torch.min(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    l_v = (v - ret) ** 2
    if value_clip:
        v_old = t(batch["old_value"])
        l_v = torch.max(l_v, (v_old + torch.clamp(v - v_old, -clip, clip) - ret) ** 2)
    l_v = 0.5 * l_v.mean()
    entropy = (ls + 0.5 + HALF_LOG_2PI).sum()
    loss = -surr.mean() + value_coef * l_v - entropy_coef * entropy
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = np.concatenate([(torch.zeros_like(leaf) if g is None else g).numpy().reshape(-1) for g, leaf in zip(grads, leaves)])
    lo, hi = t(1.0) - t(clip), t(1.0) + t(clip)
    clipped = ((r > hi) | (r < lo)).to(dt).mean()
    stats = np.array([surr.mean().item(), l_v.item(), entropy.item(), (old_logp - logp).mean().item(), clipped.item(),
                      float((grad.astype(np.float64) ** 2).sum())])
    return SimpleNamespace(grad=grad, stats=stats, logp=logp.detach().numpy(), value=v.detach().numpy(), pre=pre)


def grad_by_hand_sym(p, tables, batch, clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False):
    """the per-row formulas of include/mocca.h mocca_ppo_grad_sym in float64 numpy -> the flat gradient: mocca_ppo_grad's lines on the
    symmetrised mu, ls, v; each head receives its half; every weight's gradient is the sum over both passes"""
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    f = lambda k: np.asarray(batch[k], np.float64)
    sign = act_sign.astype(np.float64)

    def normalise(x):
        if p.obs_mean is None:
            return x
        return np.clip((x - np.asarray(p.obs_mean, np.float64)) * np.asarray(p.inv_std, np.float64), -p.clip, p.clip)

    x1, x2 = normalise(f("obs")), normalise(mirror(f("obs"), in_perm, in_sign))
    n = x1.shape[0]
    za1, za2, zc1, zc2 = [], [], [], []
    ya1, ya2, yc1, yc2 = R._forward64(p.actor, x1, za1), R._forward64(p.actor, x2, za2), R._forward64(p.critic, x1, zc1), R._forward64(p.critic, x2, zc2)
    mu = 0.5 * (ya1[-1] + ya2[-1][:, act_perm] * sign)
    log_std = np.asarray(p.log_std, np.float64)
    ls = 0.5 * (log_std + log_std[act_perm])
    s = np.exp(ls)
    z = (f("action") - mu) / s
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    r, adv = np.exp(logp - f("old_logp")), f("adv")
    inactive = ((adv > 0) & (r > 1 + clip)) | ((adv < 0) & (r < 1 - clip))
    g = np.where(inactive, 0.0, -(adv * r) / n)[:, None]
    h = 0.5 * (g * (z / s))
    d_f1, d_f2 = h, np.zeros_like(h)
    d_f2[:, act_perm] = h * sign      # dL/df2[pj] = h[j] * act_sign[j]
    big_t = (g * (z * z - 1)).sum(0)
    d_ls = 0.5 * (big_t + big_t[act_perm]) - entropy_coef
    v, ret = 0.5 * (yc1[-1][:, 0] + yc2[-1][:, 0]), f("returns")
    d_v = v - ret
    if value_clip:
        dd = v - f("old_value")
        e2 = f("old_value") + np.clip(dd, -clip, clip) - ret
        d_v = np.where((np.abs(dd) > clip) & (e2 * e2 > d_v * d_v), 0.0, d_v)
    d_v = 0.5 * (value_coef * d_v / n)[:, None]
    actor = [a + b for a, b in zip(R._backward64(p.actor, ya1, za1, d_f1), R._backward64(p.actor, ya2, za2, d_f2))]
    critic = [a + b for a, b in zip(R._backward64(p.critic, yc1, zc1, d_v), R._backward64(p.critic, yc2, zc2, d_v))]
    return np.concatenate([np.asarray(q).reshape(-1) for q in actor + critic + [d_ls]])


def make_storage_sym(p, tables, n_rows, seed=0, clip=CLIP):
    """ppo_reference.make_storage for the symmetric policy: rollout storage of `n_rows` rows away from every discrete tie BY CONSTRUCTION
    (no row is left out afterwards).  Actions and old_logp come from the SYMMETRIC float64 forward -- a = mu_sym + exp(ls_sym) eps,
    old_logp = logp_sym - log(r*) with r* one of RATIOS x (1 +- 0.01) --, v_old and the returns are placed around the symmetric value as
    make_storage places them around the plain one, and the rows of a net with a relu keep every float64 pre-activation of BOTH passes
    RELU_MARGIN from 0.  -> dict of float32 arrays obs [R, in_dim], action [R, A], old_logp, adv, returns, old_value [R]"""
    rng = np.random.default_rng([seed, n_rows, 6])
    in_dim, act_dim = p.actor[0][0].shape[1], p.log_std.size
    relu = any(act == "relu" for _, _, act in p.actor + p.critic)
    obs = rng.normal(0, 3.0, (4 * n_rows + 64 if relu else n_rows, in_dim)).astype(np.float32)
    zero = np.zeros(obs.shape[0])
    probe = dict(obs=obs, action=np.zeros((obs.shape[0], act_dim)), old_logp=zero, adv=zero, returns=zero, old_value=zero)
    if relu:
        pre = loss_autograd_sym(p, tables, probe).pre      # both passes of both nets
        keep = np.all([np.all(np.abs(z) > RELU_MARGIN, axis=1) for z in pre], axis=0)
        obs = obs[keep][:n_rows]
        assert obs.shape[0] == n_rows, "too few candidate rows"
        probe = {k: v[:n_rows] for k, v in probe.items()}
        probe["obs"] = obs
    mu64, _ = S.sym_forward64(p, tables, obs)
    action = (mu64 + np.exp(S.log_std_sym(p, tables)) * rng.normal(0, 1, mu64.shape)).astype(np.float32)
    probe["action"] = action
    fwd = loss_autograd_sym(p, tables, probe)     # logp of the float32 actions, value
    ratio = rng.choice(RATIOS, n_rows) * (1 + rng.choice([-1.0, 1.0], n_rows) * rng.uniform(0.002, 0.01, n_rows))
    old_logp = (fwd.logp - np.log(ratio)).astype(np.float32)
    adv = (rng.choice([-1.0, 1.0], n_rows) * rng.uniform(0.1, 2.0, n_rows)).astype(np.float32)
    v = fwd.value
    clipped = rng.random(n_rows) < 0.5
    gap = np.where(clipped, rng.uniform(0.35, 0.8, n_rows), rng.uniform(0.0, 0.08, n_rows)) * rng.choice([-1.0, 1.0], n_rows)
    old_value = (v - gap).astype(np.float32)
    returns = (v + rng.normal(0, 0.7, n_rows)).astype(np.float32)
    for _ in range(64):
        vc = old_value.astype(np.float64) + np.clip(v - old_value, -clip, clip)
        tie = clipped & (np.abs((v - returns) ** 2 - (vc - returns) ** 2) <= 2e-3)
        if not tie.any():
            break
        returns[tie] = (v[tie] + rng.normal(0, 0.7, int(tie.sum()))).astype(np.float32)
    assert not tie.any()
    gap32 = np.abs(v - old_value.astype(np.float64))
    assert np.all((gap32 < 0.1) | (gap32 > 0.3))
    return dict(obs=obs, action=action, old_logp=old_logp, adv=adv, returns=returns, old_value=old_value)


def mirror_storage(storage, tables):
    """the storage of the mirrored rollout: (M_o s, M_a a) with the same old_logp, adv, returns and old_value"""
    in_perm, in_sign, act_perm, act_sign = tables
    return dict(storage, obs=mirror(storage["obs"], in_perm, in_sign), action=mirror(storage["action"], act_perm, act_sign))
