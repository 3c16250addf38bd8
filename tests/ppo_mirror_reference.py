"""Checker for mocca_ppo_grad_mirror (include/mocca.h; mocca_envs_amd/csrc/mocca_ppo.h: Mirror loss), built on ppo_reference: PPO's
minibatch loss of the PLAIN policy with the mirror-symmetry loss added,

    L = L_ppo + coef L_m        L_m = mean over rows and actions of (f(n(s)) - M_a f(n(M_o s)))^2,

stated in torch on the CPU and differentiated by autograd -- at float64 the reference, at float32 the yardstick --, the same gradient from
the header's by-hand formulas in float64 numpy, and mutations: definitions of the term that differ from the right one the way a kernel
bug would (MUTATIONS).  The storage is ppo_reference.make_storage's: the term is smooth in the actor's output and adds no discrete tie.

A policy is ppo_reference's SimpleNamespace; tables are (in_perm, in_sign, act_perm, act_sign)."""
from types import SimpleNamespace

import numpy as np

import ppo_reference as R
from policy_symmetry_reference import mirror, random_tables  # noqa: F401  (re-exported for the tests)
from ppo_reference import CLIP, HALF_LOG_2PI, critic_slices  # noqa: F401
from ppo_symmetry_reference import identity_tables, mirror_storage  # noqa: F401

MUTATIONS = ("mirror_detached",   # f2 is a constant: the mirrored pass gets no gradient
             "no_sign",           # d_j = f1[j] - f2[act_perm[j]], act_sign dropped
             "no_perm",           # d_j = f1[j] - act_sign[j] f2[j], act_perm dropped
             "rows_only")         # the mean over the rows alone: the 1 / A is missing


def loss_autograd_mirror(p, tables, coef, batch, dtype="float64", clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False, how=None):
    """ppo_reference.loss_autograd with `coef` L_m added: the loss of include/mocca.h mocca_ppo_grad_mirror in torch on the CPU at `dtype`,
    differentiated by autograd.  `how`: None or one of MUTATIONS.
    -> SimpleNamespace(grad flat [n_head], stats [8] (ppo_reference's six, 0, L_m), logp [B], value [B], pre: the pre-activations of the
    actor's as-given pass, its mirrored pass and the critic's as-given pass)"""
    import torch
    if how not in (None,) + MUTATIONS:
        raise ValueError(how)
    dt = getattr(torch, dtype)
    t = lambda x: torch.tensor(np.asarray(x), dtype=dt)
    in_perm, in_sign, act_perm, act_sign = tables
    if how == "no_sign":
        act_sign = np.ones_like(act_sign)
    elif how == "no_perm":
        act_perm = np.arange(len(act_perm))
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
    x1, x2 = normalise(x), normalise(x[:, in_perm] * in_sign)      # the mirror on the RAW row
    f1, f2, v = run(nets[0], x1), run(nets[0], x2), run(nets[1], x1)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    mm = f2[:, act_perm] * act_sign
    if how == "mirror_detached":
        mm = mm.detach()
    d = f1 - mm
    l_m = (d * d).sum(-1).mean() if how == "rows_only" else (d * d).mean()
    z = (t(batch["action"]) - f1) / torch.exp(log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    old_logp, adv, ret = t(batch["old_logp"]), t(batch["adv"]), t(batch["returns"])
    r = torch.exp(logp - old_logp)
    surr = torch.min(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    l_v = (v - ret) ** 2
    if value_clip:
        v_old = t(batch["old_value"])
        l_v = torch.max(l_v, (v_old + torch.clamp(v - v_old, -clip, clip) - ret) ** 2)
    l_v = 0.5 * l_v.mean()
    entropy = (log_std + 0.5 + HALF_LOG_2PI).sum()
    loss = -surr.mean() + value_coef * l_v - entropy_coef * entropy + coef * l_m
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = np.concatenate([(torch.zeros_like(leaf) if g is None else g).numpy().reshape(-1) for g, leaf in zip(grads, leaves)])
    lo, hi = t(1.0) - t(clip), t(1.0) + t(clip)
    clipped = ((r > hi) | (r < lo)).to(dt).mean()
    stats = np.array([surr.mean().item(), l_v.item(), entropy.item(), (old_logp - logp).mean().item(), clipped.item(),
                      float((grad.astype(np.float64) ** 2).sum()), 0.0, l_m.item()])
    return SimpleNamespace(grad=grad, stats=stats, logp=logp.detach().numpy(), value=v.detach().numpy(), pre=pre)


def grad_by_hand_mirror(p, tables, coef, batch, clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False):
    """the per-row formulas of include/mocca.h mocca_ppo_grad_mirror in float64 numpy -> (the flat gradient, L_m): mocca_ppo_grad's lines on
    the plain mu = f1, ls, v; u = 2 coef d / (B A) added to dL/df1[j], -(u act_sign[j]) handed to f2[act_perm[j]]; the actor's weight
    gradients are the sum over both passes, the critic has the as-given pass alone"""
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    f = lambda k: np.asarray(batch[k], np.float64)
    sign = act_sign.astype(np.float64)

    def normalise(x):
        if p.obs_mean is None:
            return x
        return np.clip((x - np.asarray(p.obs_mean, np.float64)) * np.asarray(p.inv_std, np.float64), -p.clip, p.clip)

    x1, x2 = normalise(f("obs")), normalise(mirror(f("obs"), in_perm, in_sign))
    n, n_act = x1.shape[0], act_perm.size
    za1, za2, zc = [], [], []
    ya1, ya2, yc = R._forward64(p.actor, x1, za1), R._forward64(p.actor, x2, za2), R._forward64(p.critic, x1, zc)
    ls = np.asarray(p.log_std, np.float64)
    s = np.exp(ls)
    z = (f("action") - ya1[-1]) / s
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    r, adv = np.exp(logp - f("old_logp")), f("adv")
    inactive = ((adv > 0) & (r > 1 + clip)) | ((adv < 0) & (r < 1 - clip))
    g = np.where(inactive, 0.0, -(adv * r) / n)[:, None]
    d = ya1[-1] - ya2[-1][:, act_perm] * sign
    u = d / n / n_act * (2.0 * coef)
    d_f1, d_f2 = g * (z / s) + u, np.zeros_like(u)
    d_f2[:, act_perm] = -(u * sign)      # dL/df2[pj] = -(u[j] * act_sign[j])
    d_ls = (g * (z * z - 1)).sum(0) - entropy_coef
    v, ret = yc[-1][:, 0], f("returns")
    d_v = v - ret
    if value_clip:
        dd = v - f("old_value")
        e2 = f("old_value") + np.clip(dd, -clip, clip) - ret
        d_v = np.where((np.abs(dd) > clip) & (e2 * e2 > d_v * d_v), 0.0, d_v)
    d_v = (value_coef * d_v / n)[:, None]
    actor = [a + b for a, b in zip(R._backward64(p.actor, ya1, za1, d_f1), R._backward64(p.actor, ya2, za2, d_f2))]
    parts = actor + R._backward64(p.critic, yc, zc, d_v) + [d_ls]
    return np.concatenate([np.asarray(q).reshape(-1) for q in parts]), float((d * d).sum(-1).mean() / n_act)
