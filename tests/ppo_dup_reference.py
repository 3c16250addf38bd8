"""Checker for mocca_ppo_grad_dup (include/mocca.h; mocca_envs_amd/csrc/mocca_ppo.h: Duplicated rows), built on ppo_reference: PPO's
minibatch loss of the PLAIN policy over 2 B samples -- every row (s, a) and its twin (M_o s, M_a a), which borrows the row's old_logp, adv,
returns and old_value --, every mean over 2 B,

stated in torch on the CPU and differentiated by autograd -- at float64 the reference, at float32 the yardstick --, the same gradient from
the header's by-hand lines in float64 numpy, mutations: ways of forming the twins that differ from the right one the way a kernel bug
would (MUTATIONS), and a storage factory whose rows AND twins sit away from every discrete tie of the loss.

A policy is ppo_reference's SimpleNamespace; tables are (in_perm, in_sign, act_perm, act_sign)."""
from types import SimpleNamespace

import numpy as np

import ppo_reference as R
from policy_symmetry_reference import mirror, random_tables  # noqa: F401  (re-exported for the tests)
from ppo_reference import CLIP, HALF_LOG_2PI, critic_slices  # noqa: F401
from ppo_symmetry_reference import identity_tables  # noqa: F401

MUTATIONS = ("action_not_mirrored",   # the twin keeps the row's action
             "obs_not_mirrored",      # the twin keeps the row's observation
             "no_sign",               # in_sign and act_sign dropped
             "no_perm",               # in_perm and act_perm dropped
             "mean_over_b",           # ib = 1 / B: every mean is a sum over 2 B samples divided by B
             "twin_critic_dead")      # the critic's twins contribute nothing: the value loss sums the as-given rows alone (over 2 B)


HEAD_SCALE = 0.1


# not ppo_reference.make_policy under another name: the actor's output layer is scaled by HEAD_SCALE
def make_policy(name, norm=True, seed=0, acts=None):
    """ppo_reference.make_policy with the actor's output layer scaled by HEAD_SCALE: a policy that is CLOSE TO mirror-symmetric, which is
    what the method assumes of pi_old (a twin borrows its row's old_logp) and what a trainer's small-gain initialisation of that layer
    gives.  ppo_reference's own policies have mean(s) and M_a mean(M_o s) several standard deviations apart: no action is then likely under
    both, a sample of one kind sits at |z| of 4 to 5 and |logp| of 40, and the float32 rounding of that ONE scalar (an ulp of its largest
    terms, ~1e-6, straight into the ratio) outweighs everything else in a small minibatch -- the parity rule would compare one draw of it
    with another.  Scaled, both kinds of sample have |z| ~ 1 as a rollout's have, and the rule sees the kernel's sums."""
    p = R.make_policy(name, norm=norm, seed=seed, acts=acts)
    w, b, act = p.actor[-1]
    p.actor[-1] = (w * np.float32(HEAD_SCALE), b * np.float32(HEAD_SCALE), act)
    return p


def concatenate(batch, tables):
    """the 2 B-row minibatch: the B rows, then their mirror images with the rows' own old_logp, adv, returns and old_value.  A mirror
    permutes and flips signs: the twins' float32 entries are exact"""
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    obs, action = np.asarray(batch["obs"]), np.asarray(batch["action"])
    out = {k: np.concatenate([np.asarray(v), np.asarray(v)]) for k, v in batch.items() if k not in ("obs", "action")}
    out["obs"] = np.concatenate([obs, obs[:, in_perm] * in_sign.astype(obs.dtype)])
    out["action"] = np.concatenate([action, action[:, act_perm] * act_sign.astype(action.dtype)])
    return out


def _mutate(tables, how):
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    if how == "no_sign":
        in_sign, act_sign = np.ones_like(in_sign), np.ones_like(act_sign)
    if how == "no_perm":
        in_perm, act_perm = np.arange(in_perm.size), np.arange(act_perm.size)
    if how == "action_not_mirrored":
        act_perm, act_sign = np.arange(act_perm.size), np.ones_like(act_sign)
    if how == "obs_not_mirrored":
        in_perm, in_sign = np.arange(in_perm.size), np.ones_like(in_sign)
    return in_perm, in_sign, act_perm, act_sign


def loss_autograd_dup(p, tables, batch, dtype="float64", clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False, how=None):
    """The loss of include/mocca.h mocca_ppo_grad_dup in torch on the CPU at `dtype`, differentiated by autograd: the plain PPO loss on
    concatenate()'s 2 B rows.  `batch`: the B rows, already gathered.  `how`: None or one of MUTATIONS.
    -> SimpleNamespace(grad flat [n_head], stats [8] (ppo_reference's six over 2 B, 0, the twins' share of [3]), logp [2 B], value [2 B],
    pre: every layer's pre-activations)"""
    import torch
    if how not in (None,) + MUTATIONS:
        raise ValueError(how)
    dt = getattr(torch, dtype)
    t = lambda x: torch.tensor(np.asarray(x), dtype=dt)
    both = concatenate(batch, _mutate(tables, how))
    n = np.asarray(batch["obs"]).shape[0]
    leaves, pre = [], []

    def net(layers, x):
        for w, b, act in layers:
            w, b = t(w).requires_grad_(), t(b).requires_grad_()
            leaves.extend([w, b])
            z = x @ w.T + b
            pre.append(z.detach().numpy())
            x = R._activate(torch, z, act)
        return x

    x = t(both["obs"])
    if p.obs_mean is not None:      # the mirror was taken on the RAW row
        x = torch.clamp((x - t(p.obs_mean)) * t(p.inv_std), -p.clip, p.clip)
    mu, v = net(p.actor, x), net(p.critic, x)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    z = (t(both["action"]) - mu) / torch.exp(log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    old_logp, adv, ret = t(both["old_logp"]), t(both["adv"]), t(both["returns"])
    r = torch.exp(logp - old_logp)
    surr = torch.min(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    l_v = (v - ret) ** 2
    if value_clip:
        v_old = t(both["old_value"])
        l_v = torch.max(l_v, (v_old + torch.clamp(v - v_old, -clip, clip) - ret) ** 2)
    samples = n if how == "mean_over_b" else 2 * n
    l_v = 0.5 * (l_v[:n].sum() if how == "twin_critic_dead" else l_v.sum()) / samples
    entropy = (log_std + 0.5 + HALF_LOG_2PI).sum()
    loss = -surr.sum() / samples + value_coef * l_v - entropy_coef * entropy
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = np.concatenate([(torch.zeros_like(leaf) if g is None else g).numpy().reshape(-1) for g, leaf in zip(grads, leaves)])
    lo, hi = t(1.0) - t(clip), t(1.0) + t(clip)
    clipped = ((r > hi) | (r < lo)).to(dt).mean()
    dlogp = old_logp - logp
    stats = np.array([surr.sum().item() / samples, l_v.item(), entropy.item(), dlogp.sum().item() / samples, clipped.item(),
                      float((grad.astype(np.float64) ** 2).sum()), 0.0, dlogp[n:].sum().item() / samples])
    return SimpleNamespace(grad=grad, stats=stats, logp=logp.detach().numpy(), value=v.detach().numpy(), pre=pre)


def grad_by_hand_dup(p, tables, batch, clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False):
    """the per-row lines of include/mocca.h in float64 numpy, once per KIND of sample with ib = 1 / (2 B) -> (the flat gradient, the
    twins' share of mean(old_logp - logp)): every weight's, bias's and log_std's gradient is the sum over both kinds"""
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    f = lambda k: np.asarray(batch[k], np.float64)
    n2 = 2 * f("obs").shape[0]
    ls = np.asarray(p.log_std, np.float64)
    s = np.exp(ls)
    adv, ret, olp = f("adv"), f("returns"), f("old_logp")
    parts, share = None, 0.0
    for twin in (False, True):
        x = R.normalise64(p, mirror(f("obs"), in_perm, in_sign) if twin else f("obs"))
        a = f("action")[:, act_perm] * act_sign.astype(np.float64) if twin else f("action")
        za, zc = [], []
        ya, yc = R._forward64(p.actor, x, za), R._forward64(p.critic, x, zc)
        z = (a - ya[-1]) / s
        logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
        r = np.exp(logp - olp)
        inactive = ((adv > 0) & (r > 1 + clip)) | ((adv < 0) & (r < 1 - clip))
        g = np.where(inactive, 0.0, -(adv * r) / n2)[:, None]
        d_mu, d_ls = g * (z / s), (g * (z * z - 1)).sum(0)
        v = yc[-1][:, 0]
        d_v = v - ret
        if value_clip:
            dd = v - f("old_value")
            e2 = f("old_value") + np.clip(dd, -clip, clip) - ret
            d_v = np.where((np.abs(dd) > clip) & (e2 * e2 > d_v * d_v), 0.0, d_v)
        d_v = (value_coef * d_v / n2)[:, None]
        new = R._backward64(p.actor, ya, za, d_mu) + R._backward64(p.critic, yc, zc, d_v) + [d_ls]
        parts = new if parts is None else [u + w for u, w in zip(parts, new)]
        if twin:
            share = float((olp - logp).sum() / n2)
    parts[-1] = parts[-1] - entropy_coef
    return np.concatenate([np.asarray(q).reshape(-1) for q in parts]), share


def make_storage_dup(p, tables, n_rows, seed=0, clip=CLIP):
    """Rollout storage of `n_rows` rows for policy `p` (make_policy above: close to symmetric) whose rows AND twins are away from every discrete tie, by construction and by
    selection on the CPU before anything is compared (candidates are drawn, the first n_rows that qualify enter):
    * the action is placed so that the twin's log-probability differs from the row's by a chosen amount (the difference is a quadratic in
      the action: one step along its gradient from between the two means), and old_logp so that the row's ratio r and the twin's ratio
      are each one of ppo_reference.RATIOS x (1 +- 0.01) -- both kinds of sample sit on a known side of both clip bounds and BOTH reach
      the actor; a twin that were far off-policy would be clipped away and a wrong twin could not be seen;
    * advantages of both signs with 0.1 <= |A| <= 2;
    * v_old, returns as ppo_reference.make_storage draws them for the row; rows whose TWIN has |v_t - v_old| within 0.05 of clip, or has
      clipped squared terms closer than 2e-3, are not taken;
    * nets with a relu: every f64 pre-activation of both passes has |z| > RELU_MARGIN.
    -> dict of float32 arrays obs [R, in_dim], action [R, A], old_logp, adv, returns, old_value [R]"""
    in_perm, in_sign, act_perm, act_sign = [np.asarray(x) for x in tables]
    rng = np.random.default_rng([seed, n_rows, 11])
    in_dim, act_dim = p.actor[0][0].shape[1], p.log_std.size
    n_c = 6 * n_rows + 256
    obs = rng.normal(0, 3.0, (n_c, in_dim)).astype(np.float32)
    m_obs = obs[:, in_perm] * in_sign.astype(np.float32)
    x1, x2 = R.normalise64(p, obs), R.normalise64(p, m_obs)
    pre = []
    mu1, mu2 = R._forward64(p.actor, x1, pre)[-1], R._forward64(p.actor, x2, pre)[-1]
    v1, v2 = R._forward64(p.critic, x1, pre)[-1][:, 0], R._forward64(p.critic, x2, pre)[-1][:, 0]
    ok = np.all([np.all(np.abs(z) > R.RELU_MARGIN, axis=1) for z in pre], axis=0) if any(
        act == "relu" for _, _, act in p.actor + p.critic) else np.ones(n_c, bool)
    ls = np.asarray(p.log_std, np.float64)
    s = np.exp(ls)
    sign = act_sign.astype(np.float64)
    # in the row's action frame the twin's Gaussian has mean m2[k] = sign[k] mu2[perm[k]] and deviation s2[k] = s[perm[k]]
    m2, s2 = mu2[:, act_perm] * sign, s[act_perm]
    diff = lambda a: -0.5 * (((a - m2) / s2) ** 2 - ((a - mu1) / s) ** 2).sum(-1)      # logp_twin - logp_row
    a0 = 0.5 * (mu1 + m2) + s * rng.normal(0, 1, mu1.shape)      # a rollout's noise, about the point between the two means
    pick = lambda: rng.choice(R.RATIOS, n_c) * (1 + rng.choice([-1.0, 1.0], n_c) * rng.uniform(0.002, 0.01, n_c))
    r_row, r_twin = pick(), pick()
    g = -(a0 - m2) / s2 ** 2 + (a0 - mu1) / s ** 2                                      # d diff / d a
    qa, qb, qc = 0.5 * (g * g * (1 / s ** 2 - 1 / s2 ** 2)).sum(-1), (g * g).sum(-1), diff(a0) - np.log(r_twin / r_row)
    disc = qb * qb - 4 * qa * qc
    ok &= (disc >= 0) & (qb > 0)
    step = np.where(ok, -2 * qc / (qb + np.sqrt(np.maximum(disc, 0))), 0.0)             # the root next to 0 of qa t^2 + qb t + qc
    action = (a0 + step[:, None] * g).astype(np.float32)
    a64 = action.astype(np.float64)
    z = (a64 - mu1) / s
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    old_logp = (logp - np.log(r_row)).astype(np.float32)
    got_row, got_twin = np.exp(logp - old_logp), np.exp(logp + diff(a64) - old_logp)
    for got, want in ((got_row, r_row), (got_twin, r_twin)):
        ok &= np.abs(got / want - 1) < 1e-3      # the float32 action and old_logp moved the ratio by rounding alone
    adv = (rng.choice([-1.0, 1.0], n_c) * rng.uniform(0.1, 2.0, n_c)).astype(np.float32)
    clipped = rng.random(n_c) < 0.5
    gap = np.where(clipped, rng.uniform(0.35, 0.8, n_c), rng.uniform(0.0, 0.08, n_c)) * rng.choice([-1.0, 1.0], n_c)
    old_value = (v1 - gap).astype(np.float32)
    returns = (v1 + rng.normal(0, 0.7, n_c)).astype(np.float32)
    vo, ret = old_value.astype(np.float64), returns.astype(np.float64)
    for v in (v1, v2):
        dd = v - vo
        vc = vo + np.clip(dd, -clip, clip)
        ok &= np.abs(np.abs(dd) - clip) > 0.05
        ok &= (np.abs(dd) < clip) | (np.abs((v - ret) ** 2 - (vc - ret) ** 2) > 2e-3)
    keep = np.flatnonzero(ok)[:n_rows]
    assert keep.size == n_rows, f"too few candidate rows: {int(ok.sum())} of {n_c} for {n_rows}"
    return {k: np.ascontiguousarray(v[keep]) for k, v in dict(obs=obs, action=action, old_logp=old_logp, adv=adv, returns=returns,
                                                              old_value=old_value).items()}
