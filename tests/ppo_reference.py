"""Checker for mocca_ppo_grad (include/mocca.h; mocca_envs_amd/csrc/mocca_ppo.hip): PPO's minibatch loss stated in torch on the CPU and
differentiated by autograd -- at float64 the reference, at float32 the yardstick --, the same gradient from hand-written per-row formulas
(what the kernel's head stage and backward compute), a seeded factory of policies and of rollout storage whose rows sit away from every
discrete tie of the loss, and the parity rule.

A policy here is policy_reference's SimpleNamespace(actor, critic, log_std, obs_mean, inv_std, clip)."""
from types import SimpleNamespace

import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
CLIP = 0.2
NETS = {    # name: (in_dim, act_dim, hidden widths, the hidden layers' activations); the critic has the actor's hidden layers
    "tiny": (5, 3, [16], ["tanh"]),
    "ppo": (52, 21, [256, 256], ["tanh", "tanh"]),
    "mixed": (65, 21, [64, 32, 16], ["relu", "softsign", "tanh"]),
    "wide": (336, 21, [256], ["tanh"]),
    "single": (7, 2, [], []),
}
RATIOS = (0.7, 0.9, 1.1, 1.3)       # r* = one of these x (1 +- 0.01): both sides of both clip bounds at clip = 0.2, never on one
RELU_MARGIN = 1e-4                  # rows of relu nets keep every f64 pre-activation this far from 0


def make_policy(name, norm=True, seed=0, acts=None):
    """Weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2), log_std ~ U(-1, 0.2); statistics: mean ~ N(0, 1), var ~ U(0.05, 4), clip 5"""
    in_dim, act_dim, hidden, hidden_acts = NETS[name]
    hidden_acts = list(hidden_acts if acts is None else acts)
    rng = np.random.default_rng([seed, sorted(NETS).index(name)])

    def net(out):
        dims, layers = [in_dim] + list(hidden) + [out], []
        for i, act in enumerate(hidden_acts + ["identity"]):
            layers.append((rng.normal(0, 1 / np.sqrt(dims[i]), (dims[i + 1], dims[i])).astype(np.float32),
                           rng.normal(0, 0.1, dims[i + 1]).astype(np.float32), act))
        return layers

    p = SimpleNamespace(actor=net(act_dim), critic=net(1), log_std=rng.uniform(-1.0, 0.2, act_dim).astype(np.float32), obs_mean=None,
                        inv_std=None, clip=5.0)
    mean, var = rng.normal(0, 1, in_dim).astype(np.float32), rng.uniform(0.05, 4.0, in_dim).astype(np.float32)
    if norm:
        p.obs_mean, p.inv_std = mean, (np.float32(1) / np.sqrt(var + np.float32(1e-8))).astype(np.float32)
    return p


def flat_params(p):
    """mocca_update_policy's order without the statistics: per layer W then b, actor then critic, then log_std"""
    return np.concatenate([x.reshape(-1) for net in (p.actor, p.critic) for w, b, _ in net for x in (w, b)] + [p.log_std]).astype(np.float32)


def tensor_slices(p):
    """[(start, stop)] of every parameter tensor in flat_params' order"""
    out, pos = [], 0
    for size in [x.size for net in (p.actor, p.critic) for w, b, _ in net for x in (w, b)] + [p.log_std.size]:
        out.append((pos, pos + size))
        pos += size
    return out


def critic_slices(p):
    """[(start, stop)] of the critic's parameter tensors in flat_params' order"""
    return tensor_slices(p)[2 * len(p.actor):2 * (len(p.actor) + len(p.critic))]


def normalise64(p, x):
    x = np.asarray(x, np.float64)
    if p.obs_mean is None:
        return x
    return np.clip((x - np.asarray(p.obs_mean, np.float64)) * np.asarray(p.inv_std, np.float64), -p.clip, p.clip)


def _activate(torch, x, act):
    return {"identity": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "softsign": lambda v: v / (1 + v.abs())}[act](x)


def loss_autograd(p, batch, dtype="float64", clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False):
    """The loss of include/mocca.h mocca_ppo_grad in torch on the CPU at `dtype`, differentiated by autograd.  `batch`: dict of numpy arrays
    obs [B, in_dim] (raw), action [B, A], old_logp, adv, returns, old_value [B] -- the minibatch's rows, already gathered.
    -> SimpleNamespace(grad flat [n_head], stats [6], logp [B], value [B], pre: every layer's pre-activations)"""
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
            x = _activate(torch, z, act)
        return x

    x = t(batch["obs"])
    if p.obs_mean is not None:
        x = torch.clamp((x - t(p.obs_mean)) * t(p.inv_std), -p.clip, p.clip)
    mu, v = net(p.actor, x), net(p.critic, x)[:, 0]
    log_std = t(p.log_std).requires_grad_()
    leaves.append(log_std)
    z = (t(batch["action"]) - mu) / torch.exp(log_std)
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
    loss = -surr.mean() + value_coef * l_v - entropy_coef * entropy
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grad = np.concatenate([(torch.zeros_like(leaf) if g is None else g).numpy().reshape(-1) for g, leaf in zip(grads, leaves)])
    lo, hi = t(1.0) - t(clip), t(1.0) + t(clip)
    clipped = ((r > hi) | (r < lo)).to(dt).mean()
    stats = np.array([surr.mean().item(), l_v.item(), entropy.item(), (old_logp - logp).mean().item(), clipped.item(),
                      float((grad.astype(np.float64) ** 2).sum())])
    return SimpleNamespace(grad=grad, stats=stats, logp=logp.detach().numpy(), value=v.detach().numpy(), pre=pre)


def _slope(x, act):
    """the activation's derivative from its INPUT x, in the header's forms: sech^2 x = 4 e / (1 + e)^2 with e = exp(-2 |x|); 1 / (1 + |x|)^2"""
    e = np.exp(-2 * np.abs(x))
    return {"identity": np.ones_like(x), "relu": (x > 0).astype(x.dtype), "tanh": 4 * e / (1 + e) ** 2, "softsign": 1 / (1 + np.abs(x)) ** 2}[act]


def _forward64(layers, x, pre=None):
    """-> every layer's output, the input first; `pre`: a list that receives the pre-activations"""
    ys = [x]
    for w, b, act in layers:
        z = ys[-1] @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if pre is not None:
            pre.append(z)
        ys.append({"identity": z, "relu": np.maximum(z, 0), "tanh": np.tanh(z), "softsign": z / (1 + np.abs(z))}[act])
    return ys


def _backward64(layers, ys, zs, d_head):
    """-> [dW, db per layer] from dL/dhead [B, out]: dZ = dA * act'(x), dW = dZ^T A_prev, db = column sums, dA_prev = dZ W"""
    out, d_a = [], d_head
    for (w, _, act), z, y_prev in zip(layers[::-1], zs[::-1], ys[-2::-1]):
        d_z = d_a * _slope(z, act)
        out = [d_z.T @ y_prev, d_z.sum(0)] + out
        d_a = d_z @ np.asarray(w, np.float64)
    return out


def grad_by_hand(p, batch, clip=CLIP, value_coef=0.5, entropy_coef=0.0, value_clip=False):
    """the per-row formulas of include/mocca.h in float64 numpy -> the flat gradient"""
    f = lambda k: np.asarray(batch[k], np.float64)
    x = f("obs")
    if p.obs_mean is not None:
        x = np.clip((x - np.asarray(p.obs_mean, np.float64)) * np.asarray(p.inv_std, np.float64), -p.clip, p.clip)
    n = x.shape[0]
    za, zc = [], []
    ya, yc = _forward64(p.actor, x, za), _forward64(p.critic, x, zc)
    ls = np.asarray(p.log_std, np.float64)
    s = np.exp(ls)
    z = (f("action") - ya[-1]) / s
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    r, adv = np.exp(logp - f("old_logp")), f("adv")
    inactive = ((adv > 0) & (r > 1 + clip)) | ((adv < 0) & (r < 1 - clip))
    g = np.where(inactive, 0.0, -(adv * r) / n)[:, None]
    d_mu, d_ls = g * (z / s), (g * (z * z - 1)).sum(0) - entropy_coef
    v, ret = yc[-1][:, 0], f("returns")
    d_v = v - ret
    if value_clip:
        dd = v - f("old_value")
        e2 = f("old_value") + np.clip(dd, -clip, clip) - ret
        d_v = np.where((np.abs(dd) > clip) & (e2 * e2 > d_v * d_v), 0.0, d_v)      # the clamp passes: the same function of v, the unclipped term
    d_v = (value_coef * d_v / n)[:, None]
    parts = _backward64(p.actor, ya, za, d_mu) + _backward64(p.critic, yc, zc, d_v) + [d_ls]
    return np.concatenate([np.asarray(q).reshape(-1) for q in parts])


def make_storage(p, n_rows, seed=0, clip=CLIP):
    """Rollout storage of `n_rows` rows for policy `p`, away from every discrete tie BY CONSTRUCTION (no row is left out afterwards):
    * old_logp = logp_f64 - log(r*), r* one of RATIOS x (1 +- 0.01): the ratio sits on a known side of both clip bounds;
    * advantages of both signs with 0.1 <= |A| <= 2;
    * v_old with |v - v_old| < 0.1 (the clamp passes: both squared terms are the same function of v) or > 0.3 (it clips), and for the
      clipped rows returns drawn so that the two squared terms differ by more than 1e-3;
    * nets with a relu: only candidate rows whose f64 pre-activations ALL have |z| > RELU_MARGIN enter the storage (selected here, on the
      CPU, before anything is compared).
    -> dict of float32 arrays obs [R, in_dim], action [R, A], old_logp, adv, returns, old_value [R]"""
    rng = np.random.default_rng([seed, n_rows, 5])
    in_dim, act_dim = p.actor[0][0].shape[1], p.log_std.size
    relu = any(act == "relu" for _, _, act in p.actor + p.critic)
    obs = rng.normal(0, 3.0, (2 * n_rows + 64 if relu else n_rows, in_dim)).astype(np.float32)
    zero = np.zeros(obs.shape[0])
    probe = dict(obs=obs, action=np.zeros((obs.shape[0], act_dim)), old_logp=zero, adv=zero, returns=zero, old_value=zero)
    if relu:
        pre = loss_autograd(p, probe).pre
        keep = np.all([np.all(np.abs(z) > RELU_MARGIN, axis=1) for z in pre], axis=0)
        obs = obs[keep][:n_rows]
        assert obs.shape[0] == n_rows, "too few candidate rows"
        probe = {k: v[:n_rows] for k, v in probe.items()}
        probe["obs"] = obs
    x = np.asarray(obs, np.float64)
    if p.obs_mean is not None:
        x = np.clip((x - np.asarray(p.obs_mean, np.float64)) * np.asarray(p.inv_std, np.float64), -p.clip, p.clip)
    mu64 = _forward64(p.actor, x)[-1]
    action = (mu64 + np.exp(np.asarray(p.log_std, np.float64)) * rng.normal(0, 1, mu64.shape)).astype(np.float32)
    probe["action"] = action
    fwd = loss_autograd(p, probe)     # logp of the float32 actions, value
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


def gather(storage, idx=None, n=None):
    """the minibatch's rows: storage[idx], or the first n rows"""
    return {k: (v[:n] if idx is None else v[np.asarray(idx)]) for k, v in storage.items()}


def tensor_errors(p, got, want64):
    """the parity rule's errors: per parameter tensor |got - f64| / max |f64 of that tensor| -> one pooled array"""
    out = []
    for a, b in tensor_slices(p):
        scale = np.abs(want64[a:b]).max()
        out.append(np.abs(np.asarray(got[a:b], np.float64) - want64[a:b]) / (scale if scale > 0 else 1.0))
    return np.concatenate(out)


def triple(err):
    return [float(np.median(err)), float(np.percentile(err, 99)), float(err.max())]


def within(got, yard, factor=3.0):
    return all(got[i] <= factor * yard[i] for i in range(3))


def stat_units(got, want64):
    """errors of stats[0..3] in units of 1e-6 (1 + |x|)"""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / (1e-6 * (1 + np.abs(want64)))
