"""Checker for the mirror-symmetric device policy (csrc/mocca_policy.h: Symmetry), built on policy_reference: an independent numpy float64
statement of

    mean_sym(s) = 1/2 ( f(n(s)) + M_a f(n(M_o s)) )        value_sym(s) = 1/2 ( V(n(s)) + V(n(M_o s)) )

with (M x)[k] = sign[k] * x[perm[k]] and n the observation normalisation, its float32 yardstick, seeded random mirror tables, and mutations --
definitions that differ from the right one the way a kernel bug would.  Tables are (in_perm, in_sign, act_perm, act_sign)."""
from types import SimpleNamespace

import numpy as np

import policy_reference as R
from policy_reference import error_units, net64, normalise64, triple  # noqa: F401  (re-exported for the tests)

MUTATIONS = ("no_sign", "no_perm", "mirror_after_norm", "no_half")


def random_table(dim, seed):
    """A random signed involution of `dim` entries: about a third of them in swapped pairs (half of the pairs negated), the rest fixed
    points (half of them negated).  -> (perm int32, sign float32)"""
    rng = np.random.default_rng([seed, dim, 991])
    idx = rng.permutation(dim)
    n_pairs = max(dim // 3, 1 if dim >= 2 else 0)
    pairs, fixed = idx[:2 * n_pairs].reshape(-1, 2), idx[2 * n_pairs:]
    perm, sign = np.arange(dim, dtype=np.int32), np.ones(dim, np.float32)
    perm[pairs[:, 0]], perm[pairs[:, 1]] = pairs[:, 1], pairs[:, 0]
    sign[pairs[:(n_pairs + 1) // 2].reshape(-1)] = -1.0
    sign[fixed[:(len(fixed) + 1) // 2]] = -1.0
    return perm, sign


def random_tables(dim, seed, act_dim=None):
    """`random_table(dim, seed)`; with `act_dim`, the four tables of a policy dim -> act_dim"""
    if act_dim is None:
        return random_table(dim, seed)
    return random_table(dim, seed) + random_table(act_dim, seed + 1)


def mirror(x, perm, sign):
    """(M x)[k] = sign[k] * x[perm[k]] in x's own dtype (exact in any float format)"""
    x = np.asarray(x)
    return np.ascontiguousarray(x[..., np.asarray(perm)] * np.asarray(sign).astype(x.dtype))    # (a gather along the last axis may come out transposed)


def _combine(p, tables, x, normalise, net, how, f):
    in_perm, in_sign, act_perm, act_sign = tables
    if how == "no_sign":
        in_sign, act_sign = np.ones_like(in_sign), np.ones_like(act_sign)
    elif how == "no_perm":
        in_perm, act_perm = np.arange(len(in_perm)), np.arange(len(act_perm))
    elif how not in (None, "mirror_after_norm", "no_half"):
        raise ValueError(how)
    z = normalise(p, x)
    zm = mirror(z, in_perm, in_sign) if how == "mirror_after_norm" else normalise(p, mirror(x, in_perm, in_sign))
    half = f(1.0 if how == "no_half" else 0.5)
    mean = half * (net(p.actor, z) + mirror(net(p.actor, zm), act_perm, act_sign))
    value = half * (net(p.critic, z)[..., 0] + net(p.critic, zm)[..., 0])
    return mean, value


def sym_forward64(p, tables, x, how=None):
    """-> (mean [B, A], value [B]) in float64: the definition, from policy_reference's normalise64 / net64.  `how`: one of MUTATIONS."""
    return _combine(p, tables, np.asarray(x, np.float64)[..., :len(tables[0])], normalise64, net64, how, np.float64)


def sym_torch32(p, tables, x):
    """the same from policy_reference.torch32 (torch CPU float32 nets on the row as given and on the mirrored row), combined in float32:
    the yardstick of the rounding error"""
    in_perm, in_sign, act_perm, act_sign = tables
    x = np.asarray(x, np.float32)[..., :len(in_perm)]
    (m, v), (mm, vm) = R.torch32(p, x), R.torch32(p, mirror(x, in_perm, in_sign))
    return np.float32(0.5) * (m + mirror(mm, act_perm, act_sign)), np.float32(0.5) * (v + vm)


def log_std_sym(p, tables, dtype=np.float64):
    """1/2 (log_std[j] + log_std[act_perm[j]]) in `dtype` (float32: the kernel's own operation)"""
    ls = np.asarray(p.log_std, dtype)
    return dtype(0.5) * (ls + ls[np.asarray(tables[2])])


def device_policy(p, tables=None):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip, symmetry=tables)


def sequentials(p, dtype):
    """(actor, critic) of a policy_reference policy as torch.nn.Sequential in `dtype`, and log_std as a Parameter"""
    import torch
    from torch import nn
    acts = {"relu": nn.ReLU, "tanh": nn.Tanh, "softsign": nn.Softsign}

    def seq(layers):
        mods = []
        for w, b, act in layers:
            lin = nn.Linear(w.shape[1], w.shape[0]).to(dtype)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w).to(dtype))
                lin.bias.copy_(torch.from_numpy(b).to(dtype))
            mods.append(lin)
            if act != "identity":
                mods.append(acts[act]())
        return nn.Sequential(*mods)

    return seq(p.actor), seq(p.critic), nn.Parameter(torch.from_numpy(p.log_std).to(dtype))


def as_namespace(dp):
    """a DevicePolicy as the SimpleNamespace the reference functions take"""
    return SimpleNamespace(actor=dp.actor, critic=dp.critic, log_std=dp.log_std, obs_mean=dp.obs_mean, inv_std=dp.inv_std, clip=dp.clip)
