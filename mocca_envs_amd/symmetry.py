"""On-device mirror-symmetry transforms for SymmetricRL-style trainers.

The reference only *publishes* index sets through `get_mirror_indices()` (env_locomotion.py:224-282, :761-840);
the trainers apply them in numpy on the host.  With observations living on the GPU the same transform is a
gather + sign flip on the device, so the learner's data never leaves HBM.

`MirrorTransform` serves the trainers that mirror DATA (duplicated samples, the auxiliary loss).  The symmetric-NETWORK policy,

    mean_sym(s)  = 1/2 ( f(n(s)) + M_a f(n(M_o s)) )            value_sym(s) = 1/2 ( V(n(s)) + V(n(M_o s)) ),

n the observation normalisation, runs in the policy kernel (csrc/mocca_policy.h: Symmetry): `mirror_tables` builds what
`policy.DevicePolicy(symmetry=)` and `mocca_set_policy_symmetry` take, `SymmetricGaussian` is the same function in torch, with gradients,
for the PPO update.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

HALF_LOG_2PI = 0.9189385332046727


def _table(dim, neg, right, left, what):
    neg, right, left = (np.asarray(list(x), np.int64).reshape(-1) for x in (neg, right, left))
    if right.size != left.size:
        raise ValueError(f"{what}: the right and left index sets differ in size")
    for idx in (neg, right, left):
        if idx.size and (idx.min() < 0 or idx.max() >= dim):
            raise ValueError(f"{what}: an index is outside 0 .. {dim - 1}")
    perm, sign = np.arange(dim, dtype=np.int32), np.ones(dim, np.float32)
    perm[right], perm[left] = left, right
    sign[neg] = -1.0
    return perm, sign


def mirror_tables(mirror_indices, obs_dim: int, act_dim: int, scan_points=None, depth_shape=None, history=None):
    """-> (in_perm int32 [in_dim], in_sign float32 [in_dim], act_perm int32 [act_dim], act_sign float32 [act_dim]) in `MirrorTransform`'s
    convention, (M x)[k] = sign[k] * x[perm[k]]: perm swaps the right and left sets, sign is -1 on the neg set.  `mirror_indices`: the six
    lists of `get_mirror_indices()`.  With `scan_points` [n, 2] (a perception pattern: x ahead, y to the left) the input is [obs | scan],
    in_dim = obs_dim + n: scan entry p maps to the point at (px, -py) with sign +1, a point with py == 0 to itself; a point whose reflection
    is not in the pattern (to 1e-6 m) is a ValueError.  With `depth_shape` (H, W) (a perception.DepthCamera in the robot's sagittal plane)
    an H x W depth image follows, [obs | scan | depth]: entry (j, i), at j * W + i of the block, maps to (j, W - 1 - i) with sign +1.  The
    With `history` = (columns, hist_act_dim, steps) (a history.History as the env resolved it) the block of `steps` pairs
    [obs[columns] | action] follows, [obs | scan | depth | hist]: in every pair, observation entry p (column columns[p]) maps to the
    position in `columns` of in_perm[columns[p]], with that column's sign -- a ValueError, naming the column, if the set of columns is not
    closed under the mirror --; the action entries map through act_perm / act_sign (`hist_act_dim` must be 0 or `act_dim`).  The
    tables are checked (check_tables)."""
    if isinstance(mirror_indices, dict) or len(mirror_indices) != 6:
        raise ValueError("mirror_indices must be the six lists (neg_obs, right_obs, left_obs, neg_act, right_act, left_act) of get_mirror_indices()")
    neg_obs, right_obs, left_obs, neg_act, right_act, left_act = mirror_indices
    in_perm, in_sign = _table(int(obs_dim), neg_obs, right_obs, left_obs, "observation")
    act_perm, act_sign = _table(int(act_dim), neg_act, right_act, left_act, "action")
    if scan_points is not None:
        pts = np.asarray(scan_points, np.float64)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("scan_points must be [n, 2]")
        image = pts * np.array([1.0, -1.0])
        d = np.abs(image[:, None, :] - pts[None, :, :]).max(-1)        # d[p][q]: how far the reflection of p is from q
        scan_perm = d.argmin(1)
        on_axis = pts[:, 1] == 0.0
        scan_perm[on_axis] = np.arange(len(pts))[on_axis]
        miss = np.flatnonzero(d[np.arange(len(pts)), scan_perm] > 1e-6)
        if miss.size:
            p = int(miss[0])
            raise ValueError(f"scan point {p} ({pts[p, 0]:g}, {pts[p, 1]:g}) has no reflection ({pts[p, 0]:g}, {-pts[p, 1]:g}) in the pattern")
        in_perm = np.concatenate([in_perm, (int(obs_dim) + scan_perm).astype(np.int32)])
        in_sign = np.concatenate([in_sign, np.ones(len(pts), np.float32)])
    if depth_shape is not None:
        if len(tuple(depth_shape)) != 2 or any(int(v) != v or int(v) < 1 for v in depth_shape):
            raise ValueError("depth_shape must be (height, width), both at least 1")
        H, W = (int(v) for v in depth_shape)
        flip = (np.arange(H)[:, None] * W + (W - 1 - np.arange(W))[None, :]).reshape(-1)
        in_perm = np.concatenate([in_perm, (len(in_perm) + flip).astype(np.int32)])
        in_sign = np.concatenate([in_sign, np.ones(H * W, np.float32)])
    if history is not None:
        cols, hist_act, steps = history
        cols, hist_act, steps = [int(c) for c in np.asarray(cols).reshape(-1)], int(hist_act), int(steps)
        if hist_act not in (0, int(act_dim)):
            raise ValueError(f"the history holds {hist_act} action entries per frame: the mirror needs 0 or the policy's act_dim ({int(act_dim)})")
        where = {c: p for p, c in enumerate(cols)}
        pair_perm, pair_sign = [], []
        for c in cols:
            if not 0 <= c < int(obs_dim):
                raise ValueError(f"history column {c} is outside 0 .. {int(obs_dim) - 1}")
            if int(in_perm[c]) not in where:
                raise ValueError(f"history column {c} mirrors to column {int(in_perm[c])}, which the history does not hold: "
                                 "the columns are not closed under the mirror")
            pair_perm.append(where[int(in_perm[c])])
            pair_sign.append(in_sign[c])
        if hist_act:
            pair_perm += [len(cols) + int(a) for a in act_perm]
            pair_sign += list(act_sign)
        pair_perm, width = np.asarray(pair_perm, np.int64), len(cols) + hist_act
        base = len(in_perm) + width * np.arange(steps)[:, None]
        in_perm = np.concatenate([in_perm, (base + pair_perm[None, :]).reshape(-1).astype(np.int32)])
        in_sign = np.concatenate([in_sign, np.tile(np.asarray(pair_sign, np.float32), steps)])
    return check_tables((in_perm, in_sign, act_perm, act_sign))


def check_tables(tables, in_dim=None, act_dim=None):
    """The rules of mirror tables (in_perm, in_sign, act_perm, act_sign), the ones mocca_set_policy_symmetry checks again: indices in range,
    perm[perm[k]] == k, sign[k] +1 or -1, sign[perm[k]] == sign[k] (so that M M = I); with `in_dim` / `act_dim`, the sizes.  -> the four
    arrays as int32 / float32; ValueError otherwise."""
    if tables is None or len(tables) != 4:
        raise ValueError("mirror tables are (in_perm, in_sign, act_perm, act_sign)")
    out = []
    for name, perm, sign, dim in (("in", tables[0], tables[1], in_dim), ("act", tables[2], tables[3], act_dim)):
        perm_i, sign = np.asarray(perm), np.array(sign, dtype=np.float32).reshape(-1)
        if perm_i.dtype.kind not in "iu":
            raise ValueError(f"{name}_perm must hold integers")
        perm_i = perm_i.reshape(-1).astype(np.int64)
        n = perm_i.size
        if n != sign.size or n < 1 or (dim is not None and n != int(dim)):
            raise ValueError(f"{name}_perm / {name}_sign must have {'one entry per feature' if dim is None else f'{int(dim)} entries'} each")
        if perm_i.min() < 0 or perm_i.max() >= n:
            raise ValueError(f"{name}_perm: an index is outside 0 .. {n - 1}")
        if not np.array_equal(perm_i[perm_i], np.arange(n)):
            raise ValueError(f"{name}_perm is not an involution (perm[perm[k]] != k)")
        if not np.all((sign == 1.0) | (sign == -1.0)):
            raise ValueError(f"{name}_sign must be +1 or -1")
        if not np.array_equal(sign[perm_i], sign):
            raise ValueError(f"{name}_sign differs across a swapped pair (M M must be the identity)")
        out += [perm_i.astype(np.int32), sign]
    return tuple(out)


class MirrorTransform:
    """obs' = M_obs obs, act' = M_act act where M swaps the right/left index sets and negates the `neg` set."""

    def __init__(self, mirror_indices: Tuple[Sequence[int], ...], obs_dim: int, act_dim: int, device=None):
        neg_obs, right_obs, left_obs, neg_act, right_act, left_act = [torch.as_tensor(list(x), dtype=torch.long)
                                                                      for x in mirror_indices]
        self.obs_perm, self.obs_sign = self._build(obs_dim, neg_obs, right_obs, left_obs, device)
        self.act_perm, self.act_sign = self._build(act_dim, neg_act, right_act, left_act, device)

    @staticmethod
    def _build(dim, neg, right, left, device):
        perm = torch.arange(dim)
        perm[right], perm[left] = left.clone(), right.clone()
        sign = torch.ones(dim)
        sign[neg] = -1.0
        return perm.to(device), sign.to(device)

    def obs(self, x: torch.Tensor) -> torch.Tensor:
        return x[..., self.obs_perm] * self.obs_sign

    def act(self, a: torch.Tensor) -> torch.Tensor:
        return a[..., self.act_perm] * self.act_sign


def mirror_loss(actor_mean, obs: torch.Tensor, transform: MirrorTransform) -> torch.Tensor:
    """SymmetricRL's mirror-symmetry loss, `(mirror(actor(mirror_obs)) - actor(obs)).pow(2).mean()`: the mean over rows AND actions of
    (f(x) - M_a f(M_o x))^2, both passes carrying gradient -- what mocca_ppo_grad_mirror adds to PPO's loss, times its coef.  `actor_mean`:
    obs [..., in_dim] -> the Gaussian's mean [..., act_dim] (the normalisation included, so that the mirror acts on the raw row);
    `transform` in `obs`'s dtype."""
    d = actor_mean(obs) - transform.act(actor_mean(transform.obs(obs)))
    return d.pow(2).mean()


def duplicate_minibatch(obs: torch.Tensor, action: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor, returns: torch.Tensor,
                        old_value: Optional[torch.Tensor], transform: MirrorTransform):
    """SymmetricRL's duplicated tuples: the B rows followed by their B mirror images -- (M_o obs, M_a action) with the rows' OWN old_logp,
    adv, returns and old_value (None stays None) -- as 2 B-row tensors, what mocca_ppo_grad_dup trains on without building them.  A
    mirror only permutes and flips signs: the twins' entries are exact.  `transform` in `obs`'s dtype, `obs` RAW (un-normalised).
    -> (obs, action, old_logp, adv, returns, old_value)"""
    twice = lambda x: None if x is None else torch.cat([x, x], 0)
    return (torch.cat([obs, transform.obs(obs)], 0), torch.cat([action, transform.act(action)], 0), twice(old_logp), twice(adv),
            twice(returns), twice(old_value))


class SymmetricGaussian(torch.nn.Module):
    """The symmetric policy of `DevicePolicy(symmetry=)` / the policy kernel in torch, with gradients: what the PPO update differentiates
    while the rollout acts on the device.  Built over the trainer's own `actor_seq`, `critic_seq` (torch.nn.Sequential) and `log_std`
    (a Parameter [act_dim]) -- shared, not copied -- and `mirror_tables`' four arrays.  The mirror acts on the raw row, ahead of the
    normalisation; the statistics are passed per call (they are running statistics, not parameters)."""

    def __init__(self, actor_seq, critic_seq, log_std, tables):
        super().__init__()
        in_perm, in_sign, act_perm, act_sign = check_tables(tables)
        self.actor, self.critic, self.log_std = actor_seq, critic_seq, log_std
        self.register_buffer("in_perm", torch.from_numpy(in_perm.astype(np.int64)), persistent=False)
        self.register_buffer("act_perm", torch.from_numpy(act_perm.astype(np.int64)), persistent=False)
        self.register_buffer("in_sign", torch.from_numpy(in_sign), persistent=False)
        self.register_buffer("act_sign", torch.from_numpy(act_sign), persistent=False)

    def forward(self, obs, obs_mean=None, inv_std=None, clip=10.0):
        """-> (mean [..., act_dim], log_std_sym [act_dim], value [...]); obs [..., >= in_dim], obs_mean / inv_std [in_dim] or None"""
        x = obs[..., :self.in_perm.numel()]
        xm = x[..., self.in_perm] * self.in_sign.to(x.dtype)

        def n(v):
            return v if obs_mean is None else ((v - obs_mean) * inv_std).clamp(-clip, clip)

        act_sign = self.act_sign.to(x.dtype)
        mean = 0.5 * (self.actor(n(x)) + self.actor(n(xm))[..., self.act_perm] * act_sign)
        value = 0.5 * (self.critic(n(x)) + self.critic(n(xm)))[..., 0]
        log_std = 0.5 * (self.log_std + self.log_std[self.act_perm])
        return mean, log_std, value

    def evaluate_actions(self, obs, action, obs_mean=None, inv_std=None, clip=10.0):
        """-> (logp [...], entropy [...], value [...]) of `action` under the symmetric Gaussian"""
        mean, log_std, value = self.forward(obs, obs_mean, inv_std, clip)
        e = (action - mean) * torch.exp(-log_std)
        logp = (-0.5 * e * e - log_std - HALF_LOG_2PI).sum(-1)
        entropy = (0.5 + HALF_LOG_2PI + log_std).sum(-1).expand_as(logp)
        return logp, entropy, value
