"""The end of a PPO rollout: `ObsStats`, the running observation statistics both env surfaces take, and the argument checks of
`VecEnv.finish_rollout` / `VecEnv.update_obs_stats` (include/mocca.h mocca_gae / mocca_obs_stats); and the update that follows it:
`AdamState`, the optimiser's state on the device, and the argument checks of `VecEnv.ppo_grad` / `adam_step` / `ppo_update`.

The reference's trainers (SymmetricRL, ALLSTEPS: pytorch-a2c-ppo-acktr) normalise observations with VecNormalize's `ob_rms`, baselines'
RunningMeanStd: count, mean and variance per feature, merged batch by batch (Chan et al.).  An `ObsStats` holds them as ONE float64 tensor
`state` = [count, mean[dim], var[dim]]:

* `VecEnv.update_obs_stats(stats, rows)` / `TorchVecEnv.update_obs_stats` merge a whole rollout's rows on the device, two launches, and
  write float32 mean and 1 / sqrt(var + eps) where the caller says -- the tail of the flat tensor `update_policy` takes;
* `stats.update(rows)` is the same definition in numpy, for the single-env gym classes (and the tests).
"""
from __future__ import annotations

import numpy as np

MAX_DIM = 336            # csrc/mocca_rollout.h OBS_MAX_DIM = policy.MAX_IN
MAX_STEPS = 65536        # include/mocca.h mocca_gae
INITIAL_COUNT = 1e-4     # baselines' RunningMeanStd(epsilon=1e-4)


class ObsStats:
    def __init__(self, dim: int, device=None, eps: float = 1e-8):
        import torch
        self.dim, self.eps = int(dim), float(eps)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError(f"dim must be 1 .. {MAX_DIM}")
        if not (np.isfinite(self.eps) and self.eps >= 0.0):
            raise ValueError("eps must be finite and not negative")
        self.device = torch.device("cpu" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.state = torch.empty(1 + 2 * self.dim, dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self) -> None:
        """count 1e-4, mean 0, var 1"""
        import torch
        self.state.copy_(torch.from_numpy(initial_state(self.dim)))

    # views of the state tensor (on its device)
    @property
    def count(self):
        return self.state[0]

    @property
    def mean(self):
        return self.state[1:1 + self.dim]

    @property
    def var(self):
        return self.state[1 + self.dim:]

    def normalisation(self):
        """(mean, inv_std) as float32 numpy arrays: what `policy.DevicePolicy` and the policy kernel use"""
        return normalisation(self.state.cpu().numpy(), self.eps)

    def update(self, rows) -> None:
        """merge rows [..., >= dim] (numpy or tensor; the first dim entries of a row count) on the host, in float64"""
        import torch
        x = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        self.state.copy_(torch.from_numpy(merge(self.state.cpu().numpy(), x, self.dim)))


def initial_state(dim: int) -> np.ndarray:
    return np.concatenate([[INITIAL_COUNT], np.zeros(dim), np.ones(dim)])


def merge(state: np.ndarray, rows: np.ndarray, dim: int) -> np.ndarray:
    """the kernel's definition: batch moments of d = x - mean (shifted by the running mean), then Chan's merge, all in float64"""
    x = np.asarray(rows)
    if x.ndim == 0 or x.shape[-1] < dim:
        raise ValueError(f"rows must be [..., >= {dim}]")
    x = x.reshape(-1, x.shape[-1])[:, :dim].astype(np.float64)
    n = x.shape[0]
    if n < 1:
        raise ValueError("rows must hold at least one row")
    count, mean, var = state[0], state[1:1 + dim], state[1 + dim:]
    d = x - mean
    md = d.sum(0) / n
    bm, bv = mean + md, (d * d).sum(0) / n - md * md
    delta, tot = bm - mean, count + n
    return np.concatenate([[tot], mean + delta * n / tot, (var * count + bv * n + delta * delta * count * n / tot) / tot])


def normalisation(state: np.ndarray, eps: float):
    dim = (state.size - 1) // 2
    mean, var = state[1:1 + dim].astype(np.float32), state[1 + dim:].astype(np.float32)
    return mean, np.float32(1) / np.sqrt(var + np.float32(eps))


# ---- argument checks of VecEnv.finish_rollout / update_obs_stats: they need no device ----

def _storage(name, t, rows, n_envs, device):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous() \
            or tuple(t.shape) not in ((rows, n_envs), (rows, n_envs, 1)):
        raise ValueError(f"{name} must be a contiguous float32 [{rows}, {n_envs}] or [{rows}, {n_envs}, 1] tensor on the env's device")


def gae_args(n_envs, device, reward, value, masks, bad_masks, gamma, lam, reward_scale, returns, adv, normalise, adv_eps):
    """check the tensors and numbers of finish_rollout -> T; ValueError otherwise"""
    import torch
    if not isinstance(reward, torch.Tensor) or reward.dim() not in (2, 3):
        raise ValueError(f"reward must be a float32 [T, {n_envs}] or [T, {n_envs}, 1] tensor")
    T = int(reward.shape[0])
    if not 1 <= T <= MAX_STEPS:
        raise ValueError(f"the rollout must have 1 .. {MAX_STEPS} steps")
    _storage("reward", reward, T, n_envs, device)
    for name, t in (("value", value), ("masks", masks), ("bad_masks", bad_masks)):
        _storage(name, t, T + 1, n_envs, device)
    for name, t in (("returns", returns), ("adv", adv)):
        if t is not None:
            _storage(name, t, T, n_envs, device)
    if not all(np.isfinite(float(x)) for x in (gamma, lam, reward_scale)):
        raise ValueError("gamma, lam and reward_scale must be finite")
    if not (np.isfinite(float(adv_eps)) and float(adv_eps) >= 0.0):
        raise ValueError("adv_eps must be finite and not negative")
    if normalise and T * n_envs < 2:
        raise ValueError("normalise needs at least two advantages")
    return T


def _row_stride(n: int, stride: int, cols: int):
    """THE row-stride rule, for `n` rows of `cols` floats, `stride` floats apart -> the stride to hand to a kernel, None where rows
    overlap.  One row's stride never indexes anything, but the C side checks stride >= width: it is the row's own length at least."""
    if n == 1:
        return max(stride, cols)
    return stride if stride >= cols else None


def rows_2d(rows, dim: int):
    """rows [..., >= dim] with contiguous last dimension and one stride between consecutive rows -> (n_rows, row_stride in floats)"""
    import torch
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() < 1 or rows.shape[-1] < dim \
            or (rows.shape[-1] > 1 and rows.stride(-1) != 1):
        raise ValueError(f"rows must be a float32 [..., >= {dim}] tensor with a contiguous last dimension")
    lead = [(int(n), int(s)) for n, s in zip(rows.shape[:-1], rows.stride()[:-1]) if n != 1]
    if any(n == 0 for n, _ in lead):
        raise ValueError("rows must hold at least one row")
    for (n0, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != n1 * s1:
            raise ValueError("rows must have one uniform stride between consecutive rows (a slice of contiguous storage along the first axis will do)")
    n_rows = 1
    for n, _ in lead:
        n_rows *= n
    stride = _row_stride(n_rows, lead[-1][1] if lead else 0, int(rows.shape[-1]))
    if stride is None:
        raise ValueError(f"the row stride ({lead[-1][1]}) is smaller than the rows ({rows.shape[-1]}): they overlap")
    return n_rows, stride


def row_view(name: str, t, width: int, n_rows, device) -> int:
    """THE rule for "a float32 [n, >= width] tensor on `device` with contiguous rows" (a view of wider storage will do), for every call
    that hands such rows to a kernel: two dimensions, `n_rows` rows (None: any n >= 1), stride(1) == 1 unless there is one column, no
    overlapping rows -> the row stride in floats (_row_stride).  `name`: what the ValueError calls the tensor."""
    import torch
    if isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype == torch.float32 and t.device == device:
        (n, cols), (s0, s1) = t.shape, t.stride()
        stride = _row_stride(n, s0, cols)
        if (n == n_rows if n_rows else n >= 1) and cols >= width and (cols <= 1 or s1 == 1) and stride is not None:
            return stride
    raise ValueError(f"{name} must be a float32 [{'n_envs' if n_rows else 'n'}, >= {width}] tensor on the env's device with contiguous rows")


MAX_MINIBATCH = 1 << 22   # include/mocca.h mocca_ppo_grad
MAX_MINIBATCH_SYM = 1 << 21   # mocca_ppo_grad_sym: two scratch rows per minibatch row


def ppo_args(policy, device, obs, action, old_logp, adv, returns, idx, old_value, clip, value_coef, entropy_coef, value_clip, grad, stats,
             symmetric=False):
    """check the tensors and numbers of ppo_grad -> (R rollout rows, obs row stride, B minibatch rows); ValueError otherwise.  `symmetric`:
    the call is mocca_ppo_grad_sym, whose minibatch holds at most MAX_MINIBATCH_SYM rows"""
    import torch
    if not isinstance(obs, torch.Tensor) or obs.device != device:
        raise ValueError("obs must be a float32 tensor on the env's device")
    n_rows, stride = rows_2d(obs, policy.in_dim)
    a = policy.act_dim
    if not isinstance(action, torch.Tensor) or action.dtype != torch.float32 or action.device != device or not action.is_contiguous() \
            or action.dim() < 1 or action.shape[-1] != a or action.numel() != n_rows * a:
        raise ValueError(f"action must be a contiguous float32 [..., {a}] tensor of {n_rows} rows on the env's device")
    for name, t in (("old_logp", old_logp), ("adv", adv), ("returns", returns), ("old_value", old_value)):
        if t is None and name == "old_value" and not value_clip:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or t.numel() != n_rows:
            raise ValueError(f"{name} must be a contiguous float32 tensor of {n_rows} elements (one per row of obs) on the env's device")
    if idx is None:
        n_batch = n_rows
    else:
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.device != device or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError("idx must be a contiguous int64 [B] tensor on the env's device (a chunk of torch.randperm)")
        n_batch = int(idx.numel())
    most = MAX_MINIBATCH_SYM if symmetric else MAX_MINIBATCH
    if not 1 <= n_batch <= most:
        raise ValueError(f"the minibatch must have 1 .. {most} rows")
    for name, x in (("clip", clip), ("value_coef", value_coef), ("entropy_coef", entropy_coef)):
        if not (np.isfinite(float(x)) and float(x) >= 0.0):
            raise ValueError(f"{name} must be finite and not negative")
    stats_out("grad", grad, policy.n_head(), device)
    stats_out("stats", stats, 8, device)
    return n_rows, stride, n_batch


def distill_args(policy, device, obs, target, value_target, idx, distill_coef, value_coef, grad, stats):
    """check the tensors and numbers of distill_grad -> (R stored rows, obs row stride, B minibatch rows); ValueError otherwise"""
    import torch
    if not isinstance(obs, torch.Tensor) or obs.device != device:
        raise ValueError("obs must be a float32 tensor on the env's device")
    n_rows, stride = rows_2d(obs, policy.in_dim)
    a = policy.act_dim
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or target.device != device or not target.is_contiguous() \
            or target.dim() < 1 or target.shape[-1] != a or target.numel() != n_rows * a:
        raise ValueError(f"target must be a contiguous float32 [..., {a}] tensor of {n_rows} rows on the env's device")
    t = value_target
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous()
                          or t.numel() != n_rows):
        raise ValueError(f"value_target must be a contiguous float32 tensor of {n_rows} elements (one per row of obs) on the env's device")
    if idx is None:
        n_batch = n_rows
    else:
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.device != device or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError("idx must be a contiguous int64 [B] tensor on the env's device (a chunk of torch.randperm)")
        n_batch = int(idx.numel())
    if not 1 <= n_batch <= MAX_MINIBATCH:
        raise ValueError(f"the minibatch must have 1 .. {MAX_MINIBATCH} rows")
    for name, x in (("distill_coef", distill_coef), ("value_coef", value_coef)):
        if not (np.isfinite(float(x)) and float(x) >= 0.0):
            raise ValueError(f"{name} must be finite and not negative")
    stats_out("grad", grad, policy.n_head(), device)
    stats_out("stats", stats, 8, device)
    return n_rows, stride, n_batch


class AdamState:
    """Adam's state for the flat parameter tensor of `update_policy`, on the device (include/mocca.h mocca_adam_step): `moments` float32
    [2, n_head] -- m, then v -- and `clock` float64 [4] = {t, beta1^t, beta2^t, skipped steps}.  `n_head`: `DevicePolicy.n_head()`."""

    def __init__(self, n_head: int, device):
        import torch
        self.n_head = int(n_head)
        if self.n_head < 1:
            raise ValueError("n_head must be at least 1")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.moments = torch.empty(2, self.n_head, dtype=torch.float32, device=self.device)
        self.clock = torch.empty(4, dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self) -> None:
        """moments 0, clock {0, 1, 1, 0}"""
        import torch
        self.moments.zero_()
        self.clock.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64))

    def state_dict(self) -> dict:
        """copies on the host, for a checkpoint"""
        return {"moments": self.moments.detach().cpu().clone(), "clock": self.clock.detach().cpu().clone()}

    def load_state_dict(self, d: dict) -> None:
        import torch
        m, c = torch.as_tensor(d["moments"]), torch.as_tensor(d["clock"])
        if tuple(m.shape) != (2, self.n_head) or tuple(c.shape) != (4,):
            raise ValueError(f"the state holds moments [2, {self.n_head}] and clock [4]")
        self.moments.copy_(m.to(torch.float32))
        self.clock.copy_(c.to(torch.float64))


def adam_args(policy, device, params, grad, state, n_params, lr, betas, eps, max_grad_norm):
    """check the tensors and numbers of adam_step (`grad` None: ppo_update, which owns its gradient) -> n_params; ValueError otherwise"""
    import torch
    n_head = policy.n_head()
    n_tail = policy.n_tail() if hasattr(policy, "n_tail") else 2 * policy.in_dim   # an asymmetric policy: + the critic's statistics
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.device != device or params.dim() != 1 \
            or not params.is_contiguous() or params.numel() not in (n_head, n_head + n_tail):
        raise ValueError(f"params must be a contiguous float32 [{n_head}] or [{n_head + n_tail}] tensor on the env's device "
                         "(DevicePolicy.flat_params()'s order); it is updated in place")
    n_params = n_head if n_params is None else int(n_params)
    if not 1 <= n_params <= n_head:
        raise ValueError(f"n_params must be 1 .. {n_head}")
    if grad is not None and (not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 or grad.device != device or grad.dim() != 1
                             or not grad.is_contiguous() or grad.numel() < n_params):
        raise ValueError(f"grad must be a contiguous float32 tensor of at least {n_params} elements on the env's device")
    if not isinstance(state, AdamState) or state.n_head != n_head or state.device != device:
        raise ValueError(f"state must be an AdamState({n_head}) on the env's device")
    if not (np.isfinite(float(lr)) and float(lr) >= 0.0 and np.isfinite(float(eps)) and float(eps) >= 0.0):
        raise ValueError("lr and eps must be finite and not negative")
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError("betas must be two numbers in [0, 1)")
    if not float(max_grad_norm) >= 0.0:
        raise ValueError("max_grad_norm must not be NaN or negative (0: no clip)")
    return n_params


def update_args(n_rows, minibatch_rows, epochs, seed, stats, device, symmetric=False):
    """check ppo_update's own numbers for R = n_rows rollout rows -> M minibatches per epoch; ValueError otherwise"""
    most = MAX_MINIBATCH_SYM if symmetric else MAX_MINIBATCH
    if not 1 <= n_rows <= most:
        raise ValueError(f"the rollout must have 1 .. {most} rows")
    if not 1 <= int(minibatch_rows) <= n_rows:
        raise ValueError(f"minibatch_rows must be 1 .. {n_rows}")
    if int(epochs) < 1:
        raise ValueError("epochs must be at least 1")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be 0 .. 2^64 - 1")
    per_epoch = n_rows // int(minibatch_rows)
    stats_out("stats", stats, int(epochs) * per_epoch * 8, device)
    return per_epoch


def stats_out(name, t, dim, device):
    import torch
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or t.numel() != dim or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 tensor of {dim} elements on the env's device")
