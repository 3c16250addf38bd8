"""The observation-action history of a `VecEnv`'s policy row (include/mocca.h mocca_set_history / mocca_history): what a trainer states once
so that the actor's row ends in the last few observations it read and the actions it then output -- the only place a feed-forward policy
can see a weak motor or a late command (`randomisation.Randomisation`).  The rule and the kernel: csrc/mocca_history.h."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from . import lib as _lib


@dataclass(frozen=True)
class History:
    """steps=K (1 .. 16) pairs [o_u[columns] | a_u], NEWEST FIRST, u = t - j * stride for j = 1 .. K (stride 1 .. 8): the observation the policy
    read j * stride steps ago and the action it then output; a pair the episode has not lived yet, or whose call was skipped, is zeros.
    columns: None (all of `obs`) or an ordered list of distinct observation columns (may be empty).  actions: True (the env's action width
    -- for a planner env with its base controller the 15-number plan), False / 0 (none), or a width of its own, at most 32.  The block has
    K * (len(columns) + actions) floats, at most 1024, and at least one.  The frames hold what the policy actually saw: with `obs_noise` the
    noisy observation; `envs.privileged` is not changed.  `attach_policy` keeps its width check: a row wider than the policy kernel's 336
    inputs is refused there -- Walker3DCustom (52 observations, 21 actions) takes steps=3 with all columns, 52 + 3 * 73 = 271."""
    steps: int
    stride: int = 1
    columns: Optional[Tuple[int, ...]] = None
    actions: Union[bool, int] = True

    def __post_init__(self):
        k, s = self.steps, self.stride
        if isinstance(k, bool) or int(k) != k or not (1 <= k <= _lib.HIST_MAX_STEPS):
            raise ValueError(f"steps must be a whole number 1 .. {_lib.HIST_MAX_STEPS} (got {k})")
        if isinstance(s, bool) or int(s) != s or not (1 <= s <= _lib.HIST_MAX_STRIDE):
            raise ValueError(f"stride must be a whole number 1 .. {_lib.HIST_MAX_STRIDE} (got {s})")
        cols = self.columns
        if cols is not None:
            c = np.asarray(list(cols))
            if c.size and (c.dtype.kind not in "iu" or c.ndim != 1):
                raise ValueError("columns must be None or a list of whole observation columns")
            cols = tuple(int(x) for x in c.reshape(-1))
            if any(x < 0 for x in cols):
                raise ValueError(f"column {min(cols)} is outside the observation")
            for x in cols:
                if cols.count(x) > 1:
                    raise ValueError(f"column {x} is repeated")
        a = self.actions
        if not isinstance(a, bool) and (int(a) != a or not (0 <= a <= _lib.HIST_MAX_ACT)):
            raise ValueError(f"actions must be True, False or a width 0 .. {_lib.HIST_MAX_ACT} (got {a})")
        object.__setattr__(self, "steps", int(k))
        object.__setattr__(self, "stride", int(s))
        object.__setattr__(self, "columns", cols)
        object.__setattr__(self, "actions", a if isinstance(a, bool) else int(a))

    def resolve(self, obs_dim: int, act_dim: int) -> Tuple[np.ndarray, int]:
        """-> (columns int32 [C], action width A) for an env of `obs_dim` observations and `act_dim` actions; ValueError as mocca_set_history
        refuses"""
        cols = np.arange(obs_dim, dtype=np.int32) if self.columns is None else np.asarray(self.columns, np.int32).reshape(-1)
        if cols.size and cols.max() >= obs_dim:
            raise ValueError(f"column {int(cols.max())} is outside 0 .. {obs_dim - 1}")
        a = int(act_dim) if self.actions is True else int(self.actions)
        if not (0 <= a <= _lib.HIST_MAX_ACT):
            raise ValueError(f"the action width {a} is outside 0 .. {_lib.HIST_MAX_ACT}")
        if cols.size + a == 0:
            raise ValueError("a frame needs at least one observation column or one action entry")
        if self.steps * (cols.size + a) > _lib.HIST_MAX_DIM:
            raise ValueError(f"the block has steps x (columns + actions) = {self.steps * (cols.size + a)} floats, at most {_lib.HIST_MAX_DIM}")
        return np.ascontiguousarray(cols), a

    def as_dict(self) -> dict:
        """plain numbers (what a saved policy file records)"""
        return dict(steps=self.steps, stride=self.stride, columns=None if self.columns is None else list(self.columns), actions=self.actions)

    @classmethod
    def from_dict(cls, d: dict) -> "History":
        cols = d.get("columns")
        return cls(steps=d["steps"], stride=d.get("stride", 1), columns=None if cols is None else tuple(cols), actions=d.get("actions", True))
