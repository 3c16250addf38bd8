"""Domain randomisation of a `VecEnv` on the device (include/mocca.h mocca_set_randomisation / mocca_set_sensor_noise): what a trainer states
once and the env then applies in every episode -- weaker motors, late commands, pushes, noisy sensors.  Keying and arithmetic:
csrc/mocca_randomise.h."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from . import lib as _lib


@dataclass(frozen=True)
class Randomisation:
    """strength=(lo, hi): each episode draws its motor strength, 0 < lo <= hi <= 1, which scales the clipped action (the torque; the Cassie
    envs, whose action is a PD target, take (1, 1) alone).  latency=(lo, hi): each episode draws its action delay in steps, 0 <= lo <= hi <=
    7.  push=(interval, max): every `interval` steps (0: never; each episode draws its phase) the base's world-frame velocity jumps by up to
    `max` m/s along x and along y.  obs_noise: None, one scale for every observation column, or one per column (>= 0): uniform noise of that
    half-width is added to the POLICY's row; `envs.privileged` stays clean.  privileged=True (needs `privileged_scan=`): the four-number
    record of the env's plant -- strength, delay, steps until the next push, 0 -- becomes the tail of the privileged row."""
    strength: Tuple[float, float] = (1.0, 1.0)
    latency: Tuple[int, int] = (0, 0)
    push: Tuple[int, float] = (0, 0.0)
    obs_noise: Union[None, float, tuple] = None
    privileged: bool = False

    def __post_init__(self):
        lo, hi = (float(x) for x in self.strength)
        if not (0.0 < lo <= hi <= 1.0):
            raise ValueError(f"strength=(lo, hi) must satisfy 0 < lo <= hi <= 1 (got {self.strength})")
        dl, dh = self.latency
        if int(dl) != dl or int(dh) != dh or not (0 <= dl <= dh <= _lib.RAND_MAX_DELAY):
            raise ValueError(f"latency=(lo, hi) must be whole steps with 0 <= lo <= hi <= {_lib.RAND_MAX_DELAY} (got {self.latency})")
        interval, pmax = self.push
        if int(interval) != interval or not (0 <= interval <= _lib.RAND_MAX_INTERVAL):
            raise ValueError(f"push=(interval, max): interval must be a whole number of steps, 0 .. {_lib.RAND_MAX_INTERVAL} (got {interval})")
        if not math.isfinite(pmax) or pmax < 0:
            raise ValueError(f"push=(interval, max): max must be finite and not negative (got {pmax})")
        if self.obs_noise is not None:
            s = np.asarray(self.obs_noise, np.float64)
            if s.ndim > 1 or not np.isfinite(s).all() or (s < 0).any():
                raise ValueError("obs_noise must be None, a scale >= 0 or one finite scale >= 0 per observation column")
            object.__setattr__(self, "obs_noise", float(s) if s.ndim == 0 else tuple(float(x) for x in s))
        object.__setattr__(self, "strength", (lo, hi))
        object.__setattr__(self, "latency", (int(dl), int(dh)))
        object.__setattr__(self, "push", (int(interval), float(pmax)))
        object.__setattr__(self, "privileged", bool(self.privileged))

    def config(self) -> "_lib.RandomisationConfig":
        """the `mocca_randomisation` struct of the plant's part"""
        return _lib.RandomisationConfig(self.strength[0], self.strength[1], self.latency[0], self.latency[1], self.push[0], self.push[1])

    def noise_scales(self, obs_dim: int) -> Optional[np.ndarray]:
        """float32 [obs_dim], or None without sensor noise"""
        if self.obs_noise is None:
            return None
        s = np.asarray(self.obs_noise, np.float32)
        if s.ndim == 0:
            return np.full(obs_dim, s, np.float32)
        if s.shape != (obs_dim,):
            raise ValueError(f"obs_noise has {s.size} scales, the observation {obs_dim} columns")
        return np.ascontiguousarray(s)

    def as_dict(self) -> dict:
        """plain numbers (what a saved policy file records)"""
        return dict(strength=list(self.strength), latency=list(self.latency), push=list(self.push),
                    obs_noise=(list(self.obs_noise) if isinstance(self.obs_noise, tuple) else self.obs_noise), privileged=self.privileged)

    @classmethod
    def from_dict(cls, d: dict) -> "Randomisation":
        d = dict(d)
        if isinstance(d.get("obs_noise"), list):
            d["obs_noise"] = tuple(d["obs_noise"])
        return cls(strength=tuple(d.get("strength", (1.0, 1.0))), latency=tuple(d.get("latency", (0, 0))), push=tuple(d.get("push", (0, 0.0))),
                   obs_noise=d.get("obs_noise"), privileged=bool(d.get("privileged", False)))
