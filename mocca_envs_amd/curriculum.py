"""The per-env adaptive curriculum of a Stepper `VecEnv` on the device (include/mocca.h mocca_set_curriculum): what a trainer states once
and every env then applies to itself behind each step -- its own episodes move its own level.  The rule and the kernel:
csrc/mocca_curriculum.h."""
from __future__ import annotations

from dataclasses import dataclass

from . import lib as _lib

STEPPER_IDS_ONLY = "only the Stepper ids have curriculum levels"     # (the planner ids stand on a terrain bank without difficulty bands)


def _whole(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be a whole number (got {v!r})")
    return int(v)


@dataclass(frozen=True)
class Curriculum:
    """An episode that ends with `steps_reached >= promote_at` is a success, one with `steps_reached <= demote_at` a failure (demote_at <
    promote_at; in between it is neither and ends a run).  `patience` successes in a row move the env one level up, `patience` failures
    in a row one level down, inside [min_level, max_level].  The episode in flight when a level changes is not judged: it was laid out
    before the change.  `recycle=True`: an env promoted at max_level restarts at a level drawn uniformly from the band, so the batch keeps
    covering every level."""
    promote_at: int
    demote_at: int
    patience: int = 1
    min_level: int = 0
    max_level: int = _lib.CUR_MAX_LEVEL
    recycle: bool = False

    def __post_init__(self):
        # the ranges and their sentences are mocca_set_curriculum's (csrc/mocca_api_curriculum.hip)
        p, d = _whole("promote_at", self.promote_at), _whole("demote_at", self.demote_at)
        pat, lo, hi = _whole("patience", self.patience), _whole("min_level", self.min_level), _whole("max_level", self.max_level)
        if d >= p:
            raise ValueError(f"demote_at must be smaller than promote_at (got {d} and {p})")
        if not 1 <= pat <= _lib.CUR_MAX_PATIENCE:
            raise ValueError(f"patience must be 1 .. {_lib.CUR_MAX_PATIENCE} (got {pat})")
        if not 0 <= lo <= hi <= _lib.CUR_MAX_LEVEL:
            raise ValueError(f"the levels must satisfy 0 <= min_level <= max_level <= {_lib.CUR_MAX_LEVEL} (got {lo} and {hi})")
        if self.recycle not in (0, 1, False, True):
            raise ValueError(f"recycle must be 0 or 1 (got {self.recycle!r})")
        for k, v in (("promote_at", p), ("demote_at", d), ("patience", pat), ("min_level", lo), ("max_level", hi), ("recycle", bool(self.recycle))):
            object.__setattr__(self, k, v)

    def config(self) -> "_lib.CurriculumConfig":
        """the `mocca_curriculum` struct"""
        return _lib.CurriculumConfig(self.promote_at, self.demote_at, self.patience, self.min_level, self.max_level, int(self.recycle))

    def as_dict(self) -> dict:
        """plain numbers (what a saved policy file records)"""
        return dict(promote_at=self.promote_at, demote_at=self.demote_at, patience=self.patience, min_level=self.min_level,
                    max_level=self.max_level, recycle=self.recycle)

    @classmethod
    def from_dict(cls, d: dict) -> "Curriculum":
        return cls(**{k: d[k] for k in ("promote_at", "demote_at", "patience", "min_level", "max_level", "recycle") if k in d})
