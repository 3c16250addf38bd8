"""Reference of the terrain bank (include/mocca.h mocca_generate_heightfields / mocca_set_env_fields), shared by test_terrain_bank.py and
test_gpu_terrain_bank.py.

`KernelDraws` is an `rng` with `uniform` / `randint` / `rand` that hands `host_logic.random_height_field` -- the f64 restatement of the
reference's generator, pinned to the import by test_golden_planner.py -- exactly the parameters the kernel uses: the Philox words of
csrc/mocca_terrain.h's keying, the affine maps done in float32 and then widened.  What is left between `reference_field` and the kernel is
the field arithmetic alone, f64 against f32.  `env_field_draw` restates the field-of-env draw of redraw-at-reset."""
import numpy as np

import policy_reference as P
from mocca_envs_amd import host_logic as H

MAX_PEAKS = 256          # stride of the seven parameter arrays, whatever n_peaks is
DOMAIN_TERRAIN, DOMAIN_ENV_FIELD = 3, 2
F32 = np.float32


def uniforms(seed: int, block: int, field: int, n: int, offset: int = 0) -> np.ndarray:
    """float32 uniforms of draws d = offset .. offset + n - 1 of (block, field): (w >> 8) 2^-24, w = word d & 3 of philox4x32(d >> 2, block, field, 3)"""
    d = np.arange(offset, offset + n, dtype=np.uint64)
    c = np.zeros((n, 4), np.uint64)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = d >> np.uint64(2), block, field, DOMAIN_TERRAIN
    w = P.philox4x32(c, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w = w[np.arange(n), (d & np.uint64(3)).astype(np.int64)]
    return (w >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)


class KernelDraws:
    """the generator's draws of field `field` under `seed`, in the order host_logic.random_height_field asks for them"""

    def __init__(self, seed: int, field: int):
        self.seed, self.field = int(seed), int(field)
        self.array = 0      # next of the seven peak arrays
        self.octave = 0     # next lattice

    def _next(self, n):
        assert n <= MAX_PEAKS and self.array < 7
        u = uniforms(self.seed, 0, self.field, n, MAX_PEAKS * self.array)
        self.array += 1
        return u

    def uniform(self, lo, hi, size):
        u = self._next(size)
        lo, hi = F32(lo), F32(hi)
        if self.array == 1:
            assert (lo, hi) == (F32(0.1), F32(3.0))
            return (F32(0.1) + F32(2.9) * u).astype(np.float64)        # the kernel's constants: 0.1f + 2.9f u
        if self.array in (4, 5):
            return (F32(1.0) + F32(15.0) * u).astype(np.float64)
        return (lo + (F32(2.0) * hi) * u).astype(np.float64)           # -half + (2 half) u

    def randint(self, lo, hi, size):
        assert (lo, hi) == (1, 6)
        return np.minimum(1 + (F32(5.0) * self._next(size)).astype(np.int64), 5)

    def rand(self, r0, r1):
        self.octave += 1
        assert (r0, r1) == {1: (5, 5), 2: (9, 9)}[self.octave]
        u = uniforms(self.seed, self.octave, self.field, r0 * r1).reshape(r0, r1)
        # the kernel takes cos / sin of the float32 angle 2 pi u; host_logic multiplies by 2 pi in f64: hand it the u that gives that angle
        return (F32(6.283185307179586) * u).astype(np.float64) / (2 * np.pi)


def reference_field(seed: int, field: int, rows: int, cols: int, scale: float, n_peaks: int = 256, gain: float = 1.0) -> np.ndarray:
    """float64 [rows][cols]: host_logic.random_height_field on the kernel's draws, times gain"""
    flat = H.random_height_field(KernelDraws(seed, field), (rows, cols), scale, n_peaks)
    return flat.reshape(rows, cols) * float(gain)


def peak_params(seed: int, field: int, rows: int, cols: int, scale: float) -> np.ndarray:
    """float32 [7][256]: the parameter arrays as the kernel stages them (exponents as their halves 1 .. 5)"""
    rng = KernelDraws(seed, field)
    h0, h1 = F32(rows) / F32(scale) * F32(0.5), F32(cols) / F32(scale) * F32(0.5)
    out = [rng.uniform(0.1, 3, MAX_PEAKS), rng.uniform(-h0, h0, MAX_PEAKS), rng.uniform(-h1, h1, MAX_PEAKS), rng.uniform(1, 16, MAX_PEAKS),
           rng.uniform(1, 16, MAX_PEAKS), rng.randint(1, 6, MAX_PEAKS), rng.randint(1, 6, MAX_PEAKS)]
    return np.stack(out).astype(F32)


def gradient_angles(seed: int, field: int) -> np.ndarray:
    """float32 [106]: the lattice angles 2 pi u, octave 1 (5 x 5, row-major) then octave 2 (9 x 9)"""
    return np.concatenate([F32(6.283185307179586) * uniforms(seed, 1, field, 25), F32(6.283185307179586) * uniforms(seed, 2, field, 81)]).astype(F32)


def field_uniforms(seed: int, field: int) -> np.ndarray:
    """float32 [7 * 256 + 25 + 81]: every uniform of one field, the input of tests/terrain_host.cpp"""
    return np.concatenate([uniforms(seed, 0, field, 7 * MAX_PEAKS), uniforms(seed, 1, field, 25), uniforms(seed, 2, field, 81)])


def env_field_draw(seed: int, episode, env_ids, n_fields: int) -> np.ndarray:
    """field of (global) env ids in `episode` under redraw-at-reset: (uint64(w) n_fields) >> 32, w = word 0 of philox4x32(0, episode, env, 2)"""
    env_ids = np.asarray(env_ids, np.uint64)
    c = np.zeros((env_ids.size, 4), np.uint64)
    c[:, 1], c[:, 2], c[:, 3] = np.asarray(episode, np.uint64), env_ids, DOMAIN_ENV_FIELD
    w = P.philox4x32(c, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))[:, 0].astype(np.uint64)
    return ((w * np.uint64(n_fields)) >> np.uint64(32)).astype(np.int32)
