"""Domain randomisation off the GPU: csrc/mocca_randomise.h -- the one set of functions that holds the arithmetic of every draw for device
and host -- compiled as plain C++ into a stand-alone program (tests/randomisation_host.cpp, which composes them as the kernels do) and held,
BIT FOR BIT, to the numpy restatement (tests/randomisation_reference.py); the rule's power over plausible wrong readings; the ranges of
`Randomisation`; the ABI's declarations; and what the GPU tests rely on: among 67 envs of seed 0 every delay and every phase occurs."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import randomisation_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mocca_envs_amd", "csrc")
ENTRY_POINTS = ("mocca_set_randomisation", "mocca_get_effective_action", "mocca_set_sensor_noise", "mocca_sensor_noise",
                "mocca_randomisation_record")
SEED = 0x5EED0000BEEF
N, STEPS, EPISODES, OFFSET, ACT_DIM, DIM = 64, 40, 3, 5, 3, 9      # 9 columns: three noise blocks, the last one ragged


def _inputs(planar):
    """dyadic ranges, scales and rows: every fmaf of the restatement is exact in float64"""
    rng = np.random.default_rng(7)
    cfg = R.Config(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5), planar=planar)
    scale = (2.0 ** -np.arange(1, DIM + 1)).astype(np.float32)
    rows = (rng.integers(-64, 65, (N, DIM)) / 16.0).astype(np.float32)
    act = (rng.integers(-48, 49, (EPISODES, STEPS, N, ACT_DIM)) / 32.0).astype(np.float32)       # 1.5 x uniform: the clip acts
    act[0, 3, 2, 1] = np.nan                                                                    # a NaN passes through the clip
    return cfg, scale, rows, act


@pytest.fixture(scope="module")
def header_run(tmp_path_factory):
    """the header as a host program (g++, no HIP) -> run(planar) -> uint32 [EPISODES, STEPS, N, 11 + ACT_DIM + DIM]"""
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to pin mocca_randomise.h on the host"
    exe = str(tmp_path_factory.mktemp("randomise") / "randomisation_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(ROOT, "tests", "randomisation_host.cpp"), "-o", exe])
    cache = {}

    def run(planar):
        if planar not in cache:
            cfg, scale, rows, act = _inputs(planar)
            base = exe + f".{int(planar)}"
            with open(base + ".in", "wb") as f:
                f.write(struct.pack("<Q6i", SEED, N, STEPS, EPISODES, OFFSET, ACT_DIM, DIM))
                f.write(struct.pack("<ff3ifi", cfg.lo, cfg.hi, cfg.dmin, cfg.dmax, cfg.interval, cfg.push_max, int(planar)))
                for a in (scale, rows, act):
                    f.write(a.astype("<f4").tobytes())
            subprocess.check_call([exe, base + ".in", base + ".out"])
            cache[planar] = np.fromfile(base + ".out", "<u4").reshape(EPISODES, STEPS, N, 11 + ACT_DIM + DIM)
        return cache[planar]
    return run


def restated(planar, mutate=None):
    """the same table from the restatement"""
    cfg, scale, rows, act = _inputs(planar)
    g = OFFSET + np.arange(N)
    out = np.zeros((EPISODES, STEPS, N, 11 + ACT_DIM + DIM), np.uint32)
    plant = R.Plant(SEED, g, cfg, ACT_DIM, mutate)
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    for e in range(EPISODES):
        strength, delay, phase = R.episode_params(SEED, g, e, cfg, mutate)
        for t in range(STEPS):
            eff, fires, dv = plant.step(act[e, t], t, e)
            o = out[e, t]
            o[:, 0], o[:, 1], o[:, 2], o[:, 3] = bits(strength), delay, phase, fires
            o[:, 4:6] = bits(dv)
            o[:, 6:10] = bits(np.stack([strength, delay.astype(np.float32), R.until_push(t, phase, cfg).astype(np.float32), 0 * strength], -1))
            o[:, 11:11 + ACT_DIM] = bits(eff)
            o[:, 11 + ACT_DIM:] = bits(R.noise(SEED, g, t, e, rows, scale, mutate))
    return out


def _same(a, b):
    """bit for bit, a NaN equal to itself by its bits"""
    return np.array_equal(a, b)


def test_header_declares_the_calls_and_lib_binds_them():
    from mocca_envs_amd import lib as L
    text = open(os.path.join(ROOT, "include", "mocca.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(mocca_handle h" % name, text), name
        assert name in L.SYMBOLS, name
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", text) and L.ABI_VERSION == 8 and "MOCCA_ABI_VERSION stays 8" in text
    assert int(re.search(r"#define MOCCA_RAND_WORDS (\d+)", text).group(1)) == L.RAND_WORDS == R.RAND_WORDS == 4
    assert int(re.search(r"#define MOCCA_RAND_MAX_DELAY (\d+)", text).group(1)) == L.RAND_MAX_DELAY == R.MAX_DELAY == 7
    for said in ("NOT\n *                                      PART OF THE mocca_get_state / mocca_get_task SNAPSHOT", "ONE\n *                                      STEP LATE",
                 "MOCCA_TASK_CASSIE takes the range [1, 1] ALONE"):
        assert said in text, said
    import ctypes as C
    assert C.sizeof(L.RandomisationConfig) == 24


@pytest.mark.parametrize("planar", [False, True])
def test_header_equals_the_restatement_bit_for_bit(header_run, planar):
    got, ref = header_run(planar), restated(planar)
    names = ["strength", "delay", "phase", "fires", "dvx", "dvy", "rec0", "rec1", "rec2", "rec3", "pad"]
    for c, name in enumerate(names):
        assert _same(got[..., c], ref[..., c]), name
    assert _same(got[..., 11:11 + ACT_DIM], ref[..., 11:11 + ACT_DIM]), "effective action"
    assert _same(got[..., 11 + ACT_DIM:], ref[..., 11 + ACT_DIM:]), "noise"
    # the table exercises what it is meant to: every delay, pushes (never at T == 0), the clip, the NaN, envs still waiting for their first action
    assert set(np.unique(ref[..., 1])) == {0, 1, 2, 3} and set(np.unique(ref[..., 2])) == {0, 1, 2, 3}
    assert ref[..., 3].sum() > N and ref[:, 0, :, 3].sum() == 0
    eff = ref[..., 11:11 + ACT_DIM].view(np.float32)
    assert np.isnan(eff).sum() == 1 and np.nanmax(np.abs(eff)) <= 1.0 and (eff[:, 0][ref[:, 0, :, 1] > 0] == 0).all()
    dvy = ref[..., 5].view(np.float32)
    assert (dvy == 0).all() if planar else (dvy != 0).sum() > N


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_the_rule_rejects_a_wrong_reading(header_run, mutate):
    """each plausible wrong reading of section 1 differs from the header in many entries: the bit-for-bit rule sees it"""
    planar = mutate == "planar_dvy"
    got, wrong = header_run(planar), restated(planar, mutate)
    assert not _same(got, wrong)
    differ = (got != wrong).any(-1)
    if mutate == "push_at_zero":     # exactly the episodes whose phase is 0, at their step 0
        assert np.array_equal(differ, (got[..., 2] == 0) & (np.arange(STEPS)[None, :, None] == 0)) and differ.sum() >= EPISODES * N // 8
    else:
        assert differ.sum() >= N, mutate


def test_until_push_counts_down_to_the_push():
    cfg = R.Config(push=(4, 0.5))
    for phase in range(4):
        u = R.until_push(np.arange(20), phase, cfg)
        fires = (np.arange(20) > 0) & ((np.arange(20) + phase) % 4 == 0)
        assert (u[fires] == 0).all() and (u[~fires] > 0).all() and (np.diff(u)[~fires[:-1]] == -1).all()
    assert (R.until_push(np.arange(5), 0, R.Config()) == -1).all()


def test_fma32_is_the_correctly_rounded_fma():
    """against exact rational arithmetic, on operands whose float64 sum is inexact as well"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-30, 3, 400)).astype(np.float32)
    got = R.fma32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_every_delay_and_phase_occurs_among_67_envs_of_seed_0():
    """the GPU tests (N = 67, seed 0, delays 0 .. 3, interval 4) rely on it"""
    cfg = R.Config(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5))
    for episode in (0, 1):
        strength, delay, phase = R.episode_params(0, np.arange(67), episode, cfg)
        assert set(delay) == {0, 1, 2, 3} and set(phase) == {0, 1, 2, 3}
        assert strength.min() >= 0.5 and strength.max() <= 1.0 and np.unique(strength).size > 60


def test_randomisation_ranges():
    from mocca_envs_amd.randomisation import Randomisation
    r = Randomisation(strength=(0.5, 1), latency=(0, 3), push=(4, 0.5), obs_noise=2 ** -6, privileged=True)
    c = r.config()
    assert (c.strength_lo, c.strength_hi, c.delay_min, c.delay_max, c.push_interval, c.push_max) == (0.5, 1.0, 0, 3, 4, 0.5)
    assert np.array_equal(r.noise_scales(5), np.full(5, 2 ** -6, np.float32)) and Randomisation().noise_scales(5) is None
    assert Randomisation.from_dict(r.as_dict()) == r
    assert Randomisation(obs_noise=[0.0, 0.5]).noise_scales(2).tolist() == [0.0, 0.5]
    with pytest.raises(ValueError, match="2 scales"):
        Randomisation(obs_noise=[0.0, 0.5]).noise_scales(3)
    for kw in (dict(strength=(0.0, 1.0)), dict(strength=(0.5, 1.5)), dict(strength=(1.0, 0.5)), dict(strength=(float("nan"), 1.0)),
               dict(latency=(-1, 2)), dict(latency=(3, 2)), dict(latency=(0, 8)), dict(latency=(0, 1.5)),
               dict(push=(-1, 0.5)), dict(push=(65537, 0.5)), dict(push=(4, -0.5)), dict(push=(4, float("inf"))), dict(push=(2.5, 0.5)),
               dict(obs_noise=-1.0), dict(obs_noise=float("nan")), dict(obs_noise=[0.1, -0.1])):
        with pytest.raises(ValueError):
            Randomisation(**kw)


def test_multi_handle_wrappers_refuse():
    from mocca_envs_amd.multi import ShardedVecEnv, SubBatchedVecEnv
    for cls in (SubBatchedVecEnv, ShardedVecEnv):
        multi = object.__new__(cls)
        multi.parts = []
        for name in ("set_randomisation", "effective_action", "set_sensor_noise", "sensor_noise", "randomisation_record"):
            with pytest.raises(NotImplementedError, match="needs one handle"):
                getattr(multi, name)()
