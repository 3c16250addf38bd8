"""The per-env adaptive curriculum off the GPU: csrc/mocca_curriculum.h -- the one set of functions that holds the rule and the work of one
thread for device and host -- compiled as plain C++ into a stand-alone program (tests/curriculum_host.cpp, which runs every thread of every
launch as the kernel does, in both orders) and held, BIT FOR BIT, to the numpy restatement (tests/curriculum_reference.py); the rule's power
over five plausible wrong readings; the ranges of `Curriculum`; the ABI's declarations; the refusals that touch no device."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import curriculum_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mocca_envs_amd", "csrc")
ENTRY_POINTS = ("mocca_set_curriculum", "mocca_get_curriculum", "mocca_curriculum_apply")
N, LAUNCHES, SEED, ENV_OFFSET = 300, 400, 0x1234567899ABCDEF, 1000     # done with probability 0.2, s uniform in 0 .. 20: ~80 episodes per env


def cfg(promote_at, demote_at, patience, min_level, max_level, recycle):
    return dict(promote_at=promote_at, demote_at=demote_at, patience=patience, min_level=min_level, max_level=max_level, recycle=recycle)


# name -> (configuration, the levels the envs start at).  The band [3, 6] starts OUTSIDE itself, at the raw levels 0 and 9 a host write
# (mocca_set_param_v) may leave: the rule is judged as if the level had always been that.
CONFIGS = {
    "patience1": (cfg(12, 5, 1, 0, 9, 0), np.zeros(N, np.float32)),
    "patience3_recycle": (cfg(9, 8, 3, 0, 9, 1), np.full(N, 5, np.float32)),
    "patience1_recycle": (cfg(8, 3, 1, 0, 9, 1), np.full(N, 7, np.float32)),
    "pinned": (cfg(10, 9, 2, 4, 4, 1), np.full(N, 4, np.float32)),
    "band_3_6": (cfg(10, 7, 2, 3, 6, 1), np.where(np.arange(N) % 2, 9, 0).astype(np.float32)),
}
# which wrong reading a configuration can tell from the rule: with patience 1 a streak is never carried, a pinned level never holds, and
# only a recycling configuration draws
APPLIES = {
    "no_hold": lambda c: c["min_level"] < c["max_level"], "hold_kept": lambda c: c["min_level"] < c["max_level"],
    "streak_kept": lambda c: c["patience"] > 1 and c["min_level"] < c["max_level"], "strict": lambda c: c["min_level"] < c["max_level"],
    "recycle_by_step": lambda c: c["recycle"] and c["min_level"] < c["max_level"],
}


@pytest.fixture(scope="module")
def streams():
    return R.stream(N, LAUNCHES)


@pytest.fixture(scope="module")
def header_run(tmp_path_factory, streams):
    """the header as a host program (g++, no HIP) -> run(config name) -> per launch (level bits u32 [N], streak, hold i32 [N], totals f32
    [10, 4], draw words u32 [N])"""
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to pin mocca_curriculum.h on the host"
    exe = str(tmp_path_factory.mktemp("curriculum") / "curriculum_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "curriculum_host.cpp"), "-o", exe])
    cache = {}

    def run(name):
        if name not in cache:
            c, start = CONFIGS[name]
            base = exe + "." + name
            with open(base + ".in", "wb") as f:
                f.write(struct.pack("<9i2I", N, LAUNCHES, c["promote_at"], c["demote_at"], c["patience"], c["min_level"], c["max_level"],
                                    c["recycle"], ENV_OFFSET, SEED & 0xFFFFFFFF, SEED >> 32))
                f.write(start.astype("<f4").tobytes())
                for done, info, episode, _ in streams:
                    f.write(done.astype("u1").tobytes() + info.astype("<i4").tobytes() + episode.astype("<u4").tobytes())
            subprocess.check_call([exe, base + ".in", base + ".out"])      # (exit 7: the thread order mattered)
            raw = np.fromfile(base + ".out", "<u4").reshape(LAUNCHES, 4 * N + R.LEVELS * R.TOTALS)
            cache[name] = (raw[:, :N], raw[:, N:2 * N].view(np.int32), raw[:, 2 * N:3 * N].view(np.int32),
                           raw[:, 3 * N:3 * N + 40].view(np.float32).reshape(LAUNCHES, R.LEVELS, R.TOTALS), raw[:, 3 * N + 40:])
        return cache[name]
    return run


def restated(name, streams, mutate=None, order=1):
    """the same tables from the restatement"""
    c, start = CONFIGS[name]
    rule = R.Rule(c, start, SEED, ENV_OFFSET, mutate)
    level, streak, hold, totals, draws = [], [], [], [], []
    for done, info, episode, step in streams:
        rule(done, info, episode, step)
        level.append(rule.level.view(np.uint32).copy()); streak.append(rule.streak.copy()); hold.append(rule.hold.copy())
        totals.append(rule.totals.copy()); draws.append(R.draw(c, SEED, rule.gid, episode)[0])
    return tuple(np.stack(x) for x in (level, streak, hold, totals, draws))


def test_header_declares_the_calls_and_lib_binds_them():
    from mocca_envs_amd import lib as L
    text = open(os.path.join(ROOT, "include", "mocca.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(mocca_handle h" % name, text), name
        assert name in L.SYMBOLS, name
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", text) and L.ABI_VERSION == 8
    assert int(re.search(r"#define MOCCA_CUR_MAX_LEVEL (\d+)", text).group(1)) == L.CUR_MAX_LEVEL == R.MAX_LEVEL == 9
    assert int(re.search(r"#define MOCCA_CUR_MAX_PATIENCE (\d+)", text).group(1)) == L.CUR_MAX_PATIENCE == R.MAX_PATIENCE == 64
    assert (L.CUR_LEVELS, L.CUR_TOTALS) == (R.LEVELS, R.TOTALS) == (10, 4)
    fields = re.search(r"typedef struct mocca_curriculum \{(.*?)\} mocca_curriculum;", text, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert fields == [n for n, _ in L.CurriculumConfig._fields_] == ["promote_at", "demote_at", "patience", "min_level", "max_level", "recycle"]
    head = open(os.path.join(CSRC, "mocca_curriculum.h")).read()
    for said in ("NOT PART OF THE mocca_get_state / mocca_get_task SNAPSHOT", "A HOST WRITE OF LEVELS IS JUDGED AS IF THE LEVEL HAD ALWAYS",
                 "The planner ids are out of scope", "(g, 0, E, 6)"):
        assert said in text, said
    assert "No thread reads a word another thread of the launch writes" in head and "#if defined(__HIPCC__)" in head
    assert "CUR_DOMAIN = 6u" in head and "6 is the adaptive curriculum's" in open(os.path.join(CSRC, "mocca_randomise.h")).read()


def test_library_exports_the_calls():
    import ctypes as C
    from mocca_envs_amd.build import build_lib
    so = C.CDLL(build_lib())
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name


@pytest.mark.parametrize("name", list(CONFIGS))
def test_header_equals_the_restatement_bit_for_bit(header_run, streams, name):
    c, start = CONFIGS[name]
    got, ref = header_run(name), restated(name, streams)
    for what, a, b in zip(("levels", "streaks", "holds", "totals", "draws"), got, ref):
        assert a.shape == b.shape and np.array_equal(a, b), what
    level, streak, hold, totals, _ = ref
    lv = np.concatenate([R.level_of(start)[None], R.level_of(level.view(np.float32))])      # [1 + launches, N], the start first
    hold = np.concatenate([np.zeros((1, N), np.int32), hold])
    # the streams exercise what they are meant to
    judged = totals[-1][:, 0].sum()
    ended = sum(int((d != 0).sum()) for d, _, _, _ in streams)
    assert ended > 60 * N and totals[-1][:, 2].sum() > 0 and totals[-1][:, 3].sum() > 0
    assert (totals[-1] == np.round(totals[-1])).all() and totals[-1].max() < 2 ** 24
    if c["min_level"] == c["max_level"]:
        assert (lv == c["min_level"]).all() and not hold.any() and judged == ended       # nothing moves, nothing is held, every episode counts
    else:
        moves = (np.diff(lv, axis=0) != 0).sum()
        assert moves > 5 * N and judged == ended - (moves - hold[-1].sum())              # every move exempts exactly one later episode
        assert (np.diff(lv, axis=0) > 0).any() and (np.diff(lv, axis=0) < 0).any()
        assert (lv[-1] >= c["min_level"]).all() and (lv[-1] <= c["max_level"]).all()     # also from outside the band
    if c["patience"] > 1:
        assert streak.max() == c["patience"] - 1 and streak.min() == 1 - c["patience"]
    if c["recycle"] and c["min_level"] < c["max_level"]:
        jumps = (np.diff(lv, axis=0) < -1).sum()                                         # a recycled env lands anywhere in the band
        assert jumps > N // 10, jumps


@pytest.mark.parametrize("name,mutate", [(n, m) for n in CONFIGS for m in R.MUTATIONS if APPLIES[m](CONFIGS[n][0])])
def test_the_rule_rejects_a_wrong_reading(header_run, streams, name, mutate):
    """each plausible wrong reading of the rule differs from the header in the state of many envs on these very streams"""
    got, wrong = header_run(name), restated(name, streams, mutate)
    differs = (got[0] != wrong[0]) | (got[1] != wrong[1]) | (got[2] != wrong[2])          # [launch, env]
    assert differs.any(0).sum() >= N // 10, (mutate, int(differs.any(0).sum()))


def test_every_wrong_reading_is_told_apart_somewhere():
    assert len(R.MUTATIONS) >= 5
    for m in R.MUTATIONS:
        assert sum(bool(APPLIES[m](c)) for c, _ in CONFIGS.values()) >= 2, m


def test_both_thread_orders_give_the_same_words(header_run, streams):
    """the host program runs the threads of every launch ascending and descending and exits 7 where a word differs; the restatement with
    the envs renumbered backwards agrees too (a thread owns its env; the totals are sums of whole numbers)"""
    name = "patience3_recycle"
    c, start = CONFIGS[name]
    got = header_run(name)                                                                # (ran both orders: check_call raised otherwise)
    rule = R.Rule(c, start[::-1], SEED, 0)
    rule.gid = (ENV_OFFSET + np.arange(N))[::-1]
    for done, info, episode, step in streams:
        rule(done[::-1], info[::-1], episode[::-1])
    assert np.array_equal(rule.level[::-1].view(np.uint32), got[0][-1]) and np.array_equal(rule.streak[::-1], got[1][-1])
    assert np.array_equal(rule.hold[::-1], got[2][-1]) and np.array_equal(rule.totals, got[3][-1])


def test_the_hold_exempts_exactly_the_episode_in_flight():
    """one env, patience 1: a promotion, the exempt episode, then judgement again"""
    rule = R.Rule(cfg(10, 2, 1, 0, 9, 0), [0.0])
    step = lambda s: (rule([1], [s], [0]), (int(rule.levels()[0]), int(rule.streak[0]), int(rule.hold[0])))[1]
    assert step(10) == (1, 0, 1)             # a success at level 0: level 1, held
    assert step(0) == (1, 0, 0)              # the episode laid out at level 0 fails: not judged, the hold is cleared
    assert step(0) == (0, 0, 1)              # the first episode of level 1 fails: down
    assert step(20) == (0, 0, 0) and step(5) == (0, 0, 0) and step(2) == (0, 0, 0)        # exempt; neither; a failure at min_level stays
    assert rule.totals[0].tolist() == [3, 17, 1, 1] and rule.totals[1].tolist() == [1, 0, 0, 1]


def test_curriculum_ranges():
    from mocca_envs_amd.curriculum import Curriculum
    c = Curriculum(12, 5)
    assert (c.patience, c.min_level, c.max_level, c.recycle) == (1, 0, 9, False)
    k = Curriculum(3, -1, patience=64, min_level=9, max_level=9, recycle=True).config()
    assert (k.promote_at, k.demote_at, k.patience, k.min_level, k.max_level, k.recycle) == (3, -1, 64, 9, 9, 1)
    assert Curriculum.from_dict(Curriculum(9, 8, 3, 2, 7, True).as_dict()) == Curriculum(9, 8, 3, 2, 7, True)
    api = open(os.path.join(CSRC, "mocca_api_curriculum.hip")).read()
    for kw, said in ((dict(promote_at=5, demote_at=5), "demote_at must be smaller than promote_at"),
                     (dict(promote_at=5, demote_at=6), "demote_at must be smaller than promote_at"),
                     (dict(promote_at=5, demote_at=1, patience=0), "patience must be 1 .. "),
                     (dict(promote_at=5, demote_at=1, patience=65), "patience must be 1 .. "),
                     (dict(promote_at=5, demote_at=1, min_level=-1), "the levels must satisfy 0 <= min_level <= max_level <= "),
                     (dict(promote_at=5, demote_at=1, max_level=10), "the levels must satisfy 0 <= min_level <= max_level <= "),
                     (dict(promote_at=5, demote_at=1, min_level=6, max_level=5), "the levels must satisfy 0 <= min_level <= max_level <= "),
                     (dict(promote_at=5, demote_at=1, recycle=2), "recycle must be 0 or 1")):
        with pytest.raises(ValueError, match=re.escape(said)):
            Curriculum(**kw)
        assert '"' + said in api, said                                                   # the C side's sentence
    with pytest.raises(ValueError, match="whole number"):
        Curriculum(5.5, 1)


def test_trainer_refuses_before_touching_a_device():
    from mocca_envs_amd.curriculum import Curriculum
    from mocca_envs_amd.trainer_api import make_vec_envs
    cur = Curriculum(12, 5)
    for env_id in ("Walker3DCustomEnv-v0", "Walker3DPlannerEnv-v0", "CassieEnv-v0"):
        with pytest.raises(ValueError, match="only the Stepper ids have curriculum levels"):
            make_vec_envs(env_id, 0, 4, curriculum=cur)
    with pytest.raises(NotImplementedError, match=re.escape("curriculum needs one handle (sub_batches=1)")):
        make_vec_envs("Walker3DStepperEnv-v0", 0, 4, curriculum=cur, sub_batches=2)
    with pytest.raises(NotImplementedError, match=re.escape("curriculum needs one handle (sub_batches=1)")):
        make_vec_envs("Walker3DStepperEnv-v0", 0, 4, curriculum=cur, devices=[0, 1])


def test_multi_handle_wrappers_refuse():
    from mocca_envs_amd.multi import ShardedVecEnv, SubBatchedVecEnv
    for cls in (SubBatchedVecEnv, ShardedVecEnv):
        multi = object.__new__(cls)
        multi.parts = []
        for name in ("set_curriculum", "curriculum_levels", "curriculum_state", "curriculum_apply"):
            with pytest.raises(NotImplementedError, match=re.escape(f"{name} needs one handle (one device, sub_batches=1)")):
                getattr(multi, name)()
