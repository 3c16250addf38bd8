"""The observation-action history off the GPU: csrc/mocca_history.h -- the one set of functions that holds the index rules and the work of one
thread for device and host -- compiled as plain C++ into a stand-alone program (tests/history_host.cpp, which runs every thread of every
call as the kernel does, in both orders) and held, BIT FOR BIT, to the numpy restatement (tests/history_reference.py); the rule's power over
five plausible wrong readings; the ranges of `History`; the ABI's declarations."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import history_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mocca_envs_amd", "csrc")
ENTRY_POINTS = ("mocca_set_history", "mocca_history_dim", "mocca_history")
N, CALLS, OBS_DIM, ACT_DIM = 64, 120, 52, 21          # 64 envs x 40 calls x 3 episodes' worth of calls, episodes ending at irregular steps
JUMP_AT, SKIP_AT, NO_ACT_AT = 50, 70, 90              # one T jump as a set_task would make, one skipped call, one call without an action
AGAIN_AT, AGAIN_NO_ACT_AT = 30, 100                   # calls made a second time without a step in between: as they were, and without the action
CONFIGS = {                                           # name -> (K, s, columns, A)
    "k3_all": (3, 1, list(range(OBS_DIM)), ACT_DIM),
    "k2_s3_some": (2, 3, [0, 5, 6, 17, 30, 44, 51], ACT_DIM),
    "k4_s2_actions_only": (4, 2, [], ACT_DIM),
    "k16_one_column": (16, 1, [0], 0),
}


def schedule():
    """per call: (have_act, T [N], E [N], rows [N, OBS_DIM], act [N, ACT_DIM]) or None for the skipped call (the counters move on all the
    same; two calls are made twice).  Episode lengths are drawn per env and episode, 3 .. 45 steps; at JUMP_AT envs 0 .. 7 leap 5 steps ahead and envs 8 .. 15 fall 3
    steps back.  The rows hold a NaN and a -0.0: a copy keeps their bits."""
    rng = np.random.default_rng(11)
    t, e = np.zeros(N, np.int64), np.zeros(N, np.int64)
    left = rng.integers(3, 46, N)
    out = []
    for k in range(CALLS):
        rows = rng.standard_normal((N, OBS_DIM)).astype(np.float32)
        act = rng.standard_normal((N, ACT_DIM)).astype(np.float32)
        rows[3, 5], rows[4, 0], act[5, 2] = np.nan, -0.0, -0.0
        if k == JUMP_AT:
            t[:8] += 5
            t[8:16] = np.maximum(t[8:16] - 3, 0)
        out.append(None if k == SKIP_AT else (k != 0 and k != NO_ACT_AT, t.copy(), e.copy(), rows, act))
        if k in (AGAIN_AT, AGAIN_NO_ACT_AT):
            out.append((k == AGAIN_AT, t.copy(), e.copy(), rows, act))
        t += 1
        left -= 1
        ended = left <= 0
        t[ended], e[ended] = 0, e[ended] + 1
        left[ended] = rng.integers(3, 46, int(ended.sum()))
    return out


@pytest.fixture(scope="module")
def header_run(tmp_path_factory):
    """the header as a host program (g++, no HIP) -> run(config name) -> uint32 [calls made, N, K (C + A)]"""
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to pin mocca_history.h on the host"
    exe = str(tmp_path_factory.mktemp("history") / "history_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "history_host.cpp"), "-o", exe])
    cache = {}

    def run(name):
        if name not in cache:
            K, s, cols, A = CONFIGS[name]
            made = [c for c in schedule() if c is not None]
            base = exe + "." + name
            with open(base + ".in", "wb") as f:
                f.write(struct.pack("<8i", N, len(made), OBS_DIM, ACT_DIM, K, s, len(cols), A))
                f.write(np.asarray(cols, "<i4").tobytes())
                for have_act, t, e, rows, act in made:
                    f.write(struct.pack("<i", int(have_act)))
                    for a, kind in ((t, "<u4"), (e, "<u4"), (rows, "<f4"), (act, "<f4")):
                        f.write(a.astype(kind).tobytes())
            subprocess.check_call([exe, base + ".in", base + ".out"])      # (exit 7: the thread order mattered)
            cache[name] = np.fromfile(base + ".out", "<u4").reshape(len(made), N, K * (len(cols) + A))
        return cache[name]
    return run


def restated(name, mutate=None):
    """the same table from the restatement, and the T of every call made"""
    K, s, cols, A = CONFIGS[name]
    h = R.History(N, K, s, cols, A, mutate)
    made = [c for c in schedule() if c is not None]
    blocks = np.stack([h(rows, act if have_act else None, t, e) for have_act, t, e, rows, act in made])
    return np.ascontiguousarray(blocks).view(np.uint32), np.stack([c[1] for c in made])


def _same(a, b):
    """bit for bit, a NaN equal to itself by its bits"""
    return np.array_equal(a, b)


def test_header_declares_the_calls_and_lib_binds_them():
    from mocca_envs_amd import lib as L
    text = open(os.path.join(ROOT, "include", "mocca.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(mocca_handle h" % name, text), name
        assert name in L.SYMBOLS, name
    assert re.search(r"#define MOCCA_ABI_VERSION 8\b", text) and L.ABI_VERSION == 8
    assert int(re.search(r"#define MOCCA_HIST_MAX_STEPS (\d+)", text).group(1)) == L.HIST_MAX_STEPS == R.MAX_STEPS == 16
    assert int(re.search(r"#define MOCCA_HIST_MAX_STRIDE (\d+)", text).group(1)) == L.HIST_MAX_STRIDE == R.MAX_STRIDE == 8
    assert int(re.search(r"#define MOCCA_HIST_MAX_DIM (\d+)", text).group(1)) == L.HIST_MAX_DIM == R.MAX_DIM == 1024
    assert L.HIST_MAX_ACT == R.MAX_ACT == 32
    head = open(os.path.join(CSRC, "mocca_history.h")).read()
    for said in ("NEWEST FIRST", "No thread reads a ring word that another thread of the same launch writes",
                 "THE RING IS NOT PART OF THE mocca_get_state / mocca_get_task SNAPSHOT", "mocca_task_step advances T without a history call"):
        assert said in text, said
    assert "No thread reads a ring word another thread of the same launch writes" in head and "#if defined(__HIPCC__)" in head


@pytest.mark.parametrize("name", list(CONFIGS))
def test_header_equals_the_restatement_bit_for_bit(header_run, name):
    K, s, cols, A = CONFIGS[name]
    W = len(cols) + A
    got, (ref, t) = header_run(name), restated(name)
    assert got.shape == ref.shape and _same(got, ref)
    # the table exercises what it is meant to: full blocks, empty blocks, episode boundaries, the jump, the skipped call, the bit copies
    pairs = (ref.reshape(len(ref), N, K, W) != 0).any(-1)              # [call, env, j]: pair j holds something
    assert (pairs.all(-1) & (t >= K * s)).any(), "no env shows a full block"
    assert (t < s).any() and not pairs[t < s].any(), "a block read at t < s is all zero"
    assert (t >= K * s).any() and (~pairs[t >= K * s]).any(), "the jump and the skipped call leave zero pairs behind"
    assert (np.diff(t, axis=0) < 0).sum() >= 2 * N, "three episodes per env"
    made = [c for c in schedule() if c is not None]
    again = [k for k in range(1, len(made)) if np.array_equal(made[k][1], made[k - 1][1]) and np.array_equal(made[k][2], made[k - 1][2])]
    assert len(again) == 2 and _same(ref[again[0]], ref[again[0] - 1]) and _same(ref[again[0] + 1], got[again[0] + 1])     # the same words twice
    assert A == 0 or s > 1 or not _same(ref[again[1]], ref[again[1] - 1])                  # ... and without the action, the newest action is +0.0
    if name == "k3_all":
        f = ref.view(np.float32)
        assert np.isnan(f).any() and (ref == 0x80000000).any()


# (a history without actions has no action to file late: that reading is the rule itself there)
@pytest.mark.parametrize("name,mutate", [(n, m) for n in CONFIGS for m in R.MUTATIONS if not (m == "action_late" and CONFIGS[n][3] == 0)])
def test_the_rule_rejects_a_wrong_reading(header_run, name, mutate):
    """each plausible wrong reading of the rule differs from the header in many blocks of these very inputs"""
    got, (wrong, _) = header_run(name), restated(name, mutate)
    assert not _same(got, wrong)
    assert (got != wrong).any(-1).sum() >= N, mutate


def test_a_skipped_call_is_a_zero_pair_not_old_data():
    """one env, K = 2: the frames around a skipped call, an episode boundary and a second call without a step"""
    h = R.History(1, 2, 1, [0], 1)
    row = lambda v: np.full((1, 1), v, np.float32)
    assert h(row(10), None, [0], [0]).tolist() == [[0, 0, 0, 0]]
    assert h(row(11), row(0.5), [1], [0]).tolist() == [[10, 0.5, 0, 0]]
    again = h(row(11), row(0.5), [1], [0])                                   # no step in between: the same words
    assert again.tolist() == [[10, 0.5, 0, 0]]
    assert h(row(12), row(0.25), [2], [0]).tolist() == [[11, 0.25, 10, 0.5]]
    assert h(row(14), row(0.75), [4], [0]).tolist() == [[0, 0, 12, 0]]        # the call at T = 3 was skipped: a zero pair; frame 2 never got its action
    assert h(row(20), None, [0], [1]).tolist() == [[0, 0, 0, 0]]              # a new episode reads nothing of the old one
    assert h(row(21), row(-1), [1], [1]).tolist() == [[20, -1, 0, 0]]


def test_history_ranges():
    from mocca_envs_amd.history import History
    h = History(3)
    cols, a = h.resolve(52, 21)
    assert cols.tolist() == list(range(52)) and cols.dtype == np.int32 and a == 21 and h.steps * (cols.size + a) == 219
    cols, a = History(2, stride=3, columns=[5, 0], actions=False).resolve(52, 21)
    assert cols.tolist() == [5, 0] and a == 0
    assert History(4, columns=[], actions=15).resolve(52, 21)[1] == 15
    assert History.from_dict(History(2, 3, (0, 5), True).as_dict()) == History(2, 3, (0, 5), True)
    for kw in (dict(steps=0), dict(steps=17), dict(steps=2.5), dict(steps=2, stride=0), dict(steps=2, stride=9), dict(steps=2, columns=[1, 1]),
               dict(steps=2, columns=[-1]), dict(steps=2, columns=[0.5]), dict(steps=2, actions=33), dict(steps=2, actions=-1)):
        with pytest.raises(ValueError):
            History(**kw)
    with pytest.raises(ValueError, match="column 52 is outside"):
        History(2, columns=[52]).resolve(52, 21)
    with pytest.raises(ValueError, match="at least one"):
        History(2, columns=[], actions=False).resolve(52, 21)
    with pytest.raises(ValueError, match="at most 1024"):
        History(16).resolve(52, 21)
    with pytest.raises(ValueError, match="outside 0 .. 32"):
        History(1).resolve(52, 33)


def test_trainer_refuses_before_touching_a_device():
    from mocca_envs_amd.history import History
    from mocca_envs_amd.trainer_api import TorchVecEnv
    with pytest.raises(NotImplementedError, match="history with terminal_observation=True"):
        TorchVecEnv("Walker3DCustomEnv-v0", 4, history=History(2), terminal_observation=True)
    with pytest.raises(NotImplementedError, match="history needs one handle"):
        TorchVecEnv("Walker3DCustomEnv-v0", 4, history=History(2), sub_batches=2)


def test_multi_handle_wrappers_refuse():
    from mocca_envs_amd.multi import ShardedVecEnv, SubBatchedVecEnv
    for cls in (SubBatchedVecEnv, ShardedVecEnv):
        multi = object.__new__(cls)
        multi.parts = []
        for name in ("set_history", "history"):
            with pytest.raises(NotImplementedError, match="needs one handle"):
                getattr(multi, name)()
