"""The per-env adaptive curriculum on the GPU (include/mocca.h mocca_set_curriculum .. mocca_curriculum_apply): the kernel BY BITS against the
numpy restatement (tests/curriculum_reference.py, which tests/test_curriculum.py holds to the header) on synthetic streams; twin handles on
real physics, one with the rule's launch behind its steps, one plain whose levels the test moves with the restatement and mocca_set_param_v;
a captured graph; the trainer's surface; refusals; and a handle with nothing attached against the parent's recording.  Everything compared
is integers and whole f32 numbers: bit for bit, no tolerance.  N = 300 where the kernel's ragged last workgroup matters (256 + 44), 64
elsewhere."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import curriculum_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mocca_envs_amd import lib as L  # noqa: E402
from mocca_envs_amd import model as M  # noqa: E402
from mocca_envs_amd.curriculum import Curriculum  # noqa: E402
from mocca_envs_amd.vec_env import VecEnv  # noqa: E402

SEED = 0
STEPPER, CUSTOM = "Walker3DStepperEnv-v0", "Walker3DCustomEnv-v0"
POLICY = os.path.join(HERE, "golden", "ppo_policy_stepper_base_controller.npz")
# arm three and the captured graph: the thresholds of the trained policy's run, chosen from what the PLAIN handle shows (see the docstring of
# test_twin_handles_trained_policy)
TRAINED = dict(promote_at=3, demote_at=2, patience=1, min_level=0, max_level=9, recycle=False)
TRAINED_STEPS, TRAINED_START = 600, 5


def cfg(promote_at, demote_at, patience=1, min_level=0, max_level=9, recycle=False):
    return dict(promote_at=promote_at, demote_at=demote_at, patience=patience, min_level=min_level, max_level=max_level, recycle=int(recycle))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _same(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _env(n, env_id=STEPPER, **kw):
    return VecEnv(env_id, n, device=0, seed=SEED, **kw)


def _near_timeout(env, every=3, left=2):
    """envs 0, every, 2 every, ..: `left` steps before the TimeLimit, so that episodes end inside a short test"""
    tk = env.get_task().clone()
    tk[::every, M.TW.T] = int(env.model.max_episode_steps) - left
    env.set_task(tk)


def _episodes(env):
    """the episode counter of every env as the task record holds it now: what a recycle draw is keyed by"""
    return _np(env.get_task())[:, M.TW.EPISODE].astype(np.int32).view(np.uint32)


def _state_agrees(env, rule, totals, what):
    st = env.curriculum_state()
    torch.cuda.synchronize()
    assert _same(st["level"], rule.levels()), (what, "levels")
    assert _same(st["streak"], rule.streak), (what, "streaks")
    assert _same(st["hold"], rule.hold), (what, "holds")
    assert _same(totals, rule.totals), (what, "totals")


# ---- 5. synthetic streams ---------------------------------------------------------------------------------------------------------------
STREAM_N, STREAM_LAUNCHES = 300, 200
STREAM_CONFIGS = {      # tests/test_curriculum.py's: name -> (configuration, start levels, written raw after attaching?)
    "patience1": (cfg(12, 5), 0, False),
    "patience3_recycle": (cfg(9, 8, 3, recycle=True), 5, False),
    "patience1_recycle": (cfg(8, 3, recycle=True), 7, False),
    "pinned": (cfg(10, 9, 2, 4, 4, True), 4, False),
    "band_3_6": (cfg(10, 7, 2, 3, 6, True), None, True),      # starts OUTSIDE the band, at the raw levels 0 and 9 a host write leaves
}


@pytest.mark.parametrize("name", list(STREAM_CONFIGS))
def test_apply_equals_the_restatement_on_synthetic_streams(name):
    """mocca_curriculum_apply, the very kernel the step launches, on 300 envs x 200 launches of random (done, info): levels, streaks, holds and
    totals after every launch.  The episode counters are the handle's own (no step runs: they stay where reset left them), the seed key
    and the env offset are not the defaults."""
    c, start, raw = STREAM_CONFIGS[name]
    n, offset, seed = STREAM_N, 1000, 0x0123456789ABCDEF
    env = VecEnv(STEPPER, n, device=0, seed=seed, env_offset=offset, auto_reset=False)
    env.reset()
    if start is not None:
        env.set_param_v(L.PARAM_CURRICULUM, [float(start)], broadcast=True)
    totals = env.set_curriculum(Curriculum(**c))
    levels = np.where(np.arange(n) % 2, 9, 0).astype(np.float32) if raw else R.start_levels(c, np.full(n, start, np.float32))
    if raw:
        env.set_param_v(L.PARAM_CURRICULUM, levels)
    rule = R.Rule(c, levels, seed, offset)
    episode = _episodes(env)
    assert (episode == 0).all()
    _state_agrees(env, rule, totals, "start")
    moved = 0
    for k, (done, info, _, _) in enumerate(R.stream(n, STREAM_LAUNCHES)):
        before = rule.levels()
        rule(done, info, episode)
        env.curriculum_apply(torch.from_numpy(done).cuda(), torch.from_numpy(info).cuda())
        _state_agrees(env, rule, totals, k)
        moved += int((rule.levels() != before).sum())
    assert (moved == 0 if c["min_level"] == c["max_level"] else moved > 2 * n) and rule.totals[:, 0].sum() > 20 * n
    env.close()


def test_attach_starts_from_the_scalar_or_the_vector_clamped_into_the_band():
    n = 300
    env = _env(n)
    env.set_param(L.PARAM_CURRICULUM, 8)
    env.set_curriculum(Curriculum(5, 1, min_level=2, max_level=6))
    assert (_np(env.curriculum_levels()) == 6).all()                                    # the scalar level, clamped
    env.set_curriculum(None)
    per_env = (np.arange(n) % 10).astype(np.float32)
    env.set_param_v(L.PARAM_CURRICULUM, per_env + 0.75)                                 # (a word is read truncated)
    env.set_curriculum(Curriculum(5, 1, min_level=2, max_level=6))
    st = env.curriculum_state()
    assert _same(st["level"], np.clip(per_env, 2, 6).astype(np.int32)) and not _np(st["streak"]).any() and not _np(st["hold"]).any()
    env.close()


# ---- 6. twin handles, real physics ------------------------------------------------------------------------------------------------------
def _twins(c, start, steps, drive, n=64, prepare=None, verbose=None):
    """Handle A has the curriculum attached; handle B is plain: after each step the restated rule runs on B's own done / info and the levels
    go to B with set_param_v -- B runs no new code.  obs, rew, done, info and the levels are compared bit for bit at every step.
    -> (the restatement, B's promotions, demotions, recycles, episodes ended)"""
    A, B = _env(n), _env(n)
    for e in (A, B):
        e.set_param_v(L.PARAM_CURRICULUM, [float(start)], broadcast=True)
        if prepare:
            prepare(e)
    totals = A.set_curriculum(Curriculum(**c))
    rule = R.Rule(c, R.start_levels(c, np.full(n, start, np.float32)), SEED, 0)
    A.reset(), B.reset()
    assert _same(A.obs, B.obs)
    ups = downs = recycles = ended = 0
    for t in range(steps):
        drive(A, t), drive(B, t)
        done = _np(B.done)
        if done.any():
            before, info = rule.levels().astype(np.int64), _np(B.info)
            rule(done, info, _episodes(B))
            B.set_param_v(L.PARAM_CURRICULUM, rule.level)
            moved, ok = rule.levels() != before, info >= c["promote_at"]       # (a level only moves in an env that was judged)
            ups += int((moved & ok & (before < c["max_level"])).sum())
            recycles += int((moved & ok & (before == c["max_level"])).sum())
            downs += int((moved & ~ok).sum())
            ended += int((done != 0).sum())
            if verbose is not None:
                verbose.append((t, [(int(l), int(s)) for l, s in zip(before[done != 0], _np(B.info)[done != 0])]))
        for what, x, y in (("obs", A.obs, B.obs), ("rew", A.rew, B.rew), ("done", A.done, B.done), ("info", A.info, B.info)):
            assert _same(x, y), (t, what)
        assert _same(A.curriculum_levels(), rule.levels()), (t, "levels")
    _state_agrees(A, rule, totals, "end")
    for what, x, y in (("state", A.get_state(), B.get_state()), ("task", A.get_task(), B.get_task()), ("terrain", A.get_terrain(), B.get_terrain())):
        assert _same(x, y), ("end", what)
    A.close(), B.close()
    return rule, ups, downs, recycles, ended


def _torques(n, steps, act_dim=21, seed=1):
    a = torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (steps, n, act_dim)).astype(np.float32)).cuda()
    return lambda env, t: env.step(a[t])


def test_twin_handles_random_torques_every_episode_fails():
    """arm one: start level 5 by broadcast, promote_at 21 and demote_at 20 -- steps_reached never exceeds 20, so every judged episode is a
    failure: the levels walk down to min_level, every other episode held"""
    steps, n = 400, 64
    rule, ups, downs, recycles, ended = _twins(cfg(21, 20, min_level=3), 5, steps, _torques(n, steps))
    print("arm one: episodes ended", ended, "demotions", downs, "levels", np.bincount(rule.levels(), minlength=10).tolist())
    assert ups == 0 and recycles == 0 and rule.totals[:, 2].sum() == 0 and rule.totals[:, 3].sum() == rule.totals[:, 0].sum()
    assert (rule.levels() <= 5).all() and (rule.levels() >= 3).all() and (rule.levels() == 3).any()
    assert downs == int((5 - rule.levels()).sum())                                       # a demotion is one level
    assert rule.totals[:, 0].sum() == ended - (downs - rule.hold.sum())                  # every move exempts exactly one later episode


def test_twin_handles_random_torques_every_episode_succeeds():
    """arm two: start level 0, promote_at 0 and demote_at -1 with recycle in the band [0, 1]: every judged episode is a success, so the levels
    walk up and recycle"""
    steps, n = 400, 64
    rule, ups, downs, recycles, ended = _twins(cfg(0, -1, max_level=1, recycle=True), 0, steps, _torques(n, steps))
    print("arm two: episodes ended", ended, "promotions", ups, "recycles", recycles, "levels", np.bincount(rule.levels(), minlength=10).tolist())
    assert downs == 0 and ups >= 1 and recycles >= 1 and rule.totals[:, 3].sum() == 0 and rule.totals[1, 0] > 0
    assert (rule.levels() <= 1).all() and rule.totals[:, 2].sum() == rule.totals[:, 0].sum()


def _trained(env):
    from mocca_envs_amd.policy import DevicePolicy
    env.set_policy(DevicePolicy.from_npz(POLICY))


def test_twin_handles_trained_policy():
    """arm three: the policy of tests/golden/ppo_policy_stepper_base_controller.npz, trained at level 0, through act_step with the kernel's own
    noise, 600 steps from level 5.  The thresholds -- promote_at 3, demote_at 2, patience 1: every judged episode is a success or a failure
    -- are chosen from what the PLAIN handle B, which is existing code only, shows: at level 5 the level-0 policy ends its episodes after 60 to
    120 steps with steps_reached 2, 3 or 4, about one in three of them at 2, so 3 / 2 splits them.  Under these thresholds B ended 350
    episodes in the 600 steps, with 134 promotions and 51 demotions, and finished spread over the levels 3 .. 9 (1, 8, 6, 25, 5, 18, 1 envs).
    The test asserts on B that it saw at least one promotion and one demotion."""
    log = []
    rule, ups, downs, recycles, ended = _twins(TRAINED, TRAINED_START, TRAINED_STEPS, lambda env, t: env.act_step(env.obs), prepare=_trained, verbose=log)
    print("arm three: episodes ended", ended, "promotions", ups, "demotions", downs, "levels", np.bincount(rule.levels(), minlength=10).tolist())
    print("arm three: (level, steps_reached) of the episodes that ended, by step:", log)
    assert ups >= 1 and downs >= 1, (ups, downs)


# ---- 7. a captured graph ----------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_replays_the_rule_like_eager():
    """arm three's loop, six act_steps to a graph, captured after attaching and replayed a hundred times on the default queue settings: the
    rule's launch is part of the graph, and every replay leaves what the uncaptured twin leaves"""
    n, per = 64, 6
    E_, G_ = _env(n), _env(n)
    totals = {}
    for name, e in (("E", E_), ("G", G_)):
        _trained(e)
        e.set_param(L.PARAM_CURRICULUM, TRAINED_START)
        totals[name] = e.set_curriculum(Curriculum(**TRAINED))
        e.reset()

    def some(e):
        for _ in range(per):
            e.act_step(e.obs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        some(G_)                                             # warm-up ahead of the capture, as torch requires
    torch.cuda.current_stream().wait_stream(side)
    some(E_)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        some(G_)                                             # (a capture records the launches; nothing runs)
    moved = False
    for t in range(TRAINED_STEPS // per - 1):
        graph.replay()
        some(E_)
        se, sg = E_.curriculum_state(), G_.curriculum_state()
        torch.cuda.synchronize()
        for what, x, y in (("obs", E_.obs, G_.obs), ("rew", E_.rew, G_.rew), ("done", E_.done, G_.done), ("info", E_.info, G_.info),
                           ("level", se["level"], sg["level"]), ("streak", se["streak"], sg["streak"]), ("hold", se["hold"], sg["hold"]),
                           ("totals", totals["E"], totals["G"])):
            assert _same(x, y), (t, what)
        moved = moved or bool((_np(sg["level"]) != TRAINED_START).any())
    assert moved and float(totals["G"][:, 0].sum()) > 0, "no level moved inside the graph"
    assert _same(E_.get_state(), G_.get_state()) and _same(E_.get_task(), G_.get_task()) and _same(E_.get_terrain(), G_.get_terrain())
    E_.close(), G_.close()


# ---- 8. the trainer's surface -----------------------------------------------------------------------------------------------------------
def test_trainer_surface_levels_totals_and_step_into():
    """make_vec_envs(curriculum=...): first with thresholds no episode meets (promote_at 21, demote_at -1: the rule's launch runs behind every
    step and counts, no level moves), so that step(into=...) must fill the trainer's rows exactly as a plain twin's does; then with levels
    that move, against the restatement"""
    from mocca_envs_amd.trainer_api import make_vec_envs
    n, steps = 64, 120
    act = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, (steps, n, 21)).astype(np.float32)).cuda()
    f32 = dict(dtype=torch.float32, device="cuda")
    rows = lambda: dict(obs=torch.zeros(n, 65, **f32), reward=torch.zeros(n, 1, **f32), masks=torch.zeros(n, 1, **f32), bad_masks=torch.zeros(n, 1, **f32))
    still, plain = make_vec_envs(STEPPER, SEED, n, curriculum=Curriculum(21, -1)), make_vec_envs(STEPPER, SEED, n)
    assert plain.curriculum_totals is None and tuple(still.curriculum_totals.shape) == (10, 4) and still.curriculum_levels.dtype == torch.int32
    with pytest.raises(L.MoccaError, match="curriculum_levels needs curriculum="):
        plain.curriculum_levels
    into_s, into_p = rows(), rows()
    assert _same(still.reset(), plain.reset())
    _near_timeout(still.venv), _near_timeout(plain.venv)
    ended = 0
    for t in range(steps // 2):
        still.step(act[t], into=into_s), plain.step(act[t], into=into_p)
        torch.cuda.synchronize()
        ended += int((_np(still.venv.done) != 0).sum())
        for k in into_s:
            assert _same(into_s[k], into_p[k]), (t, k)
    assert ended >= n // 3 and not _np(still.curriculum_levels).any()
    assert _np(still.curriculum_totals)[0, 0] == ended and _np(still.curriculum_totals)[:, 2:].sum() == 0        # counted, never judged either way
    still.venv.close(), plain.venv.close()

    c = cfg(0, -1, max_level=3, recycle=True)
    envs = make_vec_envs(STEPPER, SEED, n, curriculum=Curriculum(**c))
    rule = R.Rule(c, np.zeros(n, np.float32), SEED, 0)
    into = rows()
    envs.reset()
    _near_timeout(envs.venv)
    for t in range(steps):
        envs.step(act[t], into=into)
        done = _np(envs.venv.done)
        if done.any():
            rule(done, _np(envs.venv.info), _episodes(envs.venv))
    assert _same(envs.curriculum_levels, rule.levels()) and _same(envs.curriculum_totals, rule.totals)
    assert rule.levels().any() and rule.totals[:, 0].sum() >= n // 3
    with pytest.raises(L.MoccaError, match="mocca_set_param_v with broadcast"):
        envs.set_env_params({"curriculum": 3})
    envs.curriculum_totals.zero_()                        # the caller's to zero
    torch.cuda.synchronize()
    assert float(envs.curriculum_totals.sum()) == 0
    envs.venv.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_detach():
    n = 64
    lib = L.load()
    custom = _env(4, CUSTOM)
    with pytest.raises(L.MoccaError, match="only MOCCA_TASK_WALKER3D_STEPPER has curriculum levels"):
        custom.set_curriculum(Curriculum(5, 1))
    custom.close()
    for env_id in ("MikeStepperEnv-v0", "LaikagoStepperEnv-v0"):                       # that task: accepted
        e = _env(4, env_id)
        e.set_curriculum(Curriculum(5, 1))
        e.close()
    A, B = _env(n), _env(n)
    # nothing attached: the getters and the explicit launch need an attachment
    d, i = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    for call in (lambda: lib.mocca_get_curriculum(A.h, None, None, None, None), lambda: lib.mocca_curriculum_apply(A.h, C.c_void_p(d.data_ptr()), C.c_void_p(i.data_ptr()), None)):
        assert call() == -1 and "needs a curriculum (mocca_set_curriculum)" in lib.mocca_last_error(A.h).decode()
    for bad, said in ((dict(promote_at=5, demote_at=5), "demote_at must be smaller than promote_at"),
                      (dict(promote_at=5, demote_at=1, patience=0), "patience must be 1 .. 64"),
                      (dict(promote_at=5, demote_at=1, patience=65), "patience must be 1 .. 64"),
                      (dict(promote_at=5, demote_at=1, min_level=-1), "the levels must satisfy 0 <= min_level <= max_level <= 9"),
                      (dict(promote_at=5, demote_at=1, max_level=10), "the levels must satisfy 0 <= min_level <= max_level <= 9"),
                      (dict(promote_at=5, demote_at=1, min_level=7, max_level=6), "the levels must satisfy 0 <= min_level <= max_level <= 9"),
                      (dict(promote_at=5, demote_at=1, recycle=2), "recycle must be 0 or 1")):
        raw = L.CurriculumConfig(**{**dict(patience=1, min_level=0, max_level=9, recycle=0), **bad})
        assert lib.mocca_set_curriculum(A.h, C.byref(raw), None) == -1
        assert lib.mocca_last_error(A.h).decode() == "mocca_set_curriculum: " + said
    A.set_param(L.PARAM_CURRICULUM, 2)                                                  # the refused calls attached nothing: the scalar is taken
    A.set_curriculum(Curriculum(5, 1))
    with pytest.raises(L.MoccaError, match="mocca_set_param_v with broadcast"):
        A.set_param(L.PARAM_CURRICULUM, 3)
    with pytest.raises(L.MoccaError, match="mocca_set_param_v with broadcast"):
        A.set_env_params({"curriculum": 3})
    assert lib.mocca_curriculum_apply(A.h, None, C.c_void_p(i.data_ptr()), None) == -1 and "done_dev or info_dev is NULL" in lib.mocca_last_error(A.h).decode()
    A.set_param_v(L.PARAM_CURRICULUM, [7.0], broadcast=True)                            # the per-env form keeps working
    assert (_np(A.curriculum_levels()) == 7).all()
    # detach restores the scalar path: a step after it is the step of a handle that never attached
    A.set_curriculum(None)
    with pytest.raises(L.MoccaError, match="needs a Curriculum"):
        A.curriculum_levels()
    A.set_param(L.PARAM_CURRICULUM, 3), B.set_param(L.PARAM_CURRICULUM, 3)
    A.reset(), B.reset()
    _near_timeout(A), _near_timeout(B)
    act = torch.from_numpy(np.random.default_rng(2).uniform(-1.0, 1.0, (40, n, 21)).astype(np.float32)).cuda()
    ended = 0
    for t in range(40):
        A.step(act[t]), B.step(act[t])
        ended += int((_np(B.done) != 0).sum())
        for what, x, y in (("obs", A.obs, B.obs), ("rew", A.rew, B.rew), ("done", A.done, B.done), ("info", A.info, B.info)):
            assert _same(x, y), (t, what)
    assert _same(A.get_terrain(), B.get_terrain()) and _same(A.get_task(), B.get_task()) and ended >= 1
    A.close(), B.close()


def test_auto_reset_off_launches_nothing_and_a_null_info_goes_to_the_handles_buffer():
    """with auto-reset off the step launches no rule (done is sticky there); with it on and info_dev NULL the step's info words go to a
    buffer of the handle's and the rule reads them: the same levels as a twin that passes its own"""
    n, steps = 64, 120
    lib = L.load()
    off = _env(n, auto_reset=False)
    totals = off.set_curriculum(Curriculum(0, -1))
    off.reset()
    _near_timeout(off)
    act = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, (steps, n, 21)).astype(np.float32)).cuda()
    for t in range(steps):
        off.step(act[t])
    assert _np(off.done).any() and not _np(off.curriculum_levels()).any() and float(totals.sum()) == 0
    off.close()
    A, B = _env(n), _env(n)
    ta, tb = A.set_curriculum(Curriculum(0, -1)), B.set_curriculum(Curriculum(0, -1))
    A.reset(), B.reset()
    _near_timeout(A), _near_timeout(B)
    for t in range(steps):
        A.step(act[t])
        L.check(lib.mocca_step(B.h, C.c_void_p(act[t].data_ptr()), C.c_void_p(B.obs.data_ptr()), C.c_void_p(B.rew.data_ptr()), C.c_void_p(B.done.data_ptr()),
                               None, B._stream()), B.h)
    sa, sb = A.curriculum_state(), B.curriculum_state()
    for k in sa:
        assert _same(sa[k], sb[k]), k
    assert _same(ta, tb) and _same(A.obs, B.obs) and _np(sa["level"]).any()
    A.close(), B.close()


# ---- 10. nothing attached ---------------------------------------------------------------------------------------------------------------
def test_nothing_attached_is_the_parents_recording():
    """the Stepper case of the parent's recording (tests/golden/step_bits5_stepper.json: one SHA-256 per step over the state and the step's
    outputs, recorded from the library before this feature), replayed while another handle of the process has a curriculum attached"""
    spec = importlib.util.spec_from_file_location("record_step_bits5", os.path.join(os.path.dirname(HERE), "tools", "record_step_bits5.py"))
    rsb5 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rsb5)
    other = _env(8)
    other.set_curriculum(Curriculum(5, 1))
    with open(rsb5.golden_path("stepper")) as f:
        want = json.load(f)
    got = rsb5.record("stepper")
    assert got["hashes"] == want["hashes"] and got["auto_resets"] == want["auto_resets"] and got["lds_bytes"] == want["lds_bytes"]
    other.close()
