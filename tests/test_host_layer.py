"""The Python host layer without a GPU: the one bracket every streamed library call of `VecEnv` goes through, the one rule by which
`TorchVecEnv` hands calls to its single handle, the rows `TorchVecEnv` fills and the order of the launches that fill them, the one rule
for rows that are views of wider storage, and the one list of what sub-batched and sharded batches refuse."""
import ctypes as C
import itertools
import json
import os
import re
from types import SimpleNamespace

import pytest
import torch

from mocca_envs_amd import lib as _lib
from mocca_envs_amd import multi, rollout, trainer_api
from mocca_envs_amd.vec_env import VecEnv


class _Stream:
    """stands in for a torch.cuda.Stream: records what it is asked to wait for"""

    def __init__(self, name, handle, events):
        self.name, self.cuda_stream, self.events = name, handle, events

    def wait_stream(self, other):
        self.events.append(("wait", self.name, other.name))

    def synchronize(self):
        self.events.append(("sync", self.name))


@pytest.fixture
def handle(monkeypatch):
    """a VecEnv that never saw a device, its pinned and torch's current stream, the event log and a library function that records its call"""
    events = []
    pinned, current = _Stream("pinned", 0x1000, events), _Stream("current", 0x2000, events)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: current)
    monkeypatch.setattr(_lib, "load", lambda: type("Lib", (), {"mocca_last_error": staticmethod(lambda h: b"boom")})())
    env = object.__new__(VecEnv)
    env.h, env.device, env.stream = "HANDLE", torch.device("cpu"), pinned
    rc = [0]

    def fn(*args):
        events.append(("call",) + args)
        return rc[0]
    yield env, events, fn, rc
    env.h = None        # (nothing for close() to destroy)


WAIT_IN, WAIT_OUT, SYNC = ("wait", "pinned", "current"), ("wait", "current", "pinned"), ("sync", "pinned")


@pytest.mark.parametrize("kw, before, after", [
    ({}, [WAIT_IN], [WAIT_OUT]),                                  # nearly every call
    ({"then": "sync"}, [WAIT_IN], [SYNC]),                        # set_state, set_task, set_terrain, task_step
    ({"wait": False}, [], [WAIT_OUT]),                            # base_outputs; the second call of _download
    ({"wait": False, "then": None}, [], []),                      # the first call of _download
])
def test_call_brackets_the_library_call_on_a_pinned_stream(handle, kw, before, after):
    env, events, fn, _ = handle
    t = torch.arange(3, dtype=torch.float32)
    env._call(fn, t, None, 5, 0.25, **kw)
    assert [e[:1] if e[0] == "call" else e for e in events] == before + [("call",)] + after
    h, ptr, none, i, f, stream = next(e for e in events if e[0] == "call")[1:]
    assert h == "HANDLE" and isinstance(ptr, C.c_void_p) and ptr.value == t.data_ptr()
    assert none is None and (i, f) == (5, 0.25)
    assert isinstance(stream, C.c_void_p) and stream.value == 0x1000           # the handle's own stream, last


def test_call_on_the_current_stream_orders_nothing(handle):
    env, events, fn, _ = handle
    env.stream = None
    env._call(fn, 1)
    env._call(fn, 2, then="sync")
    assert [e[0] for e in events] == ["call", "call", "sync"] and events[2] == ("sync", "current")
    assert [e[1:3] for e in events[:2]] == [("HANDLE", 1), ("HANDLE", 2)] and all(e[3].value == 0x2000 for e in events[:2])


def test_call_raises_the_library_s_error_before_anything_waits_for_it(handle):
    env, events, fn, rc = handle
    rc[0] = 3
    with pytest.raises(_lib.MoccaError, match="error 3: boom"):
        env._call(fn, torch.zeros(1))
    assert [e[0] for e in events] == ["wait", "call"]


def test_a_streamed_method_goes_through_the_bracket(handle):
    """one real caller end to end: observe() is _in, mocca_observe(handle, obs, stream), _out"""
    env, events, fn, _ = handle
    env.obs, env.lib = torch.zeros(2, 4), type("Lib", (), {"mocca_observe": staticmethod(fn)})()
    assert env.observe() is env.obs
    assert events[0] == WAIT_IN and events[2] == WAIT_OUT and events[1][0] == "call"
    assert events[1][2].value == env.obs.data_ptr() and events[1][3].value == 0x1000 and len(events[1]) == 4


# ---- TorchVecEnv: the one-handle rule ------------------------------------------------------------------------------------------------
GUARDED = {"attach_policy": (None,), "attach_teacher": (None,), "capture_rollout": ()}      # guard first, then work of their own


def test_every_forwarded_name_refuses_a_batch_without_one_handle():
    envs = object.__new__(trainer_api.TorchVecEnv)
    envs.venv = object()                 # no `lib`: what a sub-batched or sharded batch looks like
    assert len(trainer_api._FORWARDED) == 11
    for name, args in list(GUARDED.items()) + [(n, ()) for n in trainer_api._FORWARDED]:
        assert name in vars(trainer_api.TorchVecEnv)                         # a real attribute of the class, not __getattr__
        with pytest.raises(NotImplementedError, match=f"{name} needs one handle"):
            getattr(envs, name)(*args)


def test_every_forwarded_name_is_a_method_of_vecenv_and_reaches_it():
    for name in trainer_api._FORWARDED:
        assert callable(getattr(VecEnv, name))
        doc = getattr(trainer_api.TorchVecEnv, name).__doc__
        assert f"`VecEnv.{name}`" in doc and doc.endswith("One handle only.")
    seen = []
    venv = type("Venv", (), {"lib": None, "ppo_grad": lambda self, *a, **k: seen.append((a, k)) or "result"})()
    envs = object.__new__(trainer_api.TorchVecEnv)
    envs.venv = venv
    assert envs.ppo_grad(1, 2, clip=0.1) == "result" and seen == [((1, 2), {"clip": 0.1})]


# ---- TorchVecEnv: the rows and the launches that fill them ------------------------------------------------------------------------------
# The order of the launches behind a reset or a step, and the slices they get, are a contract: the GPU suites compare bits and a captured
# rollout bakes the order into its graph.  A fake handle on CPU tensors logs every call; the expected logs are tests/golden/
# trainer_rows_trace.json, recorded by this code (`python tests/test_host_layer.py` rewrites it).
TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_rows_trace.json")
N, OBS, ACT, SCAN, PRIV_SCAN, DEPTH, HIST = 2, 7, 3, 5, 4, 6, 8


class _FakeHandle:
    """what TorchVecEnv asks of a VecEnv, on CPU tensors: every call is logged with its tensor arguments (storage, shape, storage offset,
    row stride); the launches move the observation's head as the real ones do, so a row shows whose observation it holds"""
    lib, base_controller, plan_dim, task_id, hist = None, None, 0, -1, None

    def __init__(self, log):
        self.log, self.n_envs, self.obs_dim, self.act_dim, self.device = log, N, OBS, ACT, torch.device("cpu")
        self.obs, self.rew, self.done = torch.zeros(N, OBS), torch.zeros(N), torch.zeros(N, dtype=torch.uint8)
        self.info = torch.zeros(N, dtype=torch.int32)
        self.scan_dim = self.depth_dim = self.history_dim = self.launches = 0

    def _log(self, name, **kw):
        self.log.append([name] + [[k, [t.untyped_storage().data_ptr(), list(t.shape), t.storage_offset(), t.stride(0)]
                                   if isinstance(t, torch.Tensor) else None if t is None else type(t).__name__] for k, t in kw.items()])

    def set_height_scan(self, points, z_above=1.0, max_drop=2.0):
        self._log("set_height_scan", points=points)
        self.scan_dim = len(points)

    def set_depth_camera(self, cam):
        self._log("set_depth_camera", cam=cam)
        self.depth_dim = cam.pixels

    def set_randomisation(self, rand):
        self._log("set_randomisation", rand=rand)

    def set_history(self, hist):
        self._log("set_history", hist=hist)
        self.history_dim = hist.dim

    def set_policy(self, policy):
        self._log("set_policy", policy=policy)

    def episode_stats(self, on, slots=4):
        self._log("episode_stats")
        return dict(masks=torch.ones(N), bad_masks=torch.ones(N), totals=torch.zeros(4), records=torch.zeros(slots, N, 4, dtype=torch.int32),
                    slots=slots, first_serial=1)

    def _new_obs(self, obs):
        self.launches += 1
        obs.fill_(float(self.launches))
        return obs

    def reset(self):
        self._log("reset")
        return self._new_obs(self.obs)

    def step(self, actions, obs_out=None, rew_out=None):
        self._log("step", actions=actions, obs_out=obs_out, rew_out=rew_out)
        return self._new_obs(self.obs if obs_out is None else obs_out), self.rew if rew_out is None else rew_out, self.done, self.info

    def act_step(self, obs, action_out=None, logp_out=None, value_out=None, obs_out=None, rew_out=None):
        self._log("act_step", obs=obs, action_out=action_out, logp_out=logp_out, value_out=value_out, obs_out=obs_out, rew_out=rew_out)
        return self._new_obs(self.obs if obs_out is None else obs_out), self.rew if rew_out is None else rew_out, self.done, self.info

    def _sensor(self, name, out, obs):
        self._log(name, out=out, obs=obs)
        if obs is not None:
            out[:, :OBS].copy_(obs)
        return out

    def height_scan(self, out=None, obs=None):
        return self._sensor("height_scan", out, obs)

    def depth_camera(self, out=None, obs=None):
        return self._sensor("depth_camera", out, obs)

    def sensor_noise(self, rows, out=None):
        self._log("sensor_noise", rows=rows, out=out)
        if out is not None:
            out[:, :OBS].copy_(rows[:, :OBS])
        return rows if out is None else out

    def randomisation_record(self, out=None):
        self._log("randomisation_record", out=out)
        return out

    def history(self, rows, act=None, out=None):
        self._log("history", rows=rows, act=act, out=out)
        return out

    def close(self):
        pass


def _row_options():
    """(key, TorchVecEnv keywords) of every admissible combination of the options that shape the rows"""
    for scan, depth, hist in itertools.product(("", "scan", "priv_scan"), (False, True), (False, True)):
        for rand in ("", "rand", "rand+noise") + (("rand+priv", "rand+priv+noise") if scan == "priv_scan" else ()):
            kw = {}
            if scan:
                kw["height_scan" if scan == "scan" else "privileged_scan"] = dict(points=[[0.0, 0.0]] * (SCAN if scan == "scan" else PRIV_SCAN))
            if depth:
                kw["depth_camera"] = SimpleNamespace(pixels=DEPTH)
            if hist:
                kw["history"] = SimpleNamespace(dim=HIST)
            if rand:
                kw["randomisation"] = SimpleNamespace(privileged="priv" in rand, obs_noise=[0.1] * OBS if "noise" in rand else None)
            yield "|".join(x for x in (scan, "depth" * depth, "hist" * hist, rand) if x) or "plain", kw


def _trace_rows(kw) -> dict:
    """construct a TorchVecEnv over a fake handle and log reset(), step(), step(into=) and act_step()"""
    log = []
    real, trainer_api.make_vec_env = trainer_api.make_vec_env, lambda *a, **k: _FakeHandle(log)
    try:
        envs = trainer_api.TorchVecEnv("Walker3DCustomEnv-v0", N, record_events=False, **kw)
    finally:
        trainer_api.make_vec_env = real
    width = envs.observation_space.shape[0]
    names = {}             # storage -> what it is; the first name a storage gets stays (`randomisation` may be the privileged row's tail)
    into, actions = {"obs": torch.zeros(N, width), "reward": torch.zeros(N, 1)}, torch.zeros(N, ACT)

    def name(**tensors):
        for k, t in tensors.items():
            if t is not None:
                names.setdefault(t.untyped_storage().data_ptr(), k)

    name(**{"venv.obs": envs.venv.obs, "venv.rew": envs.venv.rew, "wide": envs._wide, "privileged": envs.privileged,
            "randomisation": envs.randomisation, "into.obs": into["obs"], "into.reward": into["reward"], "actions": actions})
    out = {"observation_space": list(envs.observation_space.shape), "privileged": None if envs.privileged is None else list(envs.privileged.shape),
           "randomisation": None if envs.randomisation is None else list(envs.randomisation.shape)}

    def phase(key, call):
        start = 0 if key == "init" else len(log)       # "init": what the constructor asked of the handle
        obs = call()
        obs = obs[0] if isinstance(obs, tuple) else obs
        if key == "act_step":
            name(**{"last_act." + k: t for k, t in envs.last_act.items()})
        calls = [[c[0]] + [[k, a if not isinstance(a, list) else [names.get(a[0], "other")] + a[1:]] for k, a in c[1:]] for c in log[start:]]
        # what came back: which tensor, and that its head is the observation of THIS launch
        out[key] = {"calls": calls, "returns": [names.get(obs.untyped_storage().data_ptr(), "other"), list(obs.shape), obs.storage_offset()],
                    "head_is_this_launch": bool((obs[:, :OBS] == float(envs.venv.launches)).all())}

    phase("init", lambda: envs.venv.obs)
    phase("reset", envs.reset)
    phase("step", lambda: envs.step(actions))
    phase("step_into", lambda: envs.step(actions, into=into))
    envs.attach_policy(SimpleNamespace(in_dim=width, act_dim=ACT, asymmetric=False))
    phase("act_step", envs.act_step)
    return out


ROW_OPTIONS = dict(_row_options())


def test_there_are_44_admissible_row_combinations():
    assert len(ROW_OPTIONS) == 44


@pytest.mark.parametrize("key", list(ROW_OPTIONS))
def test_trainer_rows_launch_order_and_slices(key):
    with open(TRACE) as f:
        want = json.load(f)[key]
    kw = ROW_OPTIONS[key]
    got = json.loads(json.dumps(_trace_rows(kw)))
    scan = SCAN if "height_scan" in kw else 0
    assert got["observation_space"] == [OBS + scan + DEPTH * ("depth_camera" in kw) + HIST * ("history" in kw)]
    rand = kw.get("randomisation")
    assert got["privileged"] == (None if "privileged_scan" not in kw else [N, OBS + PRIV_SCAN + 4 * bool(rand is not None and rand.privileged)])
    assert got["randomisation"] == (None if rand is None else [N, 4])
    for phase in ("reset", "step", "step_into", "act_step"):
        assert got[phase]["head_is_this_launch"], phase
    assert got == want


# ---- the row-view rule: one helper behind every call that takes "[n, >= w] rows of wider storage" ---------------------------------------
W_OBS, W_ACT, W_SCAN, W_HIST, W_IN, W_CRITIC, W_TEACHER = 6, 2, 3, 8, 6, 9, 7


def _strided_env(n):
    """a VecEnv that never saw a device, with a policy, a teacher, a scan and a history attached as far as the checks look, and the list
    every library call lands in as (name, arguments)"""
    calls = []

    class Lib:
        mocca_scan_dim = staticmethod(lambda h: W_SCAN)
        mocca_history_dim = staticmethod(lambda h: W_HIST)

        def __getattr__(self, name):
            return lambda h, *a: calls.append((name, a)) or 0

    env = object.__new__(VecEnv)
    env.h, env.lib, env.device, env.stream, env.n_envs, env.obs_dim = None, Lib(), torch.device("cpu"), None, n, W_OBS
    env._call = lambda fn, *a, **k: fn(None, *a)
    env.policy = SimpleNamespace(in_dim=W_IN, act_dim=W_ACT, asymmetric=True, critic_in_dim=W_CRITIC)
    env.teacher = SimpleNamespace(in_dim=W_TEACHER, act_dim=W_ACT)
    env.hist, env._hist_act = object(), W_ACT
    return env, calls


def _good(n, w):
    return torch.zeros(n, w)


# site -> (least width, the ValueError's text, call(env, calls, t, n) -> the row stride handed on); `t` is the argument under test, the
# others are plain contiguous tensors
ROW_SITES = {
    "_sensor_rows": (W_SCAN, "out must be a float32 [n_envs, >= 3] tensor on the env's device with contiguous rows",
                     lambda e, c, t, n: (e.height_scan(out=t), c[-1][1][1])[1]),
    "sensor_noise.rows": (W_OBS, "rows must be a float32 [n_envs, >= 6] tensor on the env's device with contiguous rows",
                          lambda e, c, t, n: (e.sensor_noise(t, out=_good(n, W_OBS)), c[-1][1][1])[1]),
    "sensor_noise.out": (W_OBS, "out must be a float32 [n_envs, >= 6] tensor on the env's device with contiguous rows",
                         lambda e, c, t, n: (e.sensor_noise(_good(n, W_OBS), out=t), c[-1][1][3])[1]),
    "randomisation_record": (4, "out must be a float32 [n_envs, >= 4] tensor on the env's device with contiguous rows",
                             lambda e, c, t, n: (e.randomisation_record(out=t), c[-1][1][1])[1]),
    "history.rows": (W_OBS, "rows must be a float32 [n_envs, >= 6] tensor on the env's device with contiguous rows",
                     lambda e, c, t, n: (e.history(t, _good(n, W_ACT), out=_good(n, W_HIST)), c[-1][1][1])[1]),
    "history.act": (W_ACT, "act must be a float32 [n_envs, >= 2] tensor on the env's device with contiguous rows",
                    lambda e, c, t, n: (e.history(_good(n, W_OBS), t, out=_good(n, W_HIST)), c[-1][1][3])[1]),
    "history.out": (W_HIST, "out must be a float32 [n_envs, >= 8] tensor on the env's device with contiguous rows",
                    lambda e, c, t, n: (e.history(_good(n, W_OBS), None, out=t), c[-1][1][5])[1]),
    "set_critic_rows": (W_CRITIC, "the critic's rows must be a float32 [n_envs, >= 9] tensor on the env's device with contiguous rows",
                        lambda e, c, t, n: (e.set_critic_rows(t), c[-1][1][1])[1]),
    "_act_args": (W_IN, "the policy's input must be a float32 [n_envs, >= 6] tensor on the env's device with contiguous rows",
                  lambda e, c, t, n: e._act_args(t, None, False, None, True, True)[0][1]),
    "teacher_act": (W_TEACHER, "the teacher's input must be a float32 [n, >= 7] tensor on the env's device with contiguous rows",
                    lambda e, c, t, n: (e.teacher_act(t), c[-1][1][1])[1]),
    "rollout.rows_2d": (5, "rows must be a float32 [..., >= 5] tensor with a contiguous last dimension",
                        lambda e, c, t, n: rollout.rows_2d(t, 5)[1]),
}


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("site", list(ROW_SITES))
def test_row_view_rule_at_every_site(site, n):
    w, text, call = ROW_SITES[site]
    env, calls = _strided_env(n)
    wide, tall = torch.zeros(n, w + 5), torch.zeros(n + 2, w + 5)
    for t, row_stride in ((torch.zeros(n, w), w), (wide[:, :w], w + 5), (tall[1:n + 1], w + 5), (tall[1:n + 1, 2:w + 2], w + 5)):
        stride = call(env, calls, t, n)
        assert isinstance(stride, int)
        assert stride == row_stride if n > 1 else stride >= w, (site, t.shape, t.stride())       # one row: only the C side's stride >= width
    any_n = site in ("teacher_act", "rollout.rows_2d")                                           # these take any n >= 1: "wrong" is none
    bad = {"dtype": torch.zeros(n, w, dtype=torch.float64), "rows": torch.zeros(0 if any_n else n + 1, w), "columns": torch.zeros(n, w - 1),
           "transposed": torch.zeros(w, n + 1).t()[:n]}
    if n > 1:                                                                                    # (one row overlaps nothing)
        bad["overlapping"] = torch.zeros(n * w).as_strided((n, w), (w - 1, 1))
        bad["one row n times"] = torch.zeros(1, w).expand(n, w)
    for what, t in bad.items():
        before = len(calls)
        pattern = re.escape(text) if site != "rollout.rows_2d" else "rows must|the row stride"
        with pytest.raises(ValueError, match=pattern):
            call(env, calls, t, n)
        assert len(calls) == before, (site, what)                                                # refused before the library is called


# ---- multi._Parts: the one list of what needs one handle ----------------------------------------------------------------------------------
def test_every_one_handle_name_is_a_refusing_stub_of_both_wrappers():
    assert len(multi._Parts.ONE_HANDLE) == 12 and len(set(multi._Parts.ONE_HANDLE)) == 12
    for cls in (multi.SubBatchedVecEnv, multi.ShardedVecEnv):
        batch = object.__new__(cls)
        batch.parts = []
        for name in multi._Parts.ONE_HANDLE:
            assert name in vars(multi._Parts) and callable(getattr(VecEnv, name))                # a real attribute; a method of the one handle
            with pytest.raises(NotImplementedError, match=re.escape(f"{name} needs one handle (one device, sub_batches=1)")):
                getattr(batch, name)()
            with pytest.raises(NotImplementedError, match=f"{name} needs one handle"):
                getattr(batch, name)(1, 2, key=3)


if __name__ == "__main__":      # record the fixture: PYTHONPATH=. python tests/test_host_layer.py
    with open(TRACE, "w") as f:
        json.dump({key: _trace_rows(kw) for key, kw in ROW_OPTIONS.items()}, f, indent=0, sort_keys=True)
