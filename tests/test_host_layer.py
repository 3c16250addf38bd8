"""The Python host layer without a GPU: the one bracket every streamed library call of `VecEnv` goes through, and the one rule by which
`TorchVecEnv` hands calls to its single handle."""
import ctypes as C

import pytest
import torch

from mocca_envs_amd import lib as _lib
from mocca_envs_amd import trainer_api
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
