"""What a handle owns on the device (include/mocca.h mocca_set_base_controller / mocca_set_policy / mocca_set_trajectory /
mocca_set_heightfield / mocca_set_height_scan): replacing an attachment leaves the handle as a fresh one that was only given the new one, a
refused attach leaves it untouched, and a detached one is an error to use, not a crash.  Tiny batches: what can go wrong here is
ownership, not arithmetic.  Every refused call is refused on the host, before any launch."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import controller_reference as CR
import policy_reference as PR

pytestmark = pytest.mark.gpu
PLANNER, N = "Walker3DPlannerEnv-v0", 8


def _env(n=N, env_id=PLANNER, **kw):
    from mocca_envs_amd.vec_env import VecEnv
    return VecEnv(env_id, n, device=0, seed=5, **kw)


def _policy(kind, in_dim, seed):
    from mocca_envs_amd.policy import DevicePolicy
    p = PR.random_policy(kind, in_dim=in_dim, act_dim=15, seed=seed)
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def _field():
    """a second height field, of another shape and scale than the shipped one: bumps of a few centimetres around the shipped field's height
    at the origin, so that a state snapshot taken on the shipped field stands on this one too"""
    from mocca_envs_amd.terrain import load_height_field
    data, _ = load_height_field()
    z0 = float(data[data.shape[0] // 2, data.shape[1] // 2])
    return (z0 + 0.05 * np.random.default_rng(3).standard_normal((48, 56))).astype(np.float32), 2.0


def _scan(p, seed):
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (p, 2)).astype(np.float32)


def _plans(steps=3):
    import torch
    return torch.randn(steps, N, 15, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))


def _snapshot(env):
    return env.get_state().clone(), env.get_task().clone(), env.get_terrain().clone()


def _restore(env, snap):
    env.set_state(snap[0]); env.set_task(snap[1]); env.set_terrain(snap[2])
    env.observe()                      # the base controller's input is the robot part of the last observation


def _planner_outputs(env, plans):
    """3 plan_steps, the controller's outputs, a height scan and the policy's deterministic action: every tensor a copy"""
    out = []
    for plan in plans:
        out += [x.clone() for x in env.plan_step(plan)] + list(env.base_outputs())
    out.append(env.height_scan().clone())
    out += [v.clone() for _, v in sorted(env.act(env.obs, deterministic=True).items())]
    return out


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.isfinite(x.float()).all() and torch.equal(x, y), k


def test_replaced_attachments_equal_a_fresh_handle():
    """A: controller, height field, scan pattern and policy attached, used, then each replaced by one of another size.  B: a fresh handle
    that was only ever given the second of each (VecEnv itself attaches the shipped height field first).  From the same state, task and
    terrain snapshot both compute the same bits -- and not the bits A computed from that snapshot under its first attachments."""
    import torch
    ctrl = [CR.random_controller(kind, seed=2) for kind in ("small", "deep8")]
    plans = _plans()
    A = _env(base_controller=ctrl[0])
    pol = [_policy(kind, A.obs_dim, seed=4) for kind in ("small", "deep8")]
    A.set_height_scan(_scan(7, 0))
    A.set_policy(pol[0])
    A.reset()
    snap = _snapshot(A)
    before = _planner_outputs(A, plans)
    A.set_base_controller(ctrl[1])
    A.set_heightfield(*_field())
    A.set_height_scan(_scan(5, 1))
    A.set_height_scan(_scan(12, 2))
    A.set_policy(pol[0])
    A.set_policy(pol[1])
    _restore(A, snap)
    got = _planner_outputs(A, plans)
    B = _env(base_controller=ctrl[1])
    B.set_heightfield(*_field())
    B.set_height_scan(_scan(12, 2))
    B.set_policy(pol[1])
    B.reset()
    _restore(B, snap)
    _same(got, _planner_outputs(B, plans))
    assert not torch.equal(got[0], before[0]) and got[-4].shape != before[-4].shape      # the first step's observation, the scan [N, P]
    A.close(); B.close()


class _Table:
    """what VecEnv.set_trajectory takes"""

    def __init__(self, table, tmax):
        self._table, self._tmax = np.ascontiguousarray(table, np.float32), float(tmax)

    def table(self):
        return self._table

    def max_time(self):
        return self._tmax


def test_a_replaced_trajectory_equals_a_fresh_handle():
    import torch
    from mocca_envs_amd.trajectory import CassieTrajectory
    base = CassieTrajectory()
    tabs = [_Table(0.9 * base.table()[::2], base.max_time()), _Table(base.table()[::3] + np.float32(0.02), 1.1 * base.max_time())]
    n, env_id = 4, "CassiePhaseMocca2DEnv-v0"
    A = _env(n, env_id)
    acts = torch.rand(3, n, A.act_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 2 - 1

    def steps(env, snap):
        env.set_state(snap[0]); env.set_task(snap[1]); env.set_terrain(snap[2])
        return [x.clone() for a in acts for x in env.step(a)]

    A.reset()
    snap = _snapshot(A)
    A.set_trajectory(tabs[0])
    first = steps(A, snap)
    A.set_trajectory(tabs[1])
    got = steps(A, snap)
    B = _env(n, env_id)
    B.set_trajectory(tabs[1])
    B.reset()
    _same(got, steps(B, snap))
    assert not torch.equal(got[0], first[0])
    A.close(); B.close()


def test_a_refused_attach_leaves_the_handle_intact():
    """one refused call per setter on a handle that has everything attached: afterwards it computes what its twin, which never saw those
    calls, computes"""
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.controller import layer_table
    ctrl = CR.random_controller("small", seed=2)
    envs = [_env(base_controller=ctrl) for _ in range(2)]
    pol = _policy("small", envs[0].obs_dim, seed=4)
    for env in envs:
        env.set_heightfield(*_field())
        env.set_height_scan(_scan(12, 2))
        env.set_policy(pol)
        env.reset()
    env, twin = envs
    z = lambda o, i, act="tanh": (np.zeros((o, i), np.float32), np.zeros(o, np.float32), act)
    d = env.obs_dim
    two_values = SimpleNamespace(table=lambda: layer_table([z(16, d), z(15, 16)], [z(16, d), z(2, 16)]), in_dim=d, act_dim=15, clip=10.0)
    nan_scan = _scan(12, 2)
    nan_scan[7, 1] = np.nan
    for what, call in (("multiples of 16", lambda: env.set_base_controller(SimpleNamespace(actor=[z(40, 65), z(21, 40)], critic=ctrl.critic))),
                       ("the critic in 1", lambda: env.set_policy(two_values)),
                       ("not finite", lambda: env.set_height_scan(nan_scan)),
                       ("too fine", lambda: env.set_heightfield(np.zeros((64, 64), np.float32), 40)),
                       ("mocca_set_trajectory", lambda: env.set_trajectory(_Table(np.zeros((0, 32)), 1.0)))):
        with pytest.raises(L.MoccaError, match=what):
            call()
    assert env.scan_dim == 12 and env.policy is pol
    plans, act = _plans(1), torch.zeros(N, 21, device="cuda")
    _same(*[_planner_outputs(e, plans) + [x.clone() for x in e.step(act)] for e in envs])
    env.close(); twin.close()


@pytest.mark.parametrize("cycle", [0, 1])      # twice in one process: the second create follows a destroy after detach
def test_detach_then_use_is_an_error_and_destroy_follows(cycle):
    import torch
    from mocca_envs_amd import lib as L
    env = _env(base_controller=CR.random_controller("small", seed=2))
    env.set_height_scan(_scan(5, 1))
    env.set_policy(_policy("small", env.obs_dim, seed=4))
    obs = env.reset()
    env.plan_step(_plans(1)[0])
    env.set_base_controller(None)
    env.set_policy(None)
    env.set_height_scan(None)
    assert env.scan_dim == 0
    with pytest.raises(L.MoccaError, match="needs a base controller"):
        env.plan_step(_plans(1)[0])
    with pytest.raises(L.MoccaError):
        env.act(obs, deterministic=True)
    with pytest.raises(L.MoccaError):
        env.height_scan()
    # ... and so says the library itself, under the Python surface's own checks
    out, ptr = torch.zeros(N, 32, device="cuda"), lambda t: C.c_void_p(t.data_ptr())
    assert env.lib.mocca_act(env.h, ptr(obs), env.obs_dim, None, 1, ptr(out), None, None, None, None) == -1
    assert b"mocca_set_policy" in env.lib.mocca_last_error(env.h)
    assert env.lib.mocca_height_scan(env.h, ptr(out), 32, None, None) == -1
    assert b"mocca_set_height_scan" in env.lib.mocca_last_error(env.h)
    env.step(torch.zeros(N, 21, device="cuda"))       # the handle itself still steps
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs).all()
    env.close()
    assert env.h is None
