"""mocca_distill_grad on the GPU (include/mocca.h): the regression gradient and its statistics against float64 autograd with float32 autograd
as the yardstick, and the call's contract -- fixed bits, overwritten outputs, graph capture, a scratch shared with mocca_ppo_grad, a
read-only image, the argument errors.  The checker is tests/distill_reference.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_grad_cases as G
import ppo_reference as R
from ppo_grad_cases import bits as _bits, device_policy as _dp, to_device as _device

pytestmark = pytest.mark.gpu
MODE = G.MODES["distill"]
KW = MODE.kw
_storage = functools.partial(G.storage, MODE)


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.close()


def _call(env, d, idx=None, use_value=True, **kw):
    return G.call(MODE, env, d, idx, use_value, **kw)


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_gradient_and_stats_parity(env, name):
    assert not (f := G.parity(MODE, name, G.gpu_compute(MODE, env))), f


def test_same_bits_whatever_the_outputs_held_and_identity_idx(env):
    G.same_bits_contract(MODE, env)


def test_no_coefficient_and_no_value_targets_give_all_zero_bits(env):
    p, _, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p))
    grad, stats = _call(env, _device(st), use_value=False, distill_coef=0.0)
    assert not grad.view(np.uint32).any()
    assert stats[7] > 0 and stats[1] == 0 and stats[5] == 0      # the loss is still reported


def test_graph_replay_sees_an_update(env):
    G.graph_replay_contract(MODE, env)


def test_ppo_grad_and_act_are_untouched(env):
    """ppo_grad before and after a distill_grad at the same B gives the same bits (one scratch serves both, the image is only read), and
    so does act"""
    import torch
    p = R.make_policy("ppo", norm=True, seed=1)
    ppo_st, st = R.make_storage(p, 100, seed=2), _storage("ppo", True, 100)[2]
    env.set_policy(_dp(p))
    pd, d = {k: torch.from_numpy(v).cuda() for k, v in ppo_st.items()}, _device(st)
    obs4 = d["obs"][:4].contiguous()
    ppo = lambda: env.ppo_grad(pd["obs"], pd["action"], pd["old_logp"], pd["adv"], pd["returns"], clip=0.2, value_coef=0.5, entropy_coef=0.01)
    before, act_before = ppo(), {k: v.clone() for k, v in env.act(obs4, deterministic=True).items()}
    mine = _call(env, d)
    after, act_after = ppo(), env.act(obs4, deterministic=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(before["grad"]), _bits(after["grad"])) and np.array_equal(_bits(before["stats"]), _bits(after["stats"]))
    assert all(np.array_equal(_bits(act_before[k]), _bits(act_after[k])) for k in act_before)
    again = _call(env, d)
    assert np.array_equal(_bits(mine[0]), _bits(again[0])) and np.array_equal(_bits(mine[1]), _bits(again[1]))


def test_argument_errors(env):
    """every refusal of include/mocca.h: a message, outputs untouched, and the handle still works"""
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    p, _, st = _storage("tiny", True, 17)
    d = _device(st)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    grad, stats = torch.full((_dp(p).n_head(),), 7.0, device="cuda"), torch.full((8,), 7.0, device="cuda")

    def raw(e, obs=d["obs"], stride=5, target=d["target"], vt=d["value_target"], n=17, dc=1.0, vc=0.5, g=grad):
        rc = e.lib.mocca_distill_grad(e.h, ptr(obs), stride, ptr(target), ptr(vt), None, n, dc, vc, ptr(g), ptr(stats), e._stream())
        return rc, (e.lib.mocca_last_error(e.h) or b"").decode()

    fresh = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    rc, msg = raw(fresh)
    assert rc != 0 and "mocca_set_policy" in msg
    table = np.ascontiguousarray(_dp(p).table(), np.int32)      # shapes only: the image is not filled until mocca_update_policy
    assert fresh.lib.mocca_set_policy(fresh.h, table.ctypes.data_as(C.c_void_p), table.shape[0], 5, 3, 5.0) == 0
    rc, msg = raw(fresh)
    assert rc != 0 and "mocca_update_policy" in msg
    fresh.close()
    env.set_policy(_dp(p))
    cases = [dict(obs=None), dict(target=None), dict(g=None), dict(n=0), dict(n=(1 << 22) + 1), dict(stride=4), dict(dc=float("nan")),
             dict(dc=-0.1), dict(dc=float("inf")), dict(vc=float("inf")), dict(vc=-1.0), dict(vc=float("nan"))]
    for kw in cases:
        rc, msg = raw(env, **kw)
        assert rc != 0 and msg.startswith("mocca_distill_grad:"), (kw, rc, msg)
    tables = (np.arange(5)[::-1].copy(), np.ones(5, np.float32), np.arange(3), np.ones(3, np.float32))
    for attach in (env.set_policy_symmetry, lambda t: env.set_policy_mirror_loss(t, 0.5), env.set_policy_mirror_dup):
        attach(tables)
        rc, msg = raw(env)
        assert rc != 0 and msg.startswith("mocca_distill_grad:") and "detach" in msg, msg
        with pytest.raises(L.MoccaError):
            env.distill_grad(d["obs"], d["target"], d["value_target"])
        env.set_policy(_dp(p))      # drops whatever was attached
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (stats == 7.0).all()      # no refused call wrote anything
    assert raw(env)[0] == 0 and raw(env, vt=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and not (grad == 7.0).any()
    with pytest.raises(ValueError):
        env.distill_grad(d["obs"].double(), d["target"])
    with pytest.raises(ValueError):
        env.distill_grad(d["obs"], d["target"][:, :2].contiguous())
    with pytest.raises(ValueError):
        env.distill_grad(d["obs"], d["target"], d["value_target"].cpu())
    with pytest.raises(ValueError):
        env.distill_grad(d["obs"], d["target"], idx=torch.arange(4, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError):
        env.distill_grad(d["obs"], d["target"], distill_coef=-1.0)
