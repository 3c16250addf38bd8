"""mocca_ppo_grad on the GPU (include/mocca.h): the gradient and the statistics against float64 autograd with float32 autograd as the
yardstick, and the call's contract -- fixed bits, overwritten outputs, graph capture, a read-only image, the argument errors.  The checker
is tests/ppo_reference.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_grad_cases as G
import ppo_reference as R
from ppo_grad_cases import bits as _bits, device_policy as _dp, to_device as _device

pytestmark = pytest.mark.gpu
MODE = G.MODES["plain"]
KW = MODE.kw
_storage, _record = functools.partial(G.storage, MODE), functools.partial(G.record, MODE)


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.close()


def _call(env, d, idx=None, value_clip=False, **kw):
    return G.call(MODE, env, d, idx, value_clip, **kw)


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_gradient_and_stats_parity(env, name):
    assert not (f := G.parity(MODE, name, G.gpu_compute(MODE, env))), f


def test_same_bits_whatever_the_outputs_held_and_identity_idx(env):
    G.same_bits_contract(MODE, env)


def test_zero_advantages_and_no_value_coef_give_zero_gradient(env):
    """actor and critic gradient exactly 0, log_std's exactly -entropy_coef"""
    p, _, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p))
    st = dict(st, adv=np.zeros_like(st["adv"]))
    grad, _ = _call(env, _device(st, False), value_coef=0.0, entropy_coef=0.01)
    a = p.log_std.size
    assert np.all(grad[:-a] == 0) and np.all(grad[-a:] == -np.float32(0.01))


def test_graph_replay_sees_an_update_and_act_is_untouched(env):
    G.graph_replay_contract(MODE, env)


def test_one_adam_step_matches_autograd(env):
    """one torch.optim.Adam step from ppo_grad's gradient and one from float64 autograd's, on the 52 -> 256 -> 256 -> 21 policy: the
    parameters' difference, per tensor over that tensor's largest |step_f64|, stays within 3 x the difference a float32-autograd step leaves"""
    import torch
    p, _, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p))
    grad, _ = _call(env, _device(st, False))
    ref = R.loss_autograd(p, st, "float64", **KW).grad
    f32 = R.loss_autograd(p, st, "float32", **KW).grad

    def step(g):
        w = torch.tensor(R.flat_params(p), dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        w.grad = torch.tensor(np.asarray(g, np.float64))
        opt.step()
        return w.detach().numpy() - R.flat_params(p).astype(np.float64)

    want = step(ref)
    got, yard = R.triple(R.tensor_errors(p, step(grad), want)), R.triple(R.tensor_errors(p, step(f32), want))
    print(f"adam step: kernel {got}, f32 autograd {yard}")
    _record("adam", "ppo-B100", {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard})
    assert R.within(got, yard), (got, yard)


def test_argument_errors(env):
    """every refusal of include/mocca.h: a message, no fault, and the handle still works"""
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    p, _, st = _storage("tiny", True, 17)
    d = _device(st, False)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    grad, stats = torch.empty(_dp(p).n_head(), device="cuda"), torch.empty(8, device="cuda")

    def raw(e, obs=d["obs"], stride=5, action=d["action"], old_logp=d["old_logp"], adv=d["adv"], returns=d["returns"], old_value=None, n=17, clip=0.2,
            vc=0.5, ec=0.0, value_clip=0, g=grad):
        rc = e.lib.mocca_ppo_grad(e.h, ptr(obs), stride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value), None, n, clip, vc, ec,
                                  value_clip, ptr(g), ptr(stats), e._stream())
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
    cases = [dict(obs=None), dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(g=None), dict(value_clip=1),
             dict(n=0), dict(n=(1 << 22) + 1), dict(stride=4), dict(clip=float("nan")), dict(clip=-0.1), dict(vc=float("inf")), dict(vc=-1.0),
             dict(ec=float("nan")), dict(ec=-0.5)]
    for kw in cases:
        rc, msg = raw(env, **kw)
        assert rc != 0 and msg.startswith("mocca_ppo_grad:"), (kw, rc, msg)
    perm, sign = np.arange(5)[::-1].copy(), np.ones(5, np.float32)
    env.set_policy_symmetry((perm, sign, np.arange(3), np.ones(3, np.float32)))
    rc, msg = raw(env)
    assert rc != 0 and "symmetric" in msg
    env.set_policy_symmetry(None)
    assert raw(env)[0] == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"].double(), d["action"], d["old_logp"], d["adv"], d["returns"])
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"].cpu(), d["adv"], d["returns"])
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=torch.arange(4, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], value_clip=True)


def test_trainer_surface_takes_time_major_storage():
    """TorchVecEnv.ppo_grad on [T][N][...] storage viewed as rows equals VecEnv.ppo_grad on the flattened rows"""
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    p, _, st = _storage("ppo", True, 96)
    envs = make_vec_envs("Walker3DCustomEnv-v0", 1, 8, None, torch.device("cuda:0"))
    envs.attach_policy(_dp(p))
    d = _device(st, False)
    shaped = {k: v.reshape(12, 8, -1) for k, v in d.items()}
    idx = torch.randperm(96, device="cuda")[:40]
    a = envs.ppo_grad(shaped["obs"], shaped["action"], shaped["old_logp"], shaped["adv"], shaped["returns"], idx=idx, **KW)
    b = envs.venv.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, **KW)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a["grad"]), _bits(b["grad"])) and np.array_equal(_bits(a["stats"]), _bits(b["stats"]))
    envs.close()
