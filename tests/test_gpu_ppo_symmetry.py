"""mocca_ppo_grad_sym on the GPU (include/mocca.h): the symmetric policy's gradient and statistics against float64 autograd with float32
autograd as the yardstick, the mirrored minibatch, the call's contract -- fixed bits, overwritten outputs, graph capture, a read-only
image, the plain call left as it was --, the argument errors and a whole training run.  The checker is tests/ppo_symmetry_reference.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_symmetry_reference as S
import ppo_grad_cases as G
import ppo_reference as R
import ppo_symmetry_reference as PS
from ppo_grad_cases import bits as _bits, device_policy as _dp, to_device as _device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = G.MODES["sym"]
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


@pytest.mark.parametrize("name", ["mixed", "ppo"])
def test_mirrored_minibatch_gives_the_original_gradient(env, name):
    """(M_o s, M_a a) with the same old_logp, adv, returns and old_value is the same loss: the kernel's gradient of the mirrored minibatch
    passes the parity rule against the ORIGINAL minibatch's float64 gradient, float32 autograd on the original being the yardstick"""
    p, tables, st = _storage(name, True, 100)
    env.set_policy(_dp(p, tables))
    grad, stats = _call(env, _device(PS.mirror_storage(st, tables), False), value_clip=True)
    ref = PS.loss_autograd_sym(p, tables, st, "float64", value_clip=True, **KW)
    f32 = PS.loss_autograd_sym(p, tables, st, "float32", value_clip=True, **KW)
    got, yard = R.triple(R.tensor_errors(p, grad, ref.grad)), R.triple(R.tensor_errors(p, f32.grad, ref.grad))
    s_got, s_yard = R.triple(R.stat_units(stats[:4], ref.stats[:4])), R.triple(R.stat_units(f32.stats[:4], ref.stats[:4]))
    print(f"{name} mirrored: kernel {got}, f32 autograd {yard}; stats {s_got}, {s_yard}")
    _record("mirror", f"{name}-B100", {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard, "stats_kernel": s_got, "stats_f32_autograd": s_yard})
    assert R.within(got, yard), (got, yard)
    assert R.within(s_got, s_yard), (s_got, s_yard)
    assert stats[4] == np.float32(round(ref.stats[4] * 100)) / np.float32(100)


def test_same_bits_whatever_the_outputs_held_and_identity_idx(env):
    G.same_bits_contract(MODE, env)


def test_graph_replay_sees_an_update_and_act_is_untouched(env):
    G.graph_replay_contract(MODE, env)


def test_plain_call_is_untouched_by_a_symmetric_call_on_the_same_handle(env):
    """plain call, symmetric call (tables attached in between), detach, plain call again on one handle: the first and the third give
    identical bits, and they are what float64 autograd of the PLAIN loss gives; the symmetric call in between gave the symmetric gradient"""
    p = R.make_policy("ppo", norm=True, seed=1)
    tables = PS.random_tables(52, 3, 21)
    st = R.make_storage(p, 100, seed=2)
    env.set_policy(_dp(p))
    d = _device(st, False)
    first = _call(env, d, value_clip=True)
    env.set_policy_symmetry(tables)
    sym = _call(env, d, value_clip=True)
    env.set_policy_symmetry(None)
    third = _call(env, d, value_clip=True)
    assert np.array_equal(_bits(first[0]), _bits(third[0])) and np.array_equal(_bits(first[1]), _bits(third[1]))
    plain64 = R.loss_autograd(p, st, "float64", value_clip=True, **KW).grad
    sym64 = PS.loss_autograd_sym(p, tables, st, "float64", value_clip=True, **KW).grad
    assert R.tensor_errors(p, first[0], plain64).max() < 1e-4 and R.tensor_errors(p, sym[0], sym64).max() < 1e-4
    assert R.tensor_errors(p, sym[0], plain64).max() > 0.1      # two different functions


def test_one_adam_step_matches_autograd_through_symmetric_gaussian(env):
    """one torch.optim.Adam step from ppo_grad's gradient and one from float64 autograd through symmetry.SymmetricGaussian -- the module a
    trainer's torch update differentiates --, on the 52 -> 256 -> 256 -> 21 policy: the parameters' difference, per tensor over that tensor's
    largest |step_f64|, stays within 3 x the difference a float32 step through the same module leaves"""
    import torch
    from mocca_envs_amd.symmetry import SymmetricGaussian
    p, tables, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p, tables))
    grad, _ = _call(env, _device(st, False))

    def module_grad(dtype):
        actor, critic, log_std = S.sequentials(p, dtype)
        net = SymmetricGaussian(actor, critic, log_std, tables)
        t = lambda x: torch.tensor(np.asarray(x), dtype=dtype)
        logp, entropy, value = net.evaluate_actions(t(st["obs"]), t(st["action"]), t(p.obs_mean), t(p.inv_std), p.clip)
        r = torch.exp(logp - t(st["old_logp"]))
        surr = torch.min(r * t(st["adv"]), torch.clamp(r, 1 - KW["clip"], 1 + KW["clip"]) * t(st["adv"])).mean()
        loss = -surr + KW["value_coef"] * 0.5 * ((value - t(st["returns"])) ** 2).mean() - KW["entropy_coef"] * entropy.mean()
        leaves = [q for seq in (actor, critic) for m in seq if isinstance(m, torch.nn.Linear) for q in (m.weight, m.bias)] + [log_std]
        return np.concatenate([g.detach().numpy().reshape(-1) for g in torch.autograd.grad(loss, leaves)]).astype(np.float64)

    ref, f32 = module_grad(torch.float64), module_grad(torch.float32)
    assert R.tensor_errors(p, ref, PS.loss_autograd_sym(p, tables, st, "float64", **KW).grad).max() < 1e-10      # the module IS the reference's function

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
    """every refusal of include/mocca.h: a message, no fault, and the handle still works after each"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    p, tables, st = _storage("tiny", True, 17)
    d = _device(st, False)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    grad, stats = torch.empty(_dp(p).n_head(), device="cuda"), torch.empty(8, device="cuda")

    def raw(e, obs=d["obs"], stride=5, action=d["action"], old_logp=d["old_logp"], adv=d["adv"], returns=d["returns"], old_value=None, n=17, clip=0.2,
            vc=0.5, ec=0.0, value_clip=0, g=grad, fn="mocca_ppo_grad_sym"):
        rc = getattr(e.lib, fn)(e.h, ptr(obs), stride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value), None, n, clip, vc, ec,
                                value_clip, ptr(g), ptr(stats), e._stream())
        return rc, (e.lib.mocca_last_error(e.h) or b"").decode()

    fresh = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    rc, msg = raw(fresh)
    assert rc != 0 and msg.startswith("mocca_ppo_grad_sym:") and "mocca_set_policy" in msg
    table = np.ascontiguousarray(_dp(p).table(), np.int32)      # shapes only: the image is not filled until mocca_update_policy
    assert fresh.lib.mocca_set_policy(fresh.h, table.ctypes.data_as(C.c_void_p), table.shape[0], 5, 3, 5.0) == 0
    rc, msg = raw(fresh)
    assert rc != 0 and "mocca_update_policy" in msg
    fresh.close()
    env.set_policy(_dp(p))      # a policy WITHOUT tables
    rc, msg = raw(env)
    assert rc != 0 and msg.startswith("mocca_ppo_grad_sym:") and "mocca_set_policy_symmetry" in msg
    assert raw(env, fn="mocca_ppo_grad")[0] == 0      # ... and the handle still works
    env.set_policy_symmetry(tables)
    good = raw(env)
    assert good[0] == 0
    torch.cuda.synchronize()
    want = grad.clone()
    rc, msg = raw(env, fn="mocca_ppo_grad")      # the plain call keeps refusing a handle with tables, and points here
    assert rc != 0 and msg.startswith("mocca_ppo_grad:") and "symmetric" in msg and "mocca_ppo_grad_sym" in msg
    cases = [dict(obs=None), dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(g=None), dict(value_clip=1),
             dict(n=0), dict(n=(1 << 21) + 1), dict(n=(1 << 22) + 1), dict(stride=4), dict(clip=float("nan")), dict(clip=-0.1), dict(vc=float("inf")),
             dict(vc=-1.0), dict(ec=float("nan")), dict(ec=-0.5)]
    for kw in cases:
        rc, msg = raw(env, **kw)
        assert rc != 0 and msg.startswith("mocca_ppo_grad_sym:"), (kw, rc, msg)
        grad.fill_(float("nan"))
        assert raw(env)[0] == 0, kw      # after each refusal the handle still works
        torch.cuda.synchronize()
        assert np.array_equal(_bits(grad), _bits(want)), kw
    out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"])      # VecEnv.ppo_grad on a symmetric policy no longer raises
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out["grad"]), _bits(want))
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"].double(), d["action"], d["old_logp"], d["adv"], d["returns"])
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], value_clip=True)


def test_trainer_surface_passes_through():
    """TorchVecEnv.ppo_grad with a `symmetric_policy` attached, on [T][N][...] storage viewed as rows, equals VecEnv.ppo_grad on the flattened
    rows, and is the symmetric gradient for the ENV's own mirror tables"""
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    p = R.make_policy("ppo", norm=True, seed=1)
    envs = make_vec_envs("Walker3DCustomEnv-v0", 1, 8, None, torch.device("cuda:0"))
    dp = envs.symmetric_policy(_dp(p))
    st = PS.make_storage_sym(p, dp.symmetry, 96, seed=4)
    envs.attach_policy(dp)
    d = _device(st, False)
    shaped = {k: v.reshape(12, 8, -1) for k, v in d.items()}
    idx = torch.randperm(96, device="cuda")[:40]
    a = envs.ppo_grad(shaped["obs"], shaped["action"], shaped["old_logp"], shaped["adv"], shaped["returns"], idx=idx, **KW)
    b = envs.venv.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, **KW)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a["grad"]), _bits(b["grad"])) and np.array_equal(_bits(a["stats"]), _bits(b["stats"]))
    ref = PS.loss_autograd_sym(p, dp.symmetry, R.gather(st, idx.cpu().numpy()), "float64", **KW).grad
    assert R.tensor_errors(p, a["grad"].cpu().numpy(), ref).max() < 1e-4
    envs.close()


DEMO_FLAGS = ["--symmetric", "--device-policy", "--device-returns", "--device-grad", "--verify-grad", "--fixed-std", "--log-std", "-1.2", "--iters", "130"]
LEARNING_THRESHOLD = 3.83      # half the smaller of the two measured ratios (docstring below)


def test_ppo_demo_learns_with_the_symmetric_gradient(tmp_path):
    """tools/ppo_demo.py --symmetric --device-policy --device-returns --device-grad --verify-grad --fixed-std --log-std -1.2 --iters 130 as a
    child process: every verify_grad line -- the largest difference between the kernel's gradient and autograd through SymmetricGaussian on
    the first minibatch of an iteration, scaled per tensor -- stays below 1e-2 (a wiring error leaves a difference of order 1), and the
    policy learns: mean_length of the last logged line over the first exceeds LEARNING_THRESHOLD.  Measured on one MI355X with these flags
    (profiles/ppo_demo_symmetric_device_grad.jsonl, profiles/ppo_demo_symmetric_torch_grad.jsonl): mean_length 22.8 -> 174.9 (x 7.66) with
    --device-grad, 22.8 -> 184.9 (x 8.10) with the torch update through SymmetricGaussian in its place; the threshold is half the smaller
    ratio.  verify_grad over the 130 iterations: 2.9e-6 .. 6.8e-6.  This run also covers --device-grad with --fixed-std."""
    out = str(tmp_path / "demo")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ppo_demo.py"), *DEMO_FLAGS, "--out", out], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [json.loads(x) for x in res.stdout.splitlines() if x.startswith("{")]
    verify = [x["verify_grad"] for x in lines if "verify_grad" in x]
    log = [x for x in lines if "mean_length" in x]
    ratio = log[-1]["mean_length"] / log[0]["mean_length"]
    print(f"verify_grad: {len(verify)} lines, largest {max(verify):.3g}; mean_length {log[0]['mean_length']:.1f} -> {log[-1]['mean_length']:.1f} (x{ratio:.2f})")
    _record("demo", "symmetric-device-grad", {"verify_grad_max": max(verify), "verify_grad_lines": len(verify), "mean_length_first": log[0]["mean_length"],
                                              "mean_length_last": log[-1]["mean_length"], "env_steps_per_s_incl_learning": log[-1]["env_steps_per_s_incl_learning"]})
    assert len(verify) == 130 and max(verify) < 1e-2, max(verify)
    assert ratio > LEARNING_THRESHOLD, ratio
