"""mocca_ppo_grad_mirror and mocca_set_policy_mirror_loss on the GPU (include/mocca.h): the gradient and statistics of PPO's loss with the
mirror-symmetry loss added against float64 autograd with float32 autograd as the yardstick, the critic left alone by the term, the call's
contract -- fixed bits, overwritten outputs, graph capture, act and the two other gradient calls left as they were --, mocca_ppo_update with
the loss attached, every refusal, and a whole training run.  The checker is tests/ppo_mirror_reference.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ppo_grad_cases as G
import ppo_mirror_reference as PM
import ppo_reference as R
import ppo_symmetry_reference as PS
import ppo_update_reference as U
from ppo_grad_cases import device_policy as _dp, same as _same, to_device as _device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = G.MODES["mirror"]
KW = MODE.kw
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
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


@pytest.mark.parametrize("name,n_rows", [("mixed", 100), ("ppo", 100), ("ppo", 1100), ("tiny", 9)])
def test_the_critic_receives_no_mirror_term(env, name, n_rows):
    """coef = 4: the critic's tensors pass the parity rule against the float64 gradient of the PLAIN loss (ppo_reference.loss_autograd),
    float32 autograd of the plain loss being the yardstick -- the critic's mirrored columns contribute nothing --, while the actor's
    tensors are far from the plain gradient (the term acts)"""
    p, tables, st = _storage(name, True, n_rows)
    env.set_policy(_dp(p))
    env.set_policy_mirror_loss(tables, 4.0)
    grad, _ = _call(env, _device(st), value_clip=True)
    ref = R.loss_autograd(p, st, "float64", value_clip=True, **KW).grad
    f32 = R.loss_autograd(p, st, "float32", value_clip=True, **KW).grad
    critic = np.concatenate([np.arange(a, b) for a, b in PM.critic_slices(p)])
    got, yard = R.triple(R.tensor_errors(p, grad, ref)[critic]), R.triple(R.tensor_errors(p, f32, ref)[critic])
    print(f"{name} B{n_rows} critic: kernel {got}, f32 autograd {yard}")
    _record("critic", f"{name}-B{n_rows}", {"kernel_vs_f64_plain": got, "f32_autograd_vs_f64_plain": yard, "elements": int(critic.size)})
    assert R.within(got, yard), (got, yard)
    actor = np.arange(0, PM.critic_slices(p)[0][0])
    assert R.tensor_errors(p, grad, ref)[actor].max() > 0.1


def test_same_bits_whatever_the_outputs_held_and_identity_idx(env):
    G.same_bits_contract(MODE, env)


def test_graph_replay_sees_an_update_and_act_is_the_plain_policys(env):
    G.graph_replay_contract(MODE, env)


def test_the_other_two_gradient_calls_are_untouched(env):
    """one handle: plain call, attach the loss, mirror call, detach, plain call -- the two plain calls give identical bits; then the
    symmetric call before and after a mirror-loss call (symmetry detached and attached again around it) gives identical bits.  The three
    are three different functions, each what its float64 autograd gives"""
    p, tables, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p))
    d = _device(st)
    plain1 = _call(env, d, value_clip=True)
    env.set_policy_mirror_loss(tables, 4.0)
    mirror1 = _call(env, d, value_clip=True)
    env.set_policy_mirror_loss(None)
    plain2 = _call(env, d, value_clip=True)
    assert _same(plain1[0], plain2[0]) and _same(plain1[1], plain2[1]) and plain2[1][7] == 0
    env.set_policy_symmetry(tables)
    sym1 = _call(env, d, value_clip=True)
    env.set_policy_symmetry(None)
    env.set_policy_mirror_loss(tables, 4.0)
    mirror2 = _call(env, d, value_clip=True)
    env.set_policy_mirror_loss(None)
    env.set_policy_symmetry(tables)
    sym2 = _call(env, d, value_clip=True)
    env.set_policy_symmetry(None)
    assert _same(sym1[0], sym2[0]) and _same(sym1[1], sym2[1]) and sym2[1][7] == 0
    assert _same(mirror1[0], mirror2[0]) and _same(mirror1[1], mirror2[1])
    kw = dict(value_clip=True, **KW)
    plain64, sym64 = R.loss_autograd(p, st, "float64", **kw).grad, PS.loss_autograd_sym(p, tables, st, "float64", **kw).grad
    mirror64 = PM.loss_autograd_mirror(p, tables, 4.0, st, "float64", **kw).grad
    for got, want in ((plain1, plain64), (sym1, sym64), (mirror1, mirror64)):
        assert R.tensor_errors(p, got[0], want).max() < 1e-4
    assert R.tensor_errors(p, mirror1[0], plain64).max() > 0.1 and R.tensor_errors(p, mirror1[0], sym64).max() > 0.1


@pytest.mark.parametrize("name,n_rows,n_batch,epochs,coef", [("tiny", 200, 48, 3, 0.5), ("ppo", 1100, 366, 1, 4.0), ("ppo", 1100, 550, 1, 4.0)],
                         ids=["tiny", "ppo-three-minibatches", "ppo-three-row-chunks"])
def test_ppo_update_is_its_parts_with_the_loss_attached(env, name, n_rows, n_batch, epochs, coef):
    """one ppo_update with a mirror loss attached equals a Python loop of [the checker's permutation at the clock's t -> ppo_grad(idx), which
    is mocca_ppo_grad_mirror -> adam_step] from the same start, bit for bit in params, moments, clock and every stats row but [6]; stats[6]
    is the checker's clip coefficient of that minibatch's gradient, stats[7] the minibatch's L_m.  1100 rows: three minibatches of 366
    (perm + u B), and two of 550, whose 1104 scratch rows are three row chunks of launch 2"""
    import torch
    from mocca_envs_amd.rollout import AdamState
    p, tables, st = _storage(name, True, n_rows)
    dp = _dp(p)
    env.set_policy(dp)
    env.set_policy_mirror_loss(tables, coef)
    d, n_head, per_epoch = _device(st), dp.n_head(), n_rows // n_batch
    start = torch.from_numpy(dp.flat_params()).cuda()
    update = lambda params, state: env.ppo_update(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], params, state, n_batch, epochs, seed=77,
                                                  **KW, **ADAM)["stats"]
    params, state = start.clone(), AdamState(n_head, env.device)
    stats = update(params, state).clone()
    assert stats.shape == (epochs * per_epoch, 8)
    params2, state2 = start.clone(), AdamState(n_head, env.device)
    env.update_policy(params2)
    rows, coefs = [], []
    for ep in range(epochs):
        perm = U.permutation(n_rows, int(state2.clock[0].item()), 77)
        for u in range(per_epoch):
            idx = torch.from_numpy(perm[u * n_batch:(u + 1) * n_batch].copy()).cuda()
            out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, **KW)
            env.adam_step(params2, out["grad"], state2, **ADAM)
            rows.append(out["stats"].cpu().numpy())
            coefs.append(U.clip_coef(out["grad"].cpu().numpy(), ADAM["max_grad_norm"]))
    torch.cuda.synchronize()
    assert _same(params, params2) and _same(state.moments, state2.moments) and _same(state.clock, state2.clock)
    assert state.clock.tolist()[0] == epochs * per_epoch and not _same(params, start)
    got, want = stats.cpu().numpy(), np.array(rows)
    assert _same(np.delete(got, 6, axis=1), np.delete(want, 6, axis=1))
    assert _same(got[:, 6], np.array(coefs, np.float32)) and (got[:, 7] > 0).all()
    # the first minibatch's L_m is the checker's at the starting weights
    perm = U.permutation(n_rows, 0, 77)
    ref = PM.loss_autograd_mirror(p, tables, coef, R.gather(st, perm[:n_batch]), "float64", **KW)
    assert abs(got[0, 7] - ref.stats[7]) <= 1e-5 * ref.stats[7]


def test_argument_errors(env):
    """every refusal of include/mocca.h for the two entry points: a message, no fault, and afterwards the outputs and the handle are as
    they were -- the next good call gives the bits of the one before"""
    import torch
    p, tables, st = _storage("tiny", True, 17)
    d = _device(st)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    grad, stats = torch.empty(_dp(p).n_head(), device="cuda"), torch.empty(8, device="cuda")
    arr = lambda t: [x.ctypes.data_as(C.c_void_p) for x in t]
    err = lambda: (env.lib.mocca_last_error(env.h) or b"").decode()

    def raw(obs=d["obs"], stride=5, action=d["action"], old_logp=d["old_logp"], adv=d["adv"], returns=d["returns"], old_value=None, n=17, clip=0.2,
            vc=0.5, ec=0.0, value_clip=0, g=grad, fn="mocca_ppo_grad_mirror"):
        rc = getattr(env.lib, fn)(env.h, ptr(obs), stride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value), None, n, clip, vc, ec,
                                  value_clip, ptr(g), ptr(stats), env._stream())
        return rc, err()

    def attach(t, coef, fn="mocca_set_policy_mirror_loss"):
        t = [np.ascontiguousarray(x, dt) for x, dt in zip(t, (np.int32, np.float32, np.int32, np.float32))]
        rc = getattr(env.lib, fn)(env.h, *arr(t), *([] if fn == "mocca_set_policy_symmetry" else [C.c_double(coef)]))
        return rc, err()

    def good(fn="mocca_ppo_grad_mirror"):
        grad.fill_(float("nan")), stats.fill_(float("nan"))
        assert raw(fn=fn)[0] == 0
        torch.cuda.synchronize()
        return grad.clone(), stats.clone()

    env.set_policy(_dp(p))      # nothing attached
    rc, msg = raw()
    assert rc != 0 and msg.startswith("mocca_ppo_grad_mirror:") and "mocca_set_policy_mirror_loss" in msg
    plain = good("mocca_ppo_grad")      # ... and the handle still works
    # the setter's own refusals leave the handle with nothing attached
    in_perm, in_sign, act_perm, act_sign = tables
    bad_tables = [(np.full_like(in_perm, 9), in_sign, act_perm, act_sign),                        # an index out of range
                  (in_perm, in_sign, np.roll(np.arange(3, dtype=np.int32), 1), np.ones(3, np.float32)),      # a 3-cycle: not an involution
                  (in_perm, in_sign * 0.5, act_perm, act_sign),                                   # a sign that is not +-1
                  (np.array([1, 0, 2, 3, 4], np.int32), np.array([1, -1, 1, 1, 1], np.float32), act_perm, act_sign)]      # signs differ across a pair
    for t in bad_tables:
        rc, msg = attach(t, 1.0)
        assert rc != 0 and msg.startswith("mocca_set_policy_mirror_loss:"), msg
        assert raw()[0] != 0 and all(_same(a, b) for a, b in zip(plain, good("mocca_ppo_grad")))
    for coef in (-0.5, float("nan"), float("inf")):
        rc, msg = attach(tables, coef)
        assert rc != 0 and "mirror_coef" in msg, (coef, msg)
        assert raw()[0] != 0 and all(_same(a, b) for a, b in zip(plain, good("mocca_ppo_grad")))
    # the two attachments exclude each other
    env.set_policy_symmetry(tables)
    sym = good("mocca_ppo_grad_sym")
    rc, msg = attach(tables, 1.0)
    assert rc != 0 and msg.startswith("mocca_set_policy_mirror_loss:") and "mocca_set_policy_symmetry" in msg
    assert all(_same(a, b) for a, b in zip(sym, good("mocca_ppo_grad_sym")))      # still the symmetric policy
    env.set_policy_symmetry(None)
    env.set_policy_mirror_loss(tables, 0.5)
    want = good()
    assert want[1][7].item() > 0
    rc, msg = attach(tables, 0.0, fn="mocca_set_policy_symmetry")
    assert rc != 0 and msg.startswith("mocca_set_policy_symmetry:") and "mocca_set_policy_mirror_loss" in msg
    assert all(_same(a, b) for a, b in zip(want, good()))
    # a refused setter keeps the attachment in place, tables and weight
    for t, coef in [(bad_tables[0], 1.0), (tables, -1.0)]:
        assert attach(t, coef)[0] != 0 and all(_same(a, b) for a, b in zip(want, good()))
    # the two other gradient calls refuse while the loss is attached, and name the one to call
    for fn in ("mocca_ppo_grad", "mocca_ppo_grad_sym"):
        grad.fill_(float("nan")), stats.fill_(float("nan"))
        rc, msg = raw(fn=fn)
        torch.cuda.synchronize()
        assert rc != 0 and msg.startswith(fn + ":") and "mocca_ppo_grad_mirror" in msg, msg
        assert torch.isnan(grad).all() and torch.isnan(stats).all()      # nothing was launched
        assert all(_same(a, b) for a, b in zip(want, good()))
    cases = [dict(obs=None), dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(g=None), dict(value_clip=1),
             dict(n=0), dict(n=(1 << 21) + 1), dict(n=(1 << 22) + 1), dict(stride=4), dict(clip=float("nan")), dict(clip=-0.1), dict(vc=float("inf")),
             dict(vc=-1.0), dict(ec=float("nan")), dict(ec=-0.5)]
    free = torch.cuda.mem_get_info()[0]
    for kw in cases:
        grad.fill_(float("nan")), stats.fill_(float("nan"))
        rc, msg = raw(**kw)
        torch.cuda.synchronize()
        assert rc != 0 and msg.startswith("mocca_ppo_grad_mirror:"), (kw, rc, msg)
        assert (kw.get("g", 0) is None or torch.isnan(grad).all()) and torch.isnan(stats).all(), kw
        assert all(_same(a, b) for a, b in zip(want, good())), kw      # after each refusal the handle still works
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)      # B > 2^21 is an argument check: its scratch (gigabytes) was not allocated
    # ppo_update decides the same refusals before its first launch
    from mocca_envs_amd.rollout import AdamState
    params, state = torch.from_numpy(_dp(p).flat_params()).cuda(), AdamState(_dp(p).n_head(), env.device)
    before = params.clone()
    rc = env.lib.mocca_ppo_update(env.h, ptr(d["obs"]), 5, ptr(d["action"]), ptr(d["old_logp"]), ptr(d["adv"]), ptr(d["returns"]), None, 17, 8, 1, 0.2, 0.5,
                                  0.0, 1, ptr(params), params.numel(), _dp(p).n_head(), ptr(state.moments), ptr(state.clock), 3e-4, 0.9, 0.999, 1e-5,
                                  0.5, 77, None, env._stream())      # value_clip without old_value_dev
    torch.cuda.synchronize()
    assert rc != 0 and err().startswith("mocca_ppo_update:") and _same(params, before) and state.clock.tolist()[0] == 0
    assert all(_same(a, b) for a, b in zip(want, good()))
    # the Python surface: ValueError ahead of the library for a wrong table size, detaching through None, set_policy drops the attachment
    with pytest.raises(ValueError):
        env.set_policy_mirror_loss((in_perm[:4], in_sign[:4], act_perm, act_sign), 1.0)
    assert env.mirror_loss is not None and all(_same(a, b) for a, b in zip(want, good()))
    env.set_policy_mirror_loss(None)
    assert env.mirror_loss is None and raw()[0] != 0 and all(_same(a, b) for a, b in zip(plain, good("mocca_ppo_grad")))
    env.set_policy_mirror_loss(tables, 0.5)
    env.set_policy(_dp(p))
    assert env.mirror_loss is None and raw()[0] != 0 and all(_same(a, b) for a, b in zip(plain, good("mocca_ppo_grad")))


def test_trainer_surface_passes_through():
    """TorchVecEnv.set_policy_mirror_loss with policy_mirror_tables -- the tables symmetric_policy attaches --, then ppo_grad on [T][N][...]
    storage viewed as rows: VecEnv.ppo_grad's bits on the flattened rows, and the mirror-loss gradient for the ENV's own tables"""
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    p = R.make_policy("ppo", norm=True, seed=1)
    envs = make_vec_envs("Walker3DCustomEnv-v0", 1, 8, None, torch.device("cuda:0"))
    tables = envs.policy_mirror_tables(_dp(p))
    assert all(np.array_equal(a, b) for a, b in zip(tables, envs.symmetric_policy(_dp(p)).symmetry))
    st = R.make_storage(p, 96, seed=4)
    envs.attach_policy(_dp(p))
    envs.set_policy_mirror_loss(tables, 0.5)
    d = _device(st)
    shaped = {k: v.reshape(12, 8, -1) for k, v in d.items()}
    idx = torch.randperm(96, device="cuda")[:40]
    a = envs.ppo_grad(shaped["obs"], shaped["action"], shaped["old_logp"], shaped["adv"], shaped["returns"], idx=idx, **KW)
    b = envs.venv.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, **KW)
    torch.cuda.synchronize()
    assert _same(a["grad"], b["grad"]) and _same(a["stats"], b["stats"])
    ref = PM.loss_autograd_mirror(p, tables, 0.5, R.gather(st, idx.cpu().numpy()), "float64", **KW)
    assert R.tensor_errors(p, a["grad"].cpu().numpy(), ref.grad).max() < 1e-4 and abs(a["stats"][7].item() - ref.stats[7]) < 1e-5 * ref.stats[7]
    envs.set_policy_mirror_loss(None)
    envs.close()


DEMO_FLAGS = ["--device-policy", "--device-returns", "--device-grad", "--device-update", "--verify-grad", "--fixed-std", "--log-std", "-1.2", "--iters", "130"]
DEMO_COEF = 4.0
LEARNING_THRESHOLD = 2.42      # half the smaller of the two measured ratios (docstring below)


def _demo(tmp_path, tag, coef):
    out = str(tmp_path / tag)
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "ppo_demo.py"), *DEMO_FLAGS, "--mirror-loss", str(coef),
                          "--out", out], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [json.loads(x) for x in res.stdout.splitlines() if x.startswith("{")]
    return [x["verify_grad"] for x in lines if "verify_grad" in x], [x for x in lines if "mean_length" in x]


def test_ppo_demo_learns_and_the_loss_acts(tmp_path):
    """tools/ppo_demo.py --device-policy --device-returns --device-grad --device-update --mirror-loss 4 --verify-grad --fixed-std --log-std -1.2
    --iters 130 as a child process, and the same with --mirror-loss 0 (the same seed: the term is monitored, not trained on).
    It learns: mean_length of the last logged line over the first exceeds LEARNING_THRESHOLD.  Measured on one MI355X in one session with
    these flags: 22.8 -> 110.5 (x 4.84) at coef 4, 22.8 -> 111.2 (x 4.88) for the plain --device-update run (no --mirror-loss); the
    threshold is half the smaller ratio, the sibling tests' margin for seed and scheduling noise in a 17 M-step run.
    The loss acts: the final logged L_m at coef 4 is below the coef 0 run's (measured 0.00144 against 0.0119, a factor 8.3).
    --verify-grad's per-iteration difference between the kernel's gradient and float32 autograd through symmetry.mirror_loss is printed and
    recorded, not bounded here (measured: below 9e-6 over the 130 iterations); test_gradient_and_stats_parity bounds the gradient."""
    verify, log = _demo(tmp_path, "mirror", DEMO_COEF)
    verify0, log0 = _demo(tmp_path, "monitor", 0.0)
    ratio = log[-1]["mean_length"] / log[0]["mean_length"]
    l_m, l_m0 = log[-1]["mirror_loss"], log0[-1]["mirror_loss"]
    print(f"coef {DEMO_COEF:g}: verify_grad {len(verify)} lines, largest {max(verify):.3g}; mean_length {log[0]['mean_length']:.1f} -> "
          f"{log[-1]['mean_length']:.1f} (x{ratio:.2f}); final L_m {l_m:.4g} against {l_m0:.4g} at coef 0 (x{l_m0 / l_m:.2f}); coef 0: verify_grad "
          f"largest {max(verify0):.3g}, mean_length x{log0[-1]['mean_length'] / log0[0]['mean_length']:.2f}")
    _record("demo", "mirror-loss-device-update", {
        "coef": DEMO_COEF, "verify_grad_max": max(verify), "verify_grad_lines": len(verify), "mean_length_first": log[0]["mean_length"],
        "mean_length_last": log[-1]["mean_length"], "mean_length_factor": ratio, "mean_return_last": log[-1]["mean_return"],
        "env_steps_per_s_incl_learning": log[-1]["env_steps_per_s_incl_learning"], "mirror_loss_last": l_m, "mirror_loss_first": log[0]["mirror_loss"]})
    _record("demo", "mirror-loss-0-device-update", {
        "coef": 0.0, "verify_grad_max": max(verify0), "verify_grad_lines": len(verify0), "mean_length_first": log0[0]["mean_length"],
        "mean_length_last": log0[-1]["mean_length"], "mean_length_factor": log0[-1]["mean_length"] / log0[0]["mean_length"],
        "mean_return_last": log0[-1]["mean_return"], "mirror_loss_last": l_m0, "mirror_loss_first": log0[0]["mirror_loss"]})
    _record("demo", "final_mirror_loss_ratio_coef0_over_coef", l_m0 / l_m)
    assert len(verify) == 130 and len(verify0) == 130 and log[-1]["iter"] == 130
    assert ratio > LEARNING_THRESHOLD, ratio
    assert l_m < l_m0, (l_m, l_m0)
