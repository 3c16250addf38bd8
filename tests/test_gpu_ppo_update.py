"""mocca_adam_step and mocca_ppo_update on the GPU (include/mocca.h): the step's bits against the checker (tests/ppo_update_reference.py),
the step's visibility to mocca_act, the skipped step, the update against a Python loop of its parts, the device's permutation, fixed bits,
graph replay with the clock and the shuffle advancing on the device, every refusal, and a whole training run."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_symmetry_reference as PS
import ppo_reference as R
import ppo_update_reference as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(clip=R.CLIP, value_coef=0.5, entropy_coef=0.01)
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.close()


def _dp(p, tables=None):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip, symmetry=tables)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _state(env, n_head):
    from mocca_envs_amd.rollout import AdamState
    return AdamState(n_head, env.device)


_CASES = {}


def _case(name, n_rows, sym=False):
    """(policy, mirror tables or None, storage), computed once and left unchanged"""
    key = (name, n_rows, sym)
    if key not in _CASES:
        p = R.make_policy(name, norm=True, seed=1)
        tables = PS.random_tables(R.NETS[name][0], 3, R.NETS[name][1]) if sym else None
        _CASES[key] = (p, tables, R.make_storage(p, n_rows, seed=2))
    return _CASES[key]


def _device(st):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in st.items()}


@pytest.mark.parametrize("tail", [True, False], ids=["tail", "head"])
@pytest.mark.parametrize("fixed_std", [False, True], ids=["all", "fixed-std"])
@pytest.mark.parametrize("name", ["tiny", "single", "ppo"])
def test_adam_step_bits(env, name, fixed_std, tail):
    """three consecutive steps equal the checker bit for bit in params, moments and clock: the first and the last with a norm far above
    max_grad_norm, the second with one below it (coef = 1); what lies beyond n_params -- parameters, moments, the statistics tail -- is
    untouched, and the gradient there (NaN) is not read into the norm"""
    import torch
    p = R.make_policy(name, norm=tail, seed=1)
    dp = _dp(p)
    env.set_policy(dp)
    n_head = dp.n_head()
    n_params = n_head - dp.act_dim if fixed_std else n_head
    params = torch.from_numpy(dp.flat_params()).cuda()
    assert params.numel() == n_head + (2 * dp.in_dim if tail else 0)
    state = _state(env, n_head)
    state.moments[:, n_params:] = 7.0
    want = [params.cpu().numpy(), state.moments[0].cpu().numpy(), state.moments[1].cpu().numpy(), np.array(U.FRESH_CLOCK)]
    coefs = []
    for k in range(3):
        g = U.gradients(n_head, 10 * k + len(name), hi=10.0 if k != 1 else 1e-3)
        g[n_params:] = np.nan
        env.adam_step(params, torch.from_numpy(g).cuda(), state, n_params=n_params, **ADAM)
        head, m, v, clock, coef = U.adam_step(want[0][:n_head], g, want[1], want[2], want[3], n_params=n_params, lr=ADAM["lr"], eps=ADAM["eps"],
                                              max_grad_norm=ADAM["max_grad_norm"])
        want = [np.concatenate([head, want[0][n_head:]]), m, v, clock]
        coefs.append(float(coef))
        torch.cuda.synchronize()
        assert _same(params, want[0]), f"params differ at step {k}"
        assert _same(state.moments[0], want[1]) and _same(state.moments[1], want[2]), f"moments differ at step {k}"
        assert _same(state.clock, want[3]), (k, state.clock.tolist(), want[3].tolist())
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs
    assert (state.moments[:, n_params:] == 7.0).all() and _same(params[n_params:], dp.flat_params()[n_params:])
    assert state.clock.tolist()[0] == 3.0 and state.clock.tolist()[3] == 0.0


def test_the_step_is_visible_to_act(env):
    """after adam_step, act() gives what it gives after update_policy on the stepped tensor -- and not what it gave before the step"""
    import torch
    p = R.make_policy("ppo", norm=True, seed=1)
    dp = _dp(p)
    env.set_policy(dp)
    obs = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (4, dp.in_dim)).astype(np.float32)).cuda()
    before = {k: v.clone() for k, v in env.act(obs, deterministic=True).items()}
    params, state = torch.from_numpy(dp.flat_params()).cuda(), _state(env, dp.n_head())
    env.adam_step(params, torch.from_numpy(U.gradients(dp.n_head(), 3)).cuda(), state, **ADAM)
    after = {k: v.clone() for k, v in env.act(obs, deterministic=True).items()}
    env.update_policy(params)
    again = env.act(obs, deterministic=True)
    torch.cuda.synchronize()
    assert all(_same(after[k], again[k]) for k in after)
    assert not _same(before["action"], after["action"]) and not _same(before["value"], after["value"])


def test_a_nan_gradient_skips_the_step(env):
    """one NaN in grad: params, moments, t, the products and the image stay as they were, clock[3] = 1; the next clean step is the checker's"""
    import torch
    p = R.make_policy("tiny", norm=True, seed=1)
    dp = _dp(p)
    env.set_policy(dp)
    n_head = dp.n_head()
    obs = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (4, dp.in_dim)).astype(np.float32)).cuda()
    params, state = torch.from_numpy(dp.flat_params()).cuda(), _state(env, n_head)
    g0, g1 = U.gradients(n_head, 1), U.gradients(n_head, 2)
    env.adam_step(params, torch.from_numpy(g0).cuda(), state, **ADAM)
    held = [params.clone(), state.moments.clone(), state.clock.clone()]
    before = {k: v.clone() for k, v in env.act(obs, deterministic=True).items()}
    bad = g1.copy()
    bad[n_head // 2] = np.nan
    env.adam_step(params, torch.from_numpy(bad).cuda(), state, **ADAM)
    after = env.act(obs, deterministic=True)
    torch.cuda.synchronize()
    assert _same(params, held[0]) and _same(state.moments, held[1]) and _same(state.clock[:3], held[2][:3])
    assert state.clock.tolist() == [1.0, 0.9, 0.999, 1.0]
    assert all(_same(before[k], after[k]) for k in before)
    env.adam_step(params, torch.from_numpy(g1).cuda(), state, **ADAM)
    kw = dict(lr=ADAM["lr"], eps=ADAM["eps"], max_grad_norm=ADAM["max_grad_norm"])
    head, m, v, clock, _ = U.adam_step(dp.flat_params()[:n_head], g0, np.zeros(n_head, np.float32), np.zeros(n_head, np.float32), U.FRESH_CLOCK, **kw)
    head, m, v, clock, _ = U.adam_step(head, g1, m, v, clock, **kw)
    clock[3] = 1.0
    torch.cuda.synchronize()
    assert _same(params[:n_head], head) and _same(state.moments[0], m) and _same(state.moments[1], v) and _same(state.clock, clock)


def _update(env, d, params, state, n_batch, epochs, seed=77, stats=None, **kw):
    return env.ppo_update(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], params, state, n_batch, epochs, seed=seed, stats=stats,
                          **{**KW, **ADAM, **kw})["stats"]


@pytest.mark.parametrize("name,n_rows,n_batch,epochs,sym", [("tiny", 200, 48, 3, False), ("ppo", 1100, 512, 1, False), ("tiny", 200, 48, 3, True)],
                         ids=["tiny", "ppo", "tiny-symmetric"])
def test_ppo_update_is_its_parts(env, name, n_rows, n_batch, epochs, sym):
    """one ppo_update equals a Python loop of [the checker's permutation at the clock's t -> ppo_grad(idx) -> adam_step] from the same start,
    bit for bit in params, moments, clock and every stats row but [6]; stats[6] is the checker's clip coefficient of that minibatch's gradient"""
    import torch
    p, tables, st = _case(name, n_rows, sym)
    dp = _dp(p, tables)
    env.set_policy(dp)
    d, n_head, per_epoch = _device(st), dp.n_head(), n_rows // n_batch
    start = torch.from_numpy(dp.flat_params()).cuda()
    params, state = start.clone(), _state(env, n_head)
    stats = _update(env, d, params, state, n_batch, epochs).clone()
    assert stats.shape == (epochs * per_epoch, 8)
    params2, state2 = start.clone(), _state(env, n_head)
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
    assert _same(got[:, 6], np.array(coefs, np.float32)) and (got[:, 7] == 0).all()


@pytest.mark.parametrize("n_rows", [3, 100])
def test_the_device_permutation_is_the_checkers(env, n_rows):
    """epochs = 1, lr = 0 and minibatches of ONE row: the parameters never move, so stats row k is the statistics of rollout row perm[k]
    alone; the rows' statistics are pairwise different, so equality with the checker's order pins the device's permutation.  Twice in a row:
    the second call shuffles by the clock's new t"""
    import torch
    p, _, st = _case("tiny", n_rows)
    dp = _dp(p)
    env.set_policy(dp)
    d = _device(st)
    single = []
    for r in range(n_rows):
        out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=torch.tensor([r], device="cuda"), **KW)
        single.append(out["stats"].cpu().numpy()[:6])
    single = np.array(single)
    assert len({row.tobytes() for row in single}) == n_rows
    params, state = torch.from_numpy(dp.flat_params()).cuda(), _state(env, dp.n_head())
    for t in (0, n_rows):
        got = _update(env, d, params, state, 1, 1, seed=(5 << 32) + 9, lr=0.0).cpu().numpy()
        assert _same(got[:, :6], single[U.permutation(n_rows, t, (5 << 32) + 9)]), t
    assert _same(params, dp.flat_params()) and state.clock.tolist()[0] == 2 * n_rows


def test_same_bits_twice_and_another_seed_differs(env):
    import torch
    p, _, st = _case("tiny", 200)
    dp = _dp(p)
    env.set_policy(dp)
    d, runs = _device(st), []
    for seed in (1, 1, 2):
        params, state = torch.from_numpy(dp.flat_params()).cuda(), _state(env, dp.n_head())
        env.update_policy(params)
        stats = _update(env, d, params, state, 48, 2, seed=seed)
        runs.append((params, state.moments, state.clock, stats))
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))
    assert not _same(runs[0][0], runs[2][0])


def test_graph_replay_advances_the_clock_and_the_shuffle(env):
    """a graph captured after a warm call: one eager call and two replays equal three eager calls bit for bit -- the step count, the bias
    corrections and each epoch's shuffle come from the clock on the device"""
    import torch
    p, _, st = _case("tiny", 100)
    dp = _dp(p)
    env.set_policy(dp)
    d, n_head = _device(st), dp.n_head()
    start = torch.from_numpy(dp.flat_params()).cuda()
    params, state, stats = start.clone(), _state(env, n_head), torch.zeros(4, 8, device="cuda")
    call = lambda pr, s, out: _update(env, d, pr, s, 48, 2, stats=out)
    call(params, state, stats)      # warm: the scratch is allocated
    torch.cuda.synchronize()
    params.copy_(start), state.reset(), env.update_policy(params)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(params, state, stats)
    call(params, state, stats)
    graph.replay()
    graph.replay()
    params2, state2, stats2 = start.clone(), _state(env, n_head), torch.zeros(4, 8, device="cuda")
    env.update_policy(params2)
    for _ in range(3):
        call(params2, state2, stats2)
    torch.cuda.synchronize()
    assert state.clock.tolist()[0] == 12.0
    assert _same(params, params2) and _same(state.moments, state2.moments) and _same(state.clock, state2.clock) and _same(stats, stats2)


def test_argument_errors(env):
    """every refusal of include/mocca.h: a message, nothing launched, and the handle still works"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    p, _, st = _case("tiny", 17)
    dp = _dp(p)
    d, n_head = _device(st), dp.n_head()
    n_floats = n_head + 2 * dp.in_dim
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    params, grad = torch.from_numpy(dp.flat_params()).cuda(), torch.from_numpy(U.gradients(n_head, 1)).cuda()
    state, stats = _state(env, n_head), torch.zeros(2, 8, device="cuda")

    def err(e):
        return (e.lib.mocca_last_error(e.h) or b"").decode()

    def adam(e, h="own", pr=params, nf=n_floats, g=grad, n=n_head, m=state.moments, c=state.clock, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, mx=0.5):
        rc = e.lib.mocca_adam_step(e.h if h == "own" else h, ptr(pr), nf, ptr(g), n, ptr(m), ptr(c), lr, b1, b2, eps, mx, e._stream())
        return rc, err(e)

    def update(e, h="own", obs=d["obs"], stride=5, action=d["action"], old_logp=d["old_logp"], adv=d["adv"], returns=d["returns"], old_value=None,
               rows=17, batch=8, epochs=1, clip=0.2, vc=0.5, ec=0.0, value_clip=0, pr=params, nf=n_floats, n=n_head, m=state.moments,
               c=state.clock, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, mx=0.5, out=stats):
        rc = e.lib.mocca_ppo_update(e.h if h == "own" else h, ptr(obs), stride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value),
                                    rows, batch, epochs, clip, vc, ec, value_clip, ptr(pr), nf, n, ptr(m), ptr(c), lr, b1, b2, eps, mx, 3, ptr(out),
                                    e._stream())
        return rc, err(e)

    fresh = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    for call in (adam, update):
        rc, msg = call(fresh)
        assert rc != 0 and "mocca_set_policy" in msg
    table = np.ascontiguousarray(dp.table(), np.int32)      # shapes only: the image is not filled until mocca_update_policy
    assert fresh.lib.mocca_set_policy(fresh.h, table.ctypes.data_as(C.c_void_p), table.shape[0], 5, 3, 5.0) == 0
    rc, msg = update(fresh)
    assert rc != 0 and "mocca_update_policy" in msg
    fresh.close()
    env.set_policy(dp)
    held = [params.clone(), state.moments.clone(), state.clock.clone()]
    nan, inf = float("nan"), float("inf")
    shared = [dict(pr=None), dict(m=None), dict(c=None), dict(nf=n_head + 1), dict(nf=n_floats - 1), dict(n=0), dict(n=n_head + 1), dict(n=-3),
              dict(lr=nan), dict(lr=inf), dict(lr=-1e-3), dict(eps=nan), dict(eps=inf), dict(eps=-1e-5), dict(b1=1.0), dict(b1=-0.1), dict(b1=nan),
              dict(b2=1.0), dict(b2=-0.1), dict(b2=nan), dict(mx=nan), dict(mx=-0.5)]
    for kw in shared + [dict(g=None)]:
        rc, msg = adam(env, **kw)
        assert rc != 0 and msg.startswith("mocca_adam_step:"), (kw, rc, msg)
    own = [dict(batch=0), dict(batch=18), dict(batch=-1), dict(epochs=0), dict(epochs=-2), dict(rows=0), dict(rows=(1 << 22) + 1, batch=8),
           dict(obs=None), dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(value_clip=1), dict(stride=4),
           dict(clip=nan), dict(clip=-0.1), dict(vc=inf), dict(vc=-1.0), dict(ec=nan), dict(ec=-0.5)]
    for kw in shared + own:
        rc, msg = update(env, **kw)
        assert rc != 0 and msg.startswith("mocca_ppo_update:"), (kw, rc, msg)
    assert adam(env, h=None)[0] != 0 and update(env, h=None)[0] != 0 and env.lib.mocca_last_error(None)
    torch.cuda.synchronize()
    assert _same(params, held[0]) and _same(state.moments, held[1]) and _same(state.clock, held[2])      # nothing was launched
    assert update(env)[0] == 0 and adam(env)[0] == 0      # the handle still works
    torch.cuda.synchronize()
    assert state.clock.tolist()[0] == 3.0 and not _same(params, held[0])
    with pytest.raises(ValueError):
        env.adam_step(params.double(), grad, state)
    with pytest.raises(ValueError):
        env.adam_step(params, grad.cpu(), state)
    with pytest.raises(ValueError):
        env.ppo_update(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], params, state, 18, 1)
    with pytest.raises(ValueError):
        env.ppo_update(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], params, state, 8, 0)


def test_trainer_surface_passes_both_through():
    """TorchVecEnv.ppo_update on [T][N][...] storage equals VecEnv.ppo_update on the flattened rows; adam_step likewise"""
    import torch
    from mocca_envs_amd.rollout import AdamState
    from mocca_envs_amd.trainer_api import make_vec_envs
    p = R.make_policy("ppo", norm=True, seed=1)
    st = R.make_storage(p, 96, seed=2)
    dp = _dp(p)
    envs = make_vec_envs("Walker3DCustomEnv-v0", 1, 8, None, torch.device("cuda:0"))
    envs.attach_policy(dp)
    d = _device(st)
    shaped = {k: v.reshape(12, 8, -1) for k, v in d.items()}
    runs = []
    for store, target in ((shaped, envs), (d, envs.venv)):
        params, state = torch.from_numpy(dp.flat_params()).cuda(), AdamState(dp.n_head(), envs.venv.device)
        target.update_policy(params)
        stats = target.ppo_update(store["obs"], store["action"], store["old_logp"], store["adv"], store["returns"], params, state, 40, 2, seed=4,
                                  **KW)["stats"]
        target.adam_step(params, torch.from_numpy(U.gradients(dp.n_head(), 6)).cuda(), state, n_params=dp.n_head() - dp.act_dim)
        runs.append((params, state.moments, state.clock, stats))
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(*runs))
    envs.close()


def test_ppo_with_the_update_on_the_device_learns_to_stay_up(tmp_path):
    """tests/test_gpu_learning.py's run and thresholds with collection, returns, gradient and the whole update on the device"""
    out = str(tmp_path / "ppo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ppo_demo.py"), "--iters", "130", "--minutes", "5", "--fixed-std", "--log-std", "-1.2",
                        "--device-policy", "--device-returns", "--device-grad", "--device-update", "--out", out], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in open(out + ".jsonl")]
    first, last = lines[0], lines[-1]
    print(first, last)
    assert last["iter"] == 130 and last["env_steps"] == 130 * 4096 * 32
    assert last["mean_length"] > 3 * first["mean_length"] and last["mean_return"] > 150, (first, last)
    assert os.path.exists(out + "_policy.npz")
