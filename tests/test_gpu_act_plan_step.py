"""Training the planner envs' high-level policy on the device: observation statistics for the base controller
(include/mocca.h mocca_set_base_controller_norm) and policy -> base controller -> step as one call (mocca_act_plan_step), up to the trainer
surface.  Every comparison is bit for bit against the calls the new entry points are defined by.  Needs a real MI355X: -m gpu."""
import ctypes as C

import numpy as np
import pytest

import controller_reference as R
import policy_reference as P

pytestmark = pytest.mark.gpu
SCALE = 2.0


def _env(n, ctrl=None, env_id="Walker3DPlannerEnv-v0", seed=5, **kw):
    from mocca_envs_amd.vec_env import VecEnv
    return VecEnv(env_id, n, seed=seed, base_controller=ctrl, **kw)


def _trainer_env(n, ctrl, env_id="Walker3DPlannerEnv-v0", seed=3, **kw):
    from mocca_envs_amd.trainer_api import make_vec_envs
    return make_vec_envs(env_id, seed=seed, num_processes=n, record_events=False, base_controller=ctrl, **kw)


def _dp(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def _plans(n, steps, seed=1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(steps, n, 15, device="cuda", generator=g)


def _stats(seed=0):
    """(mean, inv_std, clip) over the 65 inputs: with robot states within +-5 and scaled plans ~ N(0, 2^2) the clamp at 2 binds on part of the
    entries and leaves the rest alone"""
    rng = np.random.default_rng([seed, 65])
    return rng.normal(0, 1, 65).astype(np.float32), rng.uniform(0.3, 3.0, 65).astype(np.float32), 2.0


def _with_stats(ctrl, seed=0):
    from mocca_envs_amd.controller import BaseController
    mean, inv_std, clip = _stats(seed)
    return BaseController(ctrl.actor, ctrl.critic, obs_mean=mean, obs_inv_std=inv_std, clip=clip)


def _same(u, v):
    a, b = (np.ascontiguousarray(x.cpu().numpy()).reshape(-1).view(np.uint8) for x in (u, v))
    return a.size == b.size and np.array_equal(a, b)


# ---- T1
@pytest.mark.parametrize("kind,n", [("small", 1), ("small", 16), ("small", 33), ("reference", 33)])
def test_normalised_controller_is_the_normalised_policy_bit_for_bit(kind, n):
    """A controller with statistics gives, in plan_step, the bits of the same two nets attached as a DevicePolicy with the same mean, inv_std
    and clip (log_std zeros) and run by act(deterministic) on [robot_state, plan * action_scale] on a second handle.  The clamp binds on some
    entries and not on others, so neither a dropped clamp nor a dropped normalisation passes."""
    import torch
    from mocca_envs_amd.policy import DevicePolicy
    ctrl = R.random_controller(kind, seed=7)
    mean, inv_std, clip = _stats(n)
    env, pol = _env(n), _env(n)
    env.set_base_controller(ctrl, action_scale=SCALE)
    env.set_base_controller_norm(mean, inv_std, clip)
    env.reset(); pol.reset()
    plans = _plans(n, 2, seed=n)
    env.plan_step(plans[0])
    rs = env.obs[:, :50].clone()
    env.plan_step(plans[1])
    act, val = env.base_outputs()
    x = torch.cat([rs, plans[1] * SCALE], 1)
    z = (x.cpu().numpy() - mean) * inv_std
    bound, free = int((np.abs(z) > clip).sum()), int((np.abs(z) < clip).sum())
    assert bound > 0 and free > 0, (bound, free)
    pol.set_policy(DevicePolicy(ctrl.actor, ctrl.critic, np.zeros(R.ACTION, np.float32), obs_mean=mean, inv_std=inv_std, clip=clip))
    out = pol.act(x, deterministic=True, out={"mean": torch.zeros(n, R.ACTION, device="cuda")})
    assert _same(out["mean"], act) and _same(out["value"], val)
    # ... and they are not the bare controller's: without the statistics, or with the clamp far away, the bits differ
    for other in (None, (mean, inv_std, 1e6)):
        pol.set_policy(DevicePolicy(ctrl.actor, ctrl.critic, np.zeros(R.ACTION, np.float32), **({} if other is None else dict(obs_mean=other[0], inv_std=other[1], clip=other[2]))))
        assert not _same(pol.act(x, deterministic=True)["action"], act)
    env.close(); pol.close()


# ---- T2
def test_attach_detach_and_replace_of_the_statistics():
    """attach -> detach gives a never-attached twin's bits; attached statistics change the outputs; set_base_controller with a new controller
    drops them, and so does the Python surface for a controller object that carries none."""
    n = 33
    c1, c2 = R.random_controller("small", seed=1), R.random_controller("small", seed=2)
    mean, inv_std, clip = _stats(3)
    plans = _plans(n, 3, seed=2)

    def run(env):
        env.reset()
        for t in range(3):
            o, r, _, _ = env.plan_step(plans[t])
        return tuple(x.clone() for x in (*env.base_outputs(), o, r))

    A, B, N_ = _env(n, c1), _env(n, c1), _env(n, c1)
    A.set_base_controller_norm(mean, inv_std, clip)
    A.set_base_controller_norm(None, None)
    N_.set_base_controller_norm(mean, inv_std, clip)
    a, b, nn = run(A), run(B), run(N_)
    assert all(_same(u, v) for u, v in zip(a, b))
    assert not _same(nn[0], b[0]) and not _same(nn[1], b[1])          # the statistics are in effect while attached
    # replace: the new controller starts without statistics (C ABI), also when it arrives as an object with them on a handle that had others
    A2, B2 = _env(n, c1), _env(n, c2)
    A2.set_base_controller_norm(mean, inv_std, clip)
    A2.set_base_controller(c2)
    assert all(_same(u, v) for u, v in zip(run(A2), run(B2)))
    A3, B3 = _env(n, _with_stats(c1, seed=3)), _env(n, c1)            # the constructor attaches the object's statistics
    B3.set_base_controller_norm(mean, inv_std, clip)
    assert all(_same(u, v) for u, v in zip(run(A3), run(B3)))
    for e in (A, B, N_, A2, B2, A3, B3):
        e.close()


# ---- T3
@pytest.mark.parametrize("mode,scan", [("noise", False), ("eps", False), ("deterministic", False), ("noise", True)])
def test_act_plan_step_is_act_then_plan_step(mode, scan):
    """A: act_plan_step.  B, a twin: act, then plan_step on its plan.  Plan, logp, value, observation, reward, done, info and the whole state
    are bit-identical in every step of a window in which envs finish and auto-reset.  eps mode reads its input from rows of wider storage
    (in_stride > in_dim); scan: the input is the wide row [obs | scan] of an attached height scan."""
    import torch
    from mocca_envs_amd.perception import scan_grid
    n, steps = 33, 150
    ctrl = _with_stats(R.random_controller("small", seed=4), seed=4)
    A, B = _env(n, ctrl, seed=11), _env(n, ctrl, seed=11)
    width = 52
    if scan:
        pts = scan_grid((0.2, 1.4), (-0.4, 0.4), 4, 3)
        for e in (A, B):
            e.set_height_scan(pts)
        width = 52 + A.scan_dim
        assert width == 64
    p = _dp(P.random_policy("small", width, 15, norm=True, seed=9))
    for e in (A, B):
        e.set_policy(p)
        e.reset()
    stride = width + 12 if mode == "eps" else width
    rows = {e: torch.full((n, stride), float("nan"), device="cuda") for e in (A, B)}
    g = torch.Generator(device="cuda").manual_seed(5)
    z = lambda *s: torch.zeros(*s, device="cuda")
    pa, la, va = z(n, 15), z(n), z(n)
    finished = 0
    for t in range(steps):
        eps = torch.randn(n, 15, device="cuda", generator=g) if mode == "eps" else None
        ins = {}
        for e in (A, B):
            if scan:
                e.height_scan(out=rows[e], obs=e.obs)
            else:
                rows[e][:, :52].copy_(e.obs)
            ins[e] = rows[e][:, :width]
        oa, ra, da, ia = A.act_plan_step(ins[A], eps=eps, deterministic=mode == "deterministic", plan_out=pa, logp_out=la, value_out=va)
        out = B.act(ins[B], eps=eps, deterministic=mode == "deterministic")
        ob, rb, db, ib = B.plan_step(out["action"])
        for name, u, v in (("plan", pa, out["action"]), ("logp", la, out["logp"]), ("value", va, out["value"]), ("obs", oa, ob), ("rew", ra, rb),
                           ("done", da, db), ("info", ia, ib), ("state", A.get_state(), B.get_state())):
            assert _same(u, v), (t, name)
        finished += int((da != 0).sum())
    assert finished > 0                                               # envs ended and auto-reset inside the window
    assert all(_same(u, v) for u, v in zip(A.base_outputs(), B.base_outputs())) and _same(A.get_task(), B.get_task())
    assert _same(A.last_action, pa) and bool(torch.isfinite(la).all()) and float(pa.abs().max()) > 0
    A.close(); B.close()


# ---- T4
def test_captured_rollout_of_the_planner_policy_replays_like_eager_and_sees_update_policy():
    """capture_rollout(policy=None) on a planner env: every step of the graph is act_plan_step; replays equal an eager twin bit for bit, and
    update_policy between replays changes what the graph computes without a recapture."""
    import torch
    n, T = 33, 4
    ctrl = _with_stats(R.random_controller("small", seed=1), seed=1)
    p1, p2 = _dp(P.random_policy("small", 52, 15, norm=True, seed=12)), _dp(P.random_policy("small", 52, 15, norm=True, seed=13))

    def storage():
        z = lambda *s: torch.zeros(*s, device="cuda")
        return {"obs": z(T + 1, n, 52), "reward": z(T, n, 1), "masks": torch.ones(T + 1, n, 1, device="cuda"), "bad_masks": torch.ones(T + 1, n, 1, device="cuda"),
                "action": z(T, n, 15), "logp": z(T, n, 1), "value": z(T, n, 1)}

    def row(S):
        return lambda t: {"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1], "bad_masks": S["bad_masks"][t + 1],
                          "action": S["action"][t], "logp": S["logp"][t], "value": S["value"][t]} if t >= 0 else {"obs": S["obs"][0]}

    A, B = _trainer_env(n, ctrl, seed=5), _trainer_env(n, ctrl, seed=5)
    SA, SB = storage(), storage()
    for e in (A, B):
        e.attach_policy(p1)
    SA["obs"][0].copy_(A.reset())
    B.reset()
    graph = B.capture_rollout(num_steps=T, into=row(SB), warmup=2)      # two eager warm-up steps advance B
    for t in range(2):                                                   # ... so A takes the same two
        A.act_step(SA["obs"][0], into={"obs": SA["obs"][0]})
    assert _same(SA["obs"][0], SB["obs"][0])
    for second in (False, True):
        if second:
            for e, S in ((A, SA), (B, SB)):
                e.update_policy(p2)
                S["obs"][0].copy_(S["obs"][T])
        for t in range(T):
            A.act_step(SA["obs"][t], into=row(SA)(t))
        graph.replay()
        torch.cuda.synchronize()
        for k in SA:
            assert _same(SA[k], SB[k]), (second, k)
        assert _same(A.episode_totals, B.episode_totals) and _same(A.venv.get_state(), B.venv.get_state())
        assert float(SB["action"].abs().max()) > 0 and float(SB["reward"].abs().max()) > 0
    # the second replay ran the second policy: its value for the stored observation is in the row, the first policy's is not
    v2 = B.venv.act(SB["obs"][0], deterministic=True)["value"].clone()
    assert _same(v2, SB["value"][0].reshape(-1))
    B.update_policy(p1)
    assert not _same(B.venv.act(SB["obs"][0], deterministic=True)["value"], v2)
    A.close(); B.close()


# ---- T5
def _msg(env, h=True):
    m = env.lib.mocca_last_error(env.h if h else None)
    return m.decode() if m else ""


def test_errors_of_the_statistics_leave_the_handle_as_it_was():
    """every refusal of mocca_set_base_controller_norm is MOCCA_E_ARG with a message; after each the handle (statistics attached) still steps
    and gives the bits of a twin that saw no refused call"""
    n = 16
    ctrl = R.random_controller("small", seed=3)
    mean, inv_std, clip = _stats(5)
    A, B = _env(n, ctrl), _env(n, ctrl)
    for e in (A, B):
        e.set_base_controller_norm(mean, inv_std, clip)
        e.reset()
    plans = _plans(n, 16, seed=3)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def changed(arr, k, v):
        out = arr.copy(); out[k] = v
        return out

    nan, inf = float("nan"), float("inf")
    cases = [(mean, None, clip), (None, inv_std, clip), (changed(mean, 64, nan), inv_std, clip), (changed(mean, 0, inf), inv_std, clip),
             (mean, changed(inv_std, 3, nan), clip), (mean, changed(inv_std, 64, inf), clip), (mean, changed(inv_std, 10, -0.5), clip),
             (mean, inv_std, nan), (mean, inv_std, inf), (mean, inv_std, 0.0), (mean, inv_std, -1.0)]
    for t, (m, s, c) in enumerate(cases):
        rc = A.lib.mocca_set_base_controller_norm(A.h, ptr(m), ptr(s), c)
        assert rc == -1 and _msg(A).startswith("mocca_set_base_controller_norm:"), (t, rc, _msg(A))
        oa, ra, _, _ = A.plan_step(plans[t]); ob, rb, _, _ = B.plan_step(plans[t])
        assert _same(oa, ob) and _same(ra, rb) and all(_same(u, v) for u, v in zip(A.base_outputs(), B.base_outputs())), t
    assert A.lib.mocca_set_base_controller_norm(None, ptr(mean), ptr(inv_std), clip) == -1 and _msg(A, h=False)
    bare = _env(n)                                                    # no controller attached
    assert bare.lib.mocca_set_base_controller_norm(bare.h, ptr(mean), ptr(inv_std), clip) == -1 and "needs a base controller" in _msg(bare)
    assert bare.lib.mocca_set_base_controller_norm(bare.h, None, None, clip) == -1
    from mocca_envs_amd import lib as L
    with pytest.raises(L.MoccaError):
        bare.set_base_controller_norm(mean, inv_std, clip)
    with pytest.raises(ValueError):
        A.set_base_controller_norm(mean[:64], inv_std[:64], clip)
    bare.reset()
    bare.step(bare.obs.new_zeros(n, 21))
    for e in (A, B, bare):
        e.close()


def test_errors_of_act_plan_step_launch_nothing():
    """every refusal of mocca_act_plan_step is MOCCA_E_ARG with a message and launches nothing: the outputs keep their sentinel, and after
    each the handle still steps and gives the bits of a twin that saw no refused call"""
    import torch
    from mocca_envs_amd import lib as L
    n = 16
    ctrl = R.random_controller("small", seed=3)
    p = _dp(P.random_policy("small", 52, 15, norm=True, seed=2))
    A, B = _env(n, ctrl), _env(n, ctrl)
    for e in (A, B):
        e.set_policy(p)
        e.reset()
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    buf = dict(plan=f(n, 15), logp=f(n), value=f(n), mean=f(n, 15), obs=f(n, 52), rew=f(n))
    done, info = torch.full((n,), 7, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.int32, device="cuda")
    held = {k: v.clone() for k, v in buf.items()}

    def call(env, h=True, **kw):
        a = dict(inp=env.obs, stride=52, plan=buf["plan"], obs=buf["obs"], rew=buf["rew"], done=done)
        a.update(kw)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return env.lib.mocca_act_plan_step(env.h if h else None, ptr(a["inp"]), a["stride"], None, 0, ptr(a["plan"]), ptr(buf["logp"]), ptr(buf["value"]),
                                           ptr(buf["mean"]), ptr(a["obs"]), ptr(a["rew"]), ptr(a["done"]), ptr(info), None)

    def untouched_and_alive(t):
        torch.cuda.synchronize()
        assert all(_same(buf[k], held[k]) for k in buf) and int(done.min()) == 7 and int(info.min()) == 7, t
        oa, ra, _, _ = A.act_plan_step(A.obs); ob, rb, _, _ = B.act_plan_step(B.obs)
        assert _same(oa, ob) and _same(ra, rb) and _same(A.last_action, B.last_action) and _same(A.get_state(), B.get_state()), t

    # mocca_act's own and mocca_plan_step's own, with a policy and a controller in place
    for t, kw in enumerate((dict(inp=None), dict(plan=None), dict(stride=51), dict(obs=None), dict(rew=None), dict(done=None))):
        rc = call(A, **kw)
        assert rc == -1 and _msg(A).startswith("mocca_act_plan_step"), (kw, rc, _msg(A))
        untouched_and_alive(t)
    assert call(A, h=False) == -1
    # a policy whose actions are not plans
    A.set_policy(_dp(P.random_policy("small", 52, 21, norm=True, seed=2)))
    assert call(A) == -1 and "act_dim" in _msg(A)
    with pytest.raises(L.MoccaError, match="act_dim"):
        A.act_plan_step(A.obs)
    A.set_policy(p)
    untouched_and_alive("act_dim")
    # no policy; a policy that has not been filled is mocca_act's own error too
    A.set_policy(None)
    assert call(A) == -1 and "needs a policy" in _msg(A)
    with pytest.raises(L.MoccaError):
        A.act_plan_step(A.obs)
    A.set_policy(p)
    untouched_and_alive("no policy")
    # no base controller
    C_ = _env(n)
    C_.set_policy(p)
    C_.reset()
    assert call(C_) == -1 and "needs a base controller" in _msg(C_)
    with pytest.raises(L.MoccaError, match="needs a base controller"):
        C_.act_plan_step(C_.obs)
    C_.step(torch.zeros(n, 21, device="cuda"))
    # global env ids beyond 2^28: mocca_act's own
    far = _env(n, ctrl, env_offset=(1 << 28) - 8)
    far.set_policy(p)
    assert call(far) == -1 and "2^28" in _msg(far)
    # not the planner task
    other = _env(n, env_id="Walker3DCustomEnv-v0")
    other.set_policy(p)
    other.reset()
    assert call(other) == -1 and "planner task" in _msg(other)
    with pytest.raises(ValueError, match="planner envs only"):
        other.act_plan_step(other.obs)
    other.step(torch.zeros(n, 21, device="cuda"))
    torch.cuda.synchronize()
    assert all(_same(buf[k], held[k]) for k in buf)
    for e in (A, B, C_, far, other):
        e.close()


# ---- T6
def test_trainer_surface_attaches_a_plan_policy_and_fills_the_rows():
    import torch
    n = 33
    ctrl = _with_stats(R.random_controller("small", seed=1), seed=2)
    envs, twin = _trainer_env(n, ctrl), _trainer_env(n, ctrl)
    assert envs.action_space.shape == (15,)
    with pytest.raises(ValueError, match="52 -> 21"):
        envs.attach_policy(_dp(P.random_policy("small", 52, 21, norm=True, seed=1)))
    with pytest.raises(ValueError):
        envs.attach_policy(_dp(P.random_policy("small", 65, 15, norm=True, seed=1)))
    p = _dp(P.random_policy("small", 52, 15, norm=True, seed=1))
    envs.attach_policy(p)
    twin.venv.set_policy(p)
    obs = envs.reset()
    ot = twin.reset()
    z = lambda *s: torch.zeros(*s, device="cuda")
    rows = {"action": z(n, 15), "logp": z(n, 1), "value": z(n, 1), "obs": z(n, 52), "reward": z(n, 1)}
    for t in range(3):
        o, r, _, _ = envs.act_step(obs, into=rows)
        assert o is rows["obs"] and r is rows["reward"]
        out = twin.venv.act(ot)
        ot, rt, _, _ = twin.step(out["action"])
        assert _same(rows["action"], out["action"]) and _same(rows["logp"], out["logp"]) and _same(rows["value"], out["value"])
        assert _same(o, ot) and _same(r, rt) and _same(envs.masks, twin.masks) and _same(envs.episode_totals, twin.episode_totals)
        obs = o
    assert rows["action"].shape == (n, 15) and float(rows["action"].abs().min(dim=1).values.max()) > 0 and float(rows["logp"].abs().max()) > 0
    envs.attach_policy(None)
    envs.close(); twin.close()


# ---- T7
def test_one_ppo_iteration_on_a_planner_env_end_to_end():
    """collection (act_step x T), finish_rollout, update_obs_stats and ppo_update as they stand, on the 52 -> 15 policy of a planner env"""
    import torch
    from mocca_envs_amd.rollout import AdamState, ObsStats
    n, T = 64, 8
    ctrl = _with_stats(R.random_controller("small", seed=6), seed=6)
    envs = _trainer_env(n, ctrl, seed=2)
    dp = _dp(P.random_policy("small", 52, 15, norm=True, seed=3))
    envs.attach_policy(dp)
    dev = envs.device
    z = lambda *s: torch.zeros(*s, device=dev)
    S = {"obs": z(T + 1, n, 52), "reward": z(T, n, 1), "masks": torch.ones(T + 1, n, 1, device=dev), "bad_masks": torch.ones(T + 1, n, 1, device=dev),
         "action": z(T, n, 15), "logp": z(T, n, 1), "value": z(T + 1, n, 1)}
    params = torch.from_numpy(dp.flat_params()).to(dev)
    n_head = dp.n_head()
    assert params.numel() == n_head + 2 * 52
    stats = ObsStats(52, dev, eps=1e-8)
    S["obs"][0].copy_(envs.reset())
    envs.update_obs_stats(stats, S["obs"][:1], mean_out=params[n_head:n_head + 52], inv_std_out=params[n_head + 52:])
    envs.update_policy(params)
    before = params.clone()
    for t in range(T):
        envs.act_step(S["obs"][t], into={"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1], "bad_masks": S["bad_masks"][t + 1],
                                         "action": S["action"][t], "logp": S["logp"][t], "value": S["value"][t]})
    envs.venv.act(S["obs"][T], deterministic=True, out={"value": S["value"][T]})
    fin = envs.finish_rollout(S["reward"], S["value"], S["masks"], S["bad_masks"], 0.99, 0.95, 0.1)
    envs.update_obs_stats(stats, S["obs"][1:], mean_out=params[n_head:n_head + 52], inv_std_out=params[n_head + 52:])
    st = envs.ppo_update(S["obs"][:T], S["action"], S["logp"], fin["adv"], fin["returns"], params, AdamState(n_head, dev), 128, 1, seed=1)["stats"]
    torch.cuda.synchronize()
    assert st.shape == (4, 8) and bool(torch.isfinite(st).all())
    assert int((st[:, 6] == 0).sum()) == 0                            # no skipped step
    assert bool(torch.isfinite(params).all()) and bool(torch.isfinite(fin["adv"]).all()) and bool(torch.isfinite(S["logp"]).all())
    assert not _same(params[:n_head], before[:n_head]) and not _same(params[n_head:], before[n_head:])
    assert float(S["action"].abs().max()) > 0 and float(S["reward"].abs().max()) > 0
    envs.close()
