"""The planner envs' base controller on the device (ABI 8): `plan_step` = controller kernel + step kernel, the critic's value inside the
reward.  Checked against an independent float64 forward (tests/controller_reference.py) and against the same handle stepped through
`step()` on the controller's own actions.  Needs a real MI355X: -m gpu."""
import json
import os

import numpy as np
import pytest

import controller_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(n, ctrl=None, env_id="MikePlannerEnv-v0", seed=5, **kw):
    from mocca_envs_amd.vec_env import VecEnv
    return VecEnv(env_id, n, seed=seed, base_controller=ctrl, **kw)


def _plans(n, steps, seed=1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(steps, n, 15, device="cuda", generator=g)


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
@pytest.mark.parametrize("n", [1, 63, 4096])
def test_controller_parity_with_the_f64_forward(kind, n):
    """Yardstick: torch CPU float32 forward vs the float64 helper on the same inputs, in units of 1e-6 (1 + |x|); the kernel stays within
    3 x that at the median, the 99th percentile and the maximum.  A dropped bias, a swapped activation or action_scale 1 do not.

    With MOCCA_TEST_OUT=<dir> both triples of every case are written to <dir>/controller_parity.json (profiles/controller_parity.json)."""
    import torch
    ctrl = R.random_controller(kind, seed=7)
    env = _env(n, ctrl)
    env.reset()
    plans = _plans(n, 4, seed=n)
    for t in range(3):
        env.plan_step(plans[t])
    rs = env.obs[:, :50].cpu().numpy().copy()
    env.plan_step(plans[3])
    act, val = (x.cpu().numpy() for x in env.base_outputs())
    plan = plans[3].cpu().numpy()
    v64, a64 = R.forward64(ctrl, rs, plan)
    acts = {"relu": torch.relu, "tanh": torch.tanh, "softsign": torch.nn.functional.softsign, "identity": lambda t: t}

    def net32(layers, x):
        for w, b, a in layers:
            x = acts[a](torch.nn.functional.linear(x, torch.from_numpy(w), torch.from_numpy(b)))
        return x.numpy()

    x32 = torch.from_numpy(R.base_obs(rs, plan).astype(np.float32))
    cat = lambda a, v: np.concatenate([np.asarray(a).ravel(), np.asarray(v).ravel()])
    want = cat(a64, v64)
    yard = R.triple(R.error_units(cat(net32(ctrl.actor, x32), net32(ctrl.critic, x32)[:, 0]), want))
    got = R.triple(R.error_units(cat(act, val), want))
    print(f"\n{kind} n={n}: kernel vs f64 median/p99/max {got}, torch f32 vs f64 {yard}")
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: the measured triples are appended there (profiles/controller_parity.json)
    if out:
        path = os.path.join(out, "controller_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {
            "what": "tests/test_gpu_planner_controller.py::test_controller_parity_with_the_f64_forward: error against the float64 forward "
                    "in units of 1e-6 (1 + |x|), [median, p99, max]", "cases": {}}
        doc["cases"][f"{kind}-{n}"] = {"kernel_vs_f64": got, "torch_f32_vs_f64": yard}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    ok = lambda g: all(g[i] <= 3.0 * yard[i] for i in range(3))
    assert ok(got), (got, yard)
    for how in ("bias", "activation", "scale"):
        if how == "activation" and not any(a in ("relu", "softsign") for _, _, a in ctrl.actor + ctrl.critic):
            continue
        vm, am = R.forward64(ctrl, rs, plan, action_scale=1.0) if how == "scale" else R.forward64(R.mutated(ctrl, how), rs, plan)
        assert not ok(R.triple(R.error_units(cat(act, val), cat(am, vm)))), how
    env.close()


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
@pytest.mark.parametrize("n", [1, 17, 63])
def test_base_outputs_are_the_policy_kernels_bits(kind, n):
    """The controller is the deterministic, unnormalised case of a trainer's policy: the same two nets attached as a `DevicePolicy` (log_std
    zeros) and run by act() on [robot_state, plan * action_scale] give plan_step's base outputs bit for bit.  n: one env, a 16-env tile
    boundary, a ragged last tile."""
    import torch
    from mocca_envs_amd.policy import DevicePolicy
    ctrl, scale = R.random_controller(kind, seed=7), 2.0
    env = _env(n)
    env.set_base_controller(ctrl, action_scale=scale)
    env.reset()
    plans = _plans(n, 2, seed=n)
    env.plan_step(plans[0])
    rs = env.obs[:, :50].clone()
    env.plan_step(plans[1])
    act, val = env.base_outputs()
    env.set_policy(DevicePolicy(ctrl.actor, ctrl.critic, np.zeros(R.ACTION, np.float32)))
    out = env.act(torch.cat([rs, plans[1] * scale], 1), deterministic=True)
    assert torch.equal(out["action"], act) and torch.equal(out["value"], val)
    env.close()


@pytest.mark.parametrize("env_id", ["MikePlannerEnv-v0", "Walker3DPlannerEnv-v0"])
def test_plan_step_is_controller_plus_step_and_monitor_sees_the_reward(env_id):
    """A: plan_step(plan).  B: step(A's controller actions).  Everything but the reward identical in every step and env; A's reward is B's
    progress + log(max(1, value)) / 3; the episode records' returns are the float32 sums of A's rewards in step order."""
    import torch
    n, steps = 4096, 200
    ctrl = R.random_controller("reference", seed=2)
    A, B = _env(n, ctrl, env_id), _env(n, ctrl, env_id)
    C_ = _env(n, None, env_id)             # no controller at all: must equal B (controller attached, stepped through step())
    ep = A.episode_stats(True, slots=steps + 1)
    oa, ob = A.reset(), B.reset()
    C_.reset()
    assert torch.equal(oa, ob)
    plans = _plans(n, steps)
    ret = np.zeros(n, np.float32)
    hi = lo = total = episodes = 0
    for t in range(steps):
        rs = A.obs[:, :50].clone()
        o1, r1, d1, i1 = A.plan_step(plans[t])
        act, val = A.base_outputs()
        o2, r2, d2, i2 = B.step(act)
        o3, r3, d3, _ = C_.step(act)
        assert torch.equal(o1, o2) and torch.equal(d1, d2) and torch.equal(i1, i2), t
        assert torch.equal(o2, o3) and torch.equal(r2, r3) and torch.equal(d2, d3), t
        v = val.cpu().numpy().astype(np.float64)
        want = r2.cpu().numpy().astype(np.float64) + np.log(np.maximum(1.0, v)) / 3.0
        got = r1.cpu().numpy()
        assert (np.abs(got - want) <= 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all(), t
        hi += int((v > 1).sum()); lo += int((v <= 1).sum()); total += n
        # Monitor: float32 accumulation in step order
        ret = (ret + got).astype(np.float32)
        torch.cuda.synchronize()
        rec = ep["records"][(ep["first_serial"] + t) % ep["slots"]].numpy()
        fin = np.nonzero(d1.cpu().numpy())[0]
        assert (rec[fin, 0] == ep["first_serial"] + t).all()
        assert (rec[fin, 1].view(np.float32) == ret[fin]).all(), t
        episodes += fin.size
        ret[fin] = 0.0
        assert torch.equal(A.get_state(), B.get_state()) and torch.equal(A.get_task(), B.get_task()), t
        # the controller's input was the robot part of the observation the step before returned (auto-reset: the new episode's first)
        if t in (0, 120):
            v64, a64 = R.forward64(ctrl, rs.cpu().numpy(), plans[t].cpu().numpy())
            assert R.triple(R.error_units(act.cpu().numpy(), a64))[2] < 100.0
    assert hi >= 0.1 * total and lo >= 0.1 * total, (hi, lo, total)
    assert episodes > n // 4
    for e in (A, B, C_):
        e.close()


def _probe():
    """identity-like controller: the actor's single layer copies inputs 0..20 to its outputs, the critic's copies input 49"""
    from types import SimpleNamespace
    wa = np.zeros((21, 65), np.float32); wa[np.arange(21), np.arange(21)] = 1.0
    wc = np.zeros((1, 65), np.float32); wc[0, 49] = 1.0
    return SimpleNamespace(actor=[(wa, np.zeros(21, np.float32), "identity")], critic=[(wc, np.zeros(1, np.float32), "identity")])


def _probe2():
    """... inputs 29..49 (the rest of robot_state) and input 64 = plan[14] x action_scale"""
    from types import SimpleNamespace
    wa = np.zeros((21, 65), np.float32); wa[np.arange(21), 29 + np.arange(21)] = 1.0
    wc = np.zeros((1, 65), np.float32); wc[0, 64] = 1.0
    return SimpleNamespace(actor=[(wa, np.zeros(21, np.float32), "identity")], critic=[(wc, np.zeros(1, np.float32), "identity")])


@pytest.mark.parametrize("probe", [_probe, _probe2])
def test_the_controllers_input_is_the_last_observation_bit_for_bit(probe):
    import torch
    n = 512
    env = _env(n, probe(), seed=9)
    lo = 0 if probe is _probe else 29
    obs = env.reset().clone()
    plans = _plans(n, 80, seed=4)
    elsewhere = torch.zeros(n, env.obs_dim, device="cuda")
    resets = 0
    for t in range(80):
        into = elsewhere if t % 2 else None                     # obs_out= pointing elsewhere must not matter
        o, _, d, _ = env.plan_step(plans[t], obs_out=into)
        act, val = env.base_outputs()
        assert torch.equal(act, obs[:, lo:lo + 21]), t          # the input of THIS step: the observation the step before returned
        assert torch.equal(val, obs[:, 49] if probe is _probe else plans[t][:, 14] * 2.0), t
        obs = o.clone()
        resets += int((d != 0).sum())
    assert resets > 0                                           # auto-resets happened: the next input was the new episode's first observation
    # set_state + observe
    st = env.get_state()
    st[:, 7:10] += 0.25
    env.set_state(st)
    obs = env.observe().clone()
    env.plan_step(plans[0])
    assert torch.equal(env.base_outputs()[0], obs[:, lo:lo + 21])
    env.close()


def test_graph_capture_determinism_and_batch_independence():
    import torch
    ctrl = R.random_controller("reference", seed=4)
    n = 4096
    plans = _plans(n, 200, seed=6)
    A, B = _env(n, ctrl, seed=3), _env(n, ctrl, seed=3)
    A.reset(); B.reset()
    for t in range(200):
        A.plan_step(plans[t]); B.plan_step(plans[t])
    assert torch.equal(A.obs, B.obs) and torch.equal(A.rew, B.rew) and torch.equal(A.get_state(), B.get_state())
    # N = 1 and N = 63 are the same envs as inside the 4096 batch (env_offset)
    for m, off in ((1, 77), (63, 1000)):
        big, small = _env(n, ctrl, seed=8), _env(m, ctrl, seed=8, env_offset=off)
        big.reset(); small.reset()
        for t in range(40):
            big.plan_step(plans[t]); small.plan_step(plans[t][off:off + m].contiguous())
        assert torch.equal(big.obs[off:off + m], small.obs) and torch.equal(big.rew[off:off + m], small.rew)
        a1, v1 = big.base_outputs(); a2, v2 = small.base_outputs()
        assert torch.equal(a1[off:off + m], a2) and torch.equal(v1[off:off + m], v2)
        big.close(); small.close()
    # 10 plan_steps captured and replayed == the eager run (A and B are in the same state here)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(2):
            A.plan_step(plans[t]); B.plan_step(plans[t])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rews = torch.zeros(10, n, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(10):
            A.plan_step(plans[10 + t], rew_out=rews[t])
    g.replay()
    for t in range(10):
        assert torch.equal(B.plan_step(plans[10 + t])[1], rews[t]), t
    assert torch.equal(A.obs, B.obs) and torch.equal(A.get_state(), B.get_state()) and torch.equal(A.get_task(), B.get_task())
    A.close(); B.close()


def test_errors_are_codes_and_messages_never_crashes():
    from types import SimpleNamespace
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    good = R.random_controller("small")
    env = _env(8)
    with pytest.raises(L.MoccaError, match="needs a base controller"):
        env.plan_step(torch.zeros(8, 15, device="cuda"))
    bad_width = SimpleNamespace(actor=[(np.zeros((40, 65), np.float32), np.zeros(40, np.float32), "relu"), (np.zeros((21, 40), np.float32), np.zeros(21, np.float32), "identity")], critic=good.critic)
    with pytest.raises(L.MoccaError, match="multiples of 16"):
        env.set_base_controller(bad_width)
    wrong_out = SimpleNamespace(actor=good.critic, critic=good.critic)
    with pytest.raises(L.MoccaError, match="21 outputs"):
        env.set_base_controller(wrong_out)
    wrong_in = SimpleNamespace(actor=[(np.zeros((21, 64), np.float32), np.zeros(21, np.float32), "identity")], critic=good.critic)
    with pytest.raises(L.MoccaError, match="65-float input"):
        env.set_base_controller(wrong_in)
    env.set_base_controller(good)
    env.reset()
    env.plan_step(torch.zeros(8, 15, device="cuda"))
    env.set_base_controller(None)
    with pytest.raises(L.MoccaError):
        env.plan_step(torch.zeros(8, 15, device="cuda"))
    env.close()
    other = VecEnv("Walker3DCustomEnv-v0", 8)
    with pytest.raises(L.MoccaError, match="planner task"):
        other.set_base_controller(good)
    other.close()


def test_trainer_surface_takes_plans():
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    n = 256
    ctrl = R.random_controller("small", seed=1)
    envs = make_vec_envs("MikePlannerEnv-v0", 4, n, None, base_controller=ctrl)
    twin = make_vec_envs("MikePlannerEnv-v0", 4, n, None, base_controller=ctrl)
    assert envs.action_space.shape == (15,) and not np.isfinite(envs.action_space.high).any()
    assert torch.equal(envs.reset(), twin.reset())
    plans = _plans(n, 150, seed=2)
    into = {"obs": torch.zeros(n, envs.venv.obs_dim, device="cuda"), "reward": torch.zeros(n, 1, device="cuda")}
    ret, seen = np.zeros(n, np.float32), 0
    for t in range(150):
        obs, rew, done, infos = envs.step(plans[t])
        o2, r2, _, _ = twin.step(plans[t], into=into)
        assert torch.equal(obs, o2) and torch.equal(rew, r2) and rew.shape == (n, 1)
        ret = (ret + rew[:, 0].cpu().numpy()).astype(np.float32)
        for i, info in infos.finished():
            assert np.float32(info["episode"]["r"]) == ret[i]
            ret[i] = 0.0
            seen += 1
    assert seen > 0
    envs.close(); twin.close()


def test_captured_rollout_takes_plans():
    """TorchVecEnv.capture_rollout with a controller: the graph's launches go through plan_step and replay what eager steps compute."""
    import torch
    from mocca_envs_amd.controller import BaseController
    from mocca_envs_amd.trainer_api import make_vec_envs
    n, steps = 512, 6
    c = R.random_controller("small", seed=1)
    ctrl = BaseController.from_layers(c.actor, c.critic)
    envs = make_vec_envs("MikePlannerEnv-v0", 4, n, None, base_controller=ctrl)
    twin = make_vec_envs("MikePlannerEnv-v0", 4, n, None, base_controller=ctrl)
    envs.reset(); twin.reset()
    plans = _plans(n, steps + 2, seed=3)
    kept = torch.zeros(steps, n, envs.venv.obs_dim + 1, device="cuda")

    def sink(t, obs, rew, masks, bad_masks, action):
        assert action.shape == (n, 15)
        kept[t, :, :-1].copy_(obs); kept[t, :, -1:].copy_(rew)

    graph = envs.capture_rollout(lambda obs, t: plans[t], steps, sink=sink, warmup=2)     # the warm-up advances the envs by plans[0], plans[1]
    for t in range(2):
        twin.step(plans[t])
    graph.replay()
    torch.cuda.synchronize()
    for t in range(steps):
        obs, rew, _, _ = twin.step(plans[t])
        assert torch.equal(kept[t, :, :-1], obs) and torch.equal(kept[t, :, -1:], rew), t
    assert torch.equal(envs.venv.get_state(), twin.venv.get_state()) and torch.equal(envs.venv.get_task(), twin.venv.get_task())
    envs.close(); twin.close()


def test_single_env_class_takes_a_base_controller_object():
    """Walker3DPlannerEnv(base_controller=BaseController(...)) goes through the callable protocol: the same episode as with a plain
    function around the same layers, and the reward carries the value term computed on the host."""
    from mocca_envs_amd.controller import BaseController
    from mocca_envs_amd.envs import Walker3DPlannerEnv
    c = R.random_controller("small", seed=2)
    ctrl = BaseController.from_layers(c.actor, c.critic)
    seen = []

    def plain(base_obs):
        value, action = ctrl(base_obs)
        seen.append(float(value))
        return value, action

    a, b = Walker3DPlannerEnv(base_controller=ctrl), Walker3DPlannerEnv(base_controller=plain)
    a.seed(3); b.seed(3)
    assert np.array_equal(a.reset(), b.reset())
    rng = np.random.default_rng(0)
    for t in range(5):
        plan = rng.normal(0, 1, 15)
        oa, ra, da, _ = a.step(plan)
        ob, rb, db, _ = b.step(plan)
        assert np.array_equal(oa, ob) and ra == rb and da == db
        assert abs(ra - (a.progress + np.log(max(1.0, seen[-1])) / 3)) < 1e-12
    with pytest.raises(RuntimeError):
        Walker3DPlannerEnv().step(np.zeros(15))
    a.close(); b.close()
