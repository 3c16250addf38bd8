"""The device policy on the GPU (include/mocca.h mocca_set_policy / mocca_update_policy / mocca_act / mocca_act_step): mean and value against an
independent float64 forward, the sample and its log-probability, the in-kernel noise against a numpy restatement of its keying, act_step as
act + step, graph capture, the trainer surface and the argument errors.  The checker is tests/policy_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import policy_reference as R

pytestmark = pytest.mark.gpu
NS = (1, 17, 63, 100)      # one env, one past the 16-env tile, odd, several workgroups


def _dp(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def _env(n, env_id="Walker3DCustomEnv-v0", **kw):
    from mocca_envs_amd.vec_env import VecEnv
    return VecEnv(env_id, n, device=0, **kw)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bits(x):
    """the bytes of a tensor or array: equal bytes = equal bits"""
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def _record(name, key, value):
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: measured figures are collected there (profiles/policy_parity.json)
    if not out:
        return
    path = os.path.join(out, "policy_parity.json")
    doc = json.load(open(path)) if os.path.exists(path) else {
        "what": "tests/test_gpu_policy.py: errors in units of 1e-6 (1 + |x|) as [median, p99, max] against the float64 reference, kernel and "
                "float32 yardstick; noise: absolute errors of eps", "parity": {}, "sample": {}, "noise": {}}
    doc[name][key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _ok(got, yard):
    return all(got[i] <= 3.0 * yard[i] for i in range(3))


def _inputs(n, in_dim, strided):
    """device rows [n, in_dim]; strided: a view of wider storage (in_stride > in_dim) whose other floats are poison"""
    import torch
    x = R.plausible_inputs(n, in_dim, seed=n)
    if not strided:
        return x, torch.from_numpy(x).cuda()
    wide = torch.full((n, in_dim + 19), float("nan"), device="cuda")
    wide[:, :in_dim] = torch.from_numpy(x).cuda()
    return x, wide[:, :in_dim]


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
@pytest.mark.parametrize("n", NS)
def test_mean_and_value_parity_with_the_f64_forward(kind, n):
    """The controller test's rule: error against the float64 forward in units of 1e-6 (1 + |x|); yardstick torch CPU float32 on the same
    inputs; the kernel stays within 3 x the yardstick at the median, the 99th percentile and the maximum -- for every (in_dim, A), with the
    normalisation on and off.  Every mutation of the reference (dropped normalisation, ignored clip, wrong activation) fails the same rule.
    With MOCCA_TEST_OUT=<dir> the triples go to <dir>/policy_parity.json (profiles/policy_parity.json)."""
    import torch
    env = _env(n)
    cat = lambda m, v: np.concatenate([np.asarray(m).ravel(), np.asarray(v).ravel()])
    failures = []
    for in_dim, act_dim in R.DIMS:
        for norm in (True, False):
            p = R.random_policy(kind, in_dim, act_dim, norm=norm, seed=11)
            env.set_policy(_dp(p))
            x, xd = _inputs(n, in_dim, strided=in_dim == 142)
            out = _np(env.act(xd, deterministic=True, out={"mean": torch.empty(n, act_dim, device="cuda")}))
            m64, v64 = R.forward64(p, x)
            want = cat(m64, v64)
            yard = R.triple(R.error_units(cat(*R.torch32(p, x)), want))
            got = R.triple(R.error_units(cat(out["mean"], out["value"]), want))
            key = f"{kind}-n{n}-in{in_dim}-a{act_dim}-{'norm' if norm else 'raw'}"
            print(f"{key}: kernel vs f64 median/p99/max {got}, torch f32 vs f64 {yard}")
            _record("parity", key, {"kernel_vs_f64": got, "torch_f32_vs_f64": yard})
            if not _ok(got, yard):
                failures.append((key, got, yard))
            if not np.array_equal(_bits(out["action"]), _bits(out["mean"])):
                failures.append((key, "deterministic action != mean"))
            for how in ("no_norm", "no_clip", "activation") if norm else ("activation",):
                mm, vm = R.forward64(R.mutated(p, how), x)
                if _ok(R.triple(R.error_units(cat(out["mean"], out["value"]), cat(mm, vm))), yard):
                    failures.append((key, "mutation passes", how))
    env.close()
    assert not failures, failures


@pytest.mark.parametrize("kind,n", [("ppo", 100), ("small", 17), ("deep8", 63), ("small", 1)])
def test_caller_noise_action_and_logp(kind, n):
    """action and logp against the float64 formula evaluated on the kernel's OWN mean; yardstick: the same formula in float32 (numpy), 3 x at
    median, p99 and max.  A flipped log_std sign or a logp without the -log_std term fails the rule.  deterministic=1: action == mean bit
    for bit and logp is the formula at eps = 0."""
    import torch
    env = _env(n)
    failures = []
    for in_dim, act_dim in R.DIMS:
        p = R.random_policy(kind, in_dim, act_dim, norm=True, seed=5)
        env.set_policy(_dp(p))
        x, xd = _inputs(n, in_dim, strided=in_dim == 142)
        eps = np.random.default_rng([n, in_dim]).normal(size=(n, act_dim)).astype(np.float32)
        mean_t = torch.empty(n, act_dim, device="cuda")
        out = _np(env.act(xd, eps=torch.from_numpy(eps).cuda(), out={"mean": mean_t}))
        a64, lp64 = R.sample64(out["mean"], p.log_std, eps)
        a32, lp32 = R.sample32(out["mean"], p.log_std, eps)
        key = f"{kind}-n{n}-in{in_dim}-a{act_dim}"
        fig = {}
        for name, got, yard32, want in (("action", out["action"], a32, a64), ("logp", out["logp"], lp32, lp64)):
            g, y = R.triple(R.error_units(got, want)), R.triple(R.error_units(yard32, want))
            fig[name] = {"kernel_vs_f64": g, "numpy_f32_vs_f64": y}
            print(f"{key} {name}: kernel {g}, numpy f32 {y}")
            if not _ok(g, y):
                failures.append((key, name, g, y))
        _record("sample", key, fig)
        ya, yl = fig["action"]["numpy_f32_vs_f64"], fig["logp"]["numpy_f32_vs_f64"]
        for how in R.MUTATIONS[3:]:
            am, lpm = R.sample64_mutated(out["mean"], p.log_std, eps, how)
            if _ok(R.triple(R.error_units(out["action"], am)), ya) and _ok(R.triple(R.error_units(out["logp"], lpm)), yl):
                failures.append((key, "mutation passes", how))
        det = _np(env.act(xd, deterministic=True, out={"mean": mean_t}))
        if not (np.array_equal(_bits(det["action"]), _bits(det["mean"])) and np.array_equal(_bits(det["mean"]), _bits(out["mean"]))):
            failures.append((key, "deterministic action != mean"))
        zero = np.zeros_like(eps)
        g = R.triple(R.error_units(det["logp"], R.sample64(det["mean"], p.log_std, zero)[1]))
        y = R.triple(R.error_units(R.sample32(det["mean"], p.log_std, zero)[1], R.sample64(det["mean"], p.log_std, zero)[1]))
        if not _ok(g, y):
            failures.append((key, "deterministic logp", g, y))
    env.close()
    assert not failures, failures


def _eps_of(out, p):
    std = np.exp(p.log_std.astype(np.float64))
    return (out["action"].astype(np.float64) - out["mean"].astype(np.float64)) / std, std


def _act_with_mean(env, xd, a):
    import torch
    return _np(env.act(xd, out={"mean": torch.empty(env.n_envs, a, device="cuda")}))


def test_kernel_noise_is_the_reference_noise_and_a_function_of_device_state():
    """eps recovered as (action - mean) / std equals the reference's noise (policy_reference.noise at the handle's seed, the GLOBAL env ids and the
    task records' step and episode counters) within 4 x the error of the reference's own float32 Box-Muller against its float64 (measured here,
    over the same draws) plus 1 ulp of |mean| / std.  Rows are independent of N, a shard with ENV_OFFSET reproduces its rows, the same state
    gives the same bits, a step changes the noise, restoring state and task replays it."""
    import torch
    from mocca_envs_amd import model as M
    seed, A = R.NOISE_SEED, 21
    p = R.random_policy("ppo", 52, A, norm=True, seed=9)
    big, mid, shard = _env(100, seed=seed), _env(63, seed=seed), _env(23, seed=seed, env_offset=40)
    for e in (big, mid, shard):
        e.set_policy(_dp(p))
        e.reset()
    x = big.obs.clone()
    o100 = _act_with_mean(big, x, A)
    tk = big.get_task().cpu().numpy()
    t, ep = tk[:, M.TW.T], tk[:, M.TW.EPISODE]
    ref64, ref32 = R.noise(seed, np.arange(100), t, ep, A), R.noise(seed, np.arange(100), t, ep, A, dtype=np.float32)
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    eps, std = _eps_of(o100, p)
    tol = 4.0 * e_ref + np.spacing(np.abs(o100["mean"]).astype(np.float32)).astype(np.float64) / std
    err = np.abs(eps - ref64)
    print(f"noise: reference f32 vs f64 max {e_ref:.3e}; kernel vs reference f64 max {err.max():.3e}, worst err / tol {np.max(err / tol):.3f}")
    _record("noise", "n100", {"reference_f32_vs_f64_max": e_ref, "kernel_vs_reference_f64_max": float(err.max()), "worst_err_over_tol": float(np.max(err / tol))})
    assert np.all(err <= tol), (err.max(), e_ref)
    # the same state gives the same bits
    again = _act_with_mean(big, x, A)
    assert all(np.array_equal(_bits(again[k]), _bits(o100[k])) for k in o100)
    # N = 63: the first 63 rows; ENV_OFFSET 40, N = 23: rows 40 .. 62
    o63 = _act_with_mean(mid, x[:63].contiguous(), A)
    o23 = _act_with_mean(shard, x[40:63].contiguous(), A)
    for k in o100:
        assert np.array_equal(_bits(o63[k]), _bits(o100[k][:63])), k
        assert np.array_equal(_bits(o23[k]), _bits(o100[k][40:63])), k
    # one step later the noise differs; state and task restored, it repeats
    st, task = big.get_state().clone(), big.get_task().clone()
    big.step(torch.zeros(100, A, device="cuda"))
    later = _act_with_mean(big, x, A)
    assert np.array_equal(_bits(later["mean"]), _bits(o100["mean"])) and not np.any(later["action"] == o100["action"])
    big.set_state(st); big.set_task(task)
    back = _act_with_mean(big, x, A)
    assert all(np.array_equal(_bits(back[k]), _bits(o100[k])) for k in o100)
    for e in (big, mid, shard):
        e.close()


def test_kernel_noise_moments_at_4096_envs():
    """86 016 draws at the seed the CPU test holds the reference to: |mean| <= 4 / sqrt(n), |var - 1| <= 4 sqrt(2 / n)"""
    A = 21
    p = R.random_policy("small", 52, A, norm=False, seed=1)
    env = _env(4096, seed=R.NOISE_SEED)
    env.set_policy(_dp(p))
    env.reset()
    z, _ = _eps_of(_act_with_mean(env, env.obs, A), p)
    n = z.size
    print(f"kernel noise: n {n}, mean {z.mean():.3e}, var - 1 {z.var() - 1:.3e}")
    assert n == 86016 and abs(z.mean()) <= 4.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)
    env.close()


def _trainer_env(env_id, n, seed=3, **kw):
    from mocca_envs_amd.trainer_api import make_vec_envs
    return make_vec_envs(env_id, seed=seed, num_processes=n, record_events=False, **kw)


@pytest.mark.parametrize("env_id", ["Walker3DCustomEnv-v0", "Walker3DStepperEnv-v0"])
def test_act_step_is_act_plus_step(env_id):
    """A: act_step.  B, a twin: step(A's actions).  Observation, reward, done, info and Monitor's totals are bit-identical in each of 5 steps."""
    import torch
    n = 63
    A_, B_ = _trainer_env(env_id, n), _trainer_env(env_id, n)
    od, ad = A_.observation_space.shape[0], A_.action_space.shape[0]
    A_.attach_policy(_dp(R.random_policy("ppo", od, ad, norm=True, seed=4)))
    oa, ob = A_.reset(), B_.reset()
    assert np.array_equal(_bits(oa), _bits(ob))
    for t in range(5):
        oa, ra, _, _ = A_.act_step(oa)
        act = A_.last_act["action"].clone()
        assert float(act.abs().max()) > 0 and bool(torch.isfinite(A_.last_act["logp"]).all())
        ob, rb, _, _ = B_.step(act)
        for name, u, v in (("obs", oa, ob), ("reward", ra, rb), ("done", A_.done, B_.done), ("info", A_.venv.info, B_.venv.info),
                           ("totals", A_.episode_totals, B_.episode_totals), ("masks", A_.masks, B_.masks)):
            assert np.array_equal(_bits(u), _bits(v)), (t, name)
    A_.close(); B_.close()


def test_act_step_graph_replays_like_eager_and_sees_update_policy():
    """act_step x 3 captured in one torch.cuda.graph replays bit-identically to the eager calls of a twin; update_policy between replays changes
    the outputs without a recapture."""
    import torch
    n = 63
    p1, p2 = _dp(R.random_policy("ppo", 52, 21, norm=True, seed=6)), _dp(R.random_policy("ppo", 52, 21, norm=True, seed=7))
    E, G = _env(n, seed=8), _env(n, seed=8)
    outs = {}
    for name, e in (("E", E), ("G", G)):
        e.set_policy(p1)
        e.reset()
        outs[name] = {k: torch.zeros(3, n, 21 if k == "action" else 1, device="cuda") for k in ("action", "logp", "value")}
    run = lambda e, o: [e.act_step(e.obs, action_out=o["action"][t], logp_out=o["logp"][t], value_out=o["value"][t]) for t in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(G, outs["G"])                     # warm-up ahead of the capture, as torch requires
    torch.cuda.current_stream().wait_stream(side)
    run(E, outs["E"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(G, outs["G"])
    for second in (False, True):
        if second:
            E.update_policy(p2); G.update_policy(p2)
        before = outs["G"]["action"].clone()
        graph.replay()
        run(E, outs["E"])
        torch.cuda.synchronize()
        for k in outs["E"]:
            assert np.array_equal(_bits(outs["E"][k]), _bits(outs["G"][k])), (second, k)
        assert np.array_equal(_bits(E.obs), _bits(G.obs)) and np.array_equal(_bits(E.rew), _bits(G.rew)) and np.array_equal(_bits(E.done), _bits(G.done))
        assert not np.array_equal(_bits(before), _bits(outs["G"]["action"]))
    # the second policy really is what the replay ran: its mean for the current observation differs from the first policy's
    m1 = G.act(G.obs, deterministic=True)["action"].clone()
    G.update_policy(p1)
    assert not np.array_equal(_bits(m1), _bits(G.act(G.obs, deterministic=True)["action"]))
    E.close(); G.close()


def test_trainer_surface_fills_the_rollout_rows_and_captures():
    """act_step(into=...) writes action / logp / value / obs / reward / masks into the rollout rows; capture_rollout() with the attached
    policy equals the eager loop of a twin, bit for bit."""
    import torch
    n, T = 63, 4
    env_id = "Walker3DCustomEnv-v0"
    p = _dp(R.random_policy("ppo", 52, 21, norm=True, seed=12))

    def storage():
        z = lambda *s: torch.zeros(*s, device="cuda")
        return {"obs": z(T + 1, n, 52), "reward": z(T, n, 1), "masks": torch.ones(T + 1, n, 1, device="cuda"), "bad_masks": torch.ones(T + 1, n, 1, device="cuda"),
                "action": z(T, n, 21), "logp": z(T, n, 1), "value": z(T, n, 1)}

    def row(S):
        return lambda t: {"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1], "bad_masks": S["bad_masks"][t + 1],
                          "action": S["action"][t], "logp": S["logp"][t], "value": S["value"][t]} if t >= 0 else {"obs": S["obs"][0]}

    A_, B_ = _trainer_env(env_id, n, seed=5), _trainer_env(env_id, n, seed=5)
    SA, SB = storage(), storage()
    for e in (A_, B_):
        e.attach_policy(p)
    SA["obs"][0].copy_(A_.reset())
    B_.reset()
    graph = B_.capture_rollout(num_steps=T, into=row(SB), warmup=2)      # two eager warm-up steps advance B
    for t in range(2):                                                   # ... so A takes the same two
        A_.act_step(SA["obs"][0], into={"obs": SA["obs"][0]})
    assert np.array_equal(_bits(SA["obs"][0]), _bits(SB["obs"][0]))
    for t in range(T):
        A_.act_step(SA["obs"][t], into=row(SA)(t))
    graph.replay()
    torch.cuda.synchronize()
    for k in SA:
        assert np.array_equal(_bits(SA[k]), _bits(SB[k])), k
    assert float(SA["action"].abs().min(dim=2).values.max()) > 0 and float(SA["logp"].abs().max()) > 0 and float(SA["reward"].abs().max()) > 0
    assert np.array_equal(_bits(A_.episode_totals), _bits(B_.episode_totals))
    # the rows hold what act() gives for the stored observation (deterministic part: value)
    v = A_.venv.act(SA["obs"][1], deterministic=True)["value"]
    assert np.array_equal(_bits(v), _bits(SA["value"][1].reshape(-1)))
    A_.close(); B_.close()
    sub = _trainer_env(env_id, 64, sub_batches=2)
    with pytest.raises(NotImplementedError):
        sub.attach_policy(p)
    sub.close()


def test_bad_shapes_and_calls_are_errors_with_a_message():
    """argument checks only: nothing here launches a kernel on bad data"""
    import torch
    from mocca_envs_amd import lib as L
    env = _env(4)
    lib, h = env.lib, env.h

    def table(actor, critic, in_dim):
        rows = []
        for net, widths in enumerate((actor, critic)):
            prev = in_dim
            for w in widths:
                rows.append([net, prev, w, -(-prev // 16) * 16, -(-w // 16) * 16, 2, 0, 0])
                prev = w
        return np.array(rows, np.int32)

    def rc(tab, in_dim, act_dim, clip=10.0):
        code = lib.mocca_set_policy(h, tab.ctypes.data_as(C.c_void_p), len(tab), in_dim, act_dim, clip)
        return code, (lib.mocca_last_error(h) or b"").decode()

    x = torch.zeros(4, 52, device="cuda")
    with pytest.raises(L.MoccaError):
        env.act(x)                                                                   # no policy (Python surface)
    buf = torch.zeros(4, 21, device="cuda")
    assert lib.mocca_act(h, C.c_void_p(x.data_ptr()), 52, None, 0, C.c_void_p(buf.data_ptr()), None, None, None, None) == -1
    assert "mocca_set_policy" in lib.mocca_last_error(h).decode()                    # no policy (C ABI)
    for what, args in (("in_dim", (table([64, 21], [64, 1], 52), 36, 21)),          # the table's first layer takes 52, in_dim says 36
                       ("in_dim", (table([64, 21], [64, 1], 352), 352, 21)),         # beyond 336
                       ("multiples of 16", (table([24, 21], [64, 1], 52), 52, 21)),
                       ("1 .. 256", (table([272, 21], [64, 1], 52), 52, 21)),
                       ("8 layers", (table([16] * 8 + [21], [64, 1], 52), 52, 21)),
                       ("act_dim", (table([64, 33], [64, 1], 52), 52, 33)),
                       ("clip", (table([64, 21], [64, 1], 52), 52, 21, float("nan")))):
        code, msg = rc(*args)
        assert code == -1 and what in msg, (what, code, msg)
    assert rc(table([64, 21], [64, 1], 52), 52, 21)[0] == 0
    assert lib.mocca_act(h, C.c_void_p(x.data_ptr()), 52, None, 0, C.c_void_p(buf.data_ptr()), None, None, None, None) == -1   # shapes only: no weights yet
    assert "mocca_update_policy" in lib.mocca_last_error(h).decode()
    flat = torch.zeros(10, device="cuda")
    assert lib.mocca_update_policy(h, C.c_void_p(flat.data_ptr()), 10, None) == -1 and "floats" in lib.mocca_last_error(h).decode()
    n_base = 52 * 64 + 64 + 64 * 21 + 21 + 52 * 64 + 64 + 64 + 1 + 21
    flat = torch.zeros(n_base, device="cuda")
    assert lib.mocca_update_policy(h, C.c_void_p(flat.data_ptr()), n_base, None) == 0
    assert lib.mocca_act(h, C.c_void_p(x.data_ptr()), 51, None, 0, C.c_void_p(buf.data_ptr()), None, None, None, None) == -1   # in_stride < in_dim
    assert "in_stride" in lib.mocca_last_error(h).decode()
    assert lib.mocca_act(h, C.c_void_p(x.data_ptr()), 52, None, 1, C.c_void_p(buf.data_ptr()), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                             # zero weights: zero mean
    assert lib.mocca_set_policy(h, None, 0, 0, 0, 0.0) == 0                          # detach
    assert lib.mocca_act(h, C.c_void_p(x.data_ptr()), 52, None, 1, C.c_void_p(buf.data_ptr()), None, None, None, None) == -1
    env.close()
