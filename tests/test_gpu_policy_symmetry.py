"""The mirror-symmetric device policy on the GPU (include/mocca.h mocca_set_policy_symmetry; csrc/mocca_policy.h: Symmetry): mean and value
against the float64 definition, exact equivariance, the sample and its log-probability, the in-kernel noise, act_step as act + step, graph
capture, detaching, the argument errors and the trainer surface.  The checker is tests/policy_symmetry_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import policy_reference as R
import policy_symmetry_reference as S

pytestmark = pytest.mark.gpu
NS = (1, 7, 8, 9, 17)      # one env, one short of the 8-env tile, exactly one tile, one past it, two tiles plus one


def _env(n, env_id="Walker3DCustomEnv-v0", **kw):
    from mocca_envs_amd.vec_env import VecEnv
    return VecEnv(env_id, n, device=0, **kw)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bits(x):
    """the bytes of a tensor or array: equal bytes = equal bits"""
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def _record(name, key, value):
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: measured figures are collected there (profiles/policy_symmetry_parity.json)
    if not out:
        return
    path = os.path.join(out, "policy_symmetry_parity.json")
    doc = json.load(open(path)) if os.path.exists(path) else {
        "what": "tests/test_gpu_policy_symmetry.py: errors in units of 1e-6 (1 + |x|) as [median, p99, max] against the float64 definition, "
                "kernel and float32 yardstick", "parity": {}, "sample": {}}
    doc[name][key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _ok(got, yard):
    return all(got[i] <= 3.0 * yard[i] for i in range(3))


def _cat(m, v):
    return np.concatenate([np.asarray(m).ravel(), np.asarray(v).ravel()])


def _device_rows(x, strided):
    """device rows of x [n, in_dim]; strided: a view of wider storage (in_stride > in_dim) whose other floats are poison"""
    import torch
    if not strided:
        return torch.from_numpy(x).cuda()
    wide = torch.full((x.shape[0], x.shape[1] + 19), float("nan"), device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def _reps(n):
    """Launches per configuration, so that the rule's statistics rest on at least 64 input rows.  One row gives 11 or 22 numbers whose
    errors, in the kernel and in the float32 yardstick alike, are fractions of an ulp: the median of so few depends on which outputs
    happen to round exactly, and the ratio of two such medians has no bound.  The launches themselves keep their N."""
    return -(-64 // n)


def _act(env, xd, a, **kw):
    import torch
    return _np(env.act(xd, out={"mean": torch.empty(env.n_envs, a, device="cuda")}, **kw))


@pytest.mark.parametrize("kind,n", [(k, n) for k in ("ppo", "small") for n in NS] + [("deep8", 17)])
def test_mean_and_value_parity_with_the_f64_definition(kind, n):
    """test_gpu_policy.py's rule: error against the float64 definition in units of 1e-6 (1 + |x|); yardstick torch CPU float32 on the same
    inputs; the kernel stays within 3 x the yardstick at the median, the 99th percentile and the maximum -- for every (in_dim, A), with the
    normalisation on and off, under random tables.  Every mutation of the definition (no sign, no permutation, mirror after the
    normalisation, the sum without the 1/2) fails the same rule.  With MOCCA_TEST_OUT=<dir> the triples go to
    <dir>/policy_symmetry_parity.json.  The handle has N envs; every configuration runs _reps(N) launches on different rows."""
    env = _env(n)
    failures = []
    reps = _reps(n)
    for in_dim, act_dim in R.DIMS:
        tables = S.random_tables(in_dim, 31, act_dim=act_dim)
        for norm in (True, False):
            p = R.random_policy(kind, in_dim, act_dim, norm=norm, seed=11)
            env.set_policy(S.device_policy(p, tables))
            x = R.plausible_inputs(reps * n, in_dim, seed=n)
            outs = [_act(env, _device_rows(x[r * n:(r + 1) * n], strided=in_dim == 142), act_dim, deterministic=True) for r in range(reps)]
            out = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
            want = _cat(*S.sym_forward64(p, tables, x))
            yard = R.triple(R.error_units(_cat(*S.sym_torch32(p, tables, x)), want))
            got = R.triple(R.error_units(_cat(out["mean"], out["value"]), want))
            key = f"{kind}-n{n}-in{in_dim}-a{act_dim}-{'norm' if norm else 'raw'}"
            print(f"{key}: kernel vs f64 median/p99/max {got}, torch f32 vs f64 {yard}")
            _record("parity", key, {"kernel_vs_f64": got, "torch_f32_vs_f64": yard})
            if not _ok(got, yard):
                failures.append((key, got, yard))
            if not np.array_equal(_bits(out["action"]), _bits(out["mean"])):
                failures.append((key, "deterministic action != mean"))
            for how in S.MUTATIONS:
                if how == "mirror_after_norm" and not norm:       # without normalisation that IS the definition
                    continue
                wrong = _cat(*S.sym_forward64(p, tables, x, how))
                if _ok(R.triple(R.error_units(_cat(out["mean"], out["value"]), wrong)), yard):
                    failures.append((key, "mutation passes", how))
    env.close()
    assert not failures, failures


def _equivariance_case(which, n):
    """-> (env, symmetric DevicePolicy, its reference policy, tables)"""
    if which == "random":
        env, (in_dim, act_dim) = _env(n), (142, 21)
        p = R.random_policy("ppo", in_dim, act_dim, norm=True, seed=13)
        return env, S.device_policy(p, S.random_tables(in_dim, 32, act_dim=act_dim)), p
    env = _env(n, which)
    p = R.random_policy("ppo", env.obs_dim, 21, norm=True, seed=13)
    return env, env.symmetric_policy(S.device_policy(p)), p


@pytest.mark.parametrize("which,dims", [("Walker3DCustomEnv-v0", (52, 21)), ("Walker3DStepperEnv-v0", (65, 21)), ("random", (142, 21))])
def test_exact_equivariance(which, dims):
    """act(M_o obs, deterministic) == M_a act(obs) and the value is equal, numerically (==): the two MFMA columns of an env compute the same
    dot products in the same order wherever they sit, and the combine is commutative.  M_o obs is formed on the host (exact in f32)."""
    for n in (17, 8):
        env, dp, p = _equivariance_case(which, n)
        assert (dp.in_dim, dp.act_dim) == dims
        t = dp.symmetry
        env.set_policy(dp)
        x = R.plausible_inputs(n, dp.in_dim, seed=40 + n)
        xm = S.mirror(x, t[0], t[1])
        a, b = _act(env, _device_rows(x, False), 21, deterministic=True), _act(env, _device_rows(xm, which == "random"), 21, deterministic=True)
        assert np.all(b["mean"] == S.mirror(a["mean"], t[2], t[3])) and np.all(b["action"] == S.mirror(a["action"], t[2], t[3]))
        assert np.all(b["value"] == a["value"]) and np.all(b["logp"] == a["logp"])
        assert np.abs(S.mirror(a["mean"], t[2], t[3]) - a["mean"]).max() > 1e-3       # the mirror moves the mean: the statement is not empty
        # the env's own tables: a mirror-symmetric observation gives a mirror-symmetric action
        sym_x = np.float32(0.5) * (x + xm)
        c = _act(env, _device_rows(sym_x, False), 21, deterministic=True)
        if np.array_equal(S.mirror(sym_x, t[0], t[1]), sym_x):
            assert np.all(c["mean"] == S.mirror(c["mean"], t[2], t[3]))
        env.close()


@pytest.mark.parametrize("kind,n", [("ppo", 17), ("small", 9), ("deep8", 7), ("small", 1)])
def test_caller_noise_action_and_logp(kind, n):
    """With eps and M_a eps, action(M_o obs) == M_a action(obs) numerically.  logp sums the same terms in another order: it agrees within
    32 * 2^-23 * sum_j |term_j| (derived: at most 21 additions, each rounding a partial sum no larger than sum_j |term_j| by 2^-24 relative, on
    either side, plus the terms' own roundings -- under 32 half-ulps of that sum).  action and logp satisfy sample64 on the kernel's own
    mean with the symmetrised log_std within the sample32 yardstick rule of test_gpu_policy.py, over _reps(N) launches."""
    import torch
    env = _env(n)
    failures = []
    for in_dim, act_dim in R.DIMS:
        p, tables = R.random_policy(kind, in_dim, act_dim, norm=True, seed=5), S.random_tables(in_dim, 33, act_dim=act_dim)
        env.set_policy(S.device_policy(p, tables))
        reps = _reps(n)
        x = R.plausible_inputs(reps * n, in_dim, seed=n)
        eps = np.random.default_rng([n, in_dim]).normal(size=(reps * n, act_dim)).astype(np.float32)
        xm, em = S.mirror(x, tables[0], tables[1]), S.mirror(eps, tables[2], tables[3])
        rows = lambda v, r: v[r * n:(r + 1) * n]
        pool = lambda outs: {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
        out = pool([_act(env, _device_rows(rows(x, r), in_dim == 142), act_dim, eps=torch.from_numpy(rows(eps, r)).cuda()) for r in range(reps)])
        outm = pool([_act(env, _device_rows(rows(xm, r), False), act_dim, eps=torch.from_numpy(rows(em, r)).cuda()) for r in range(reps)])
        key = f"{kind}-n{n}-in{in_dim}-a{act_dim}"
        if not (np.all(outm["action"] == S.mirror(out["action"], tables[2], tables[3])) and np.all(outm["value"] == out["value"])):
            failures.append((key, "action(M_o obs) != M_a action(obs)"))
        ls64, ls32 = S.log_std_sym(p, tables), S.log_std_sym(p, tables, np.float32)
        terms = np.abs(-0.5 * eps.astype(np.float64) ** 2 - ls64 - R.HALF_LOG_2PI).sum(-1)
        if not np.all(np.abs(outm["logp"].astype(np.float64) - out["logp"]) <= 32 * 2.0 ** -23 * terms):
            failures.append((key, "logp(M_o obs, M_a eps) vs logp", float(np.abs(outm["logp"].astype(np.float64) - out["logp"]).max())))
        a64, lp64 = R.sample64(out["mean"], ls64, eps)
        a32, lp32 = R.sample32(out["mean"], ls32, eps)
        fig = {}
        for name, got, yard32, want in (("action", out["action"], a32, a64), ("logp", out["logp"], lp32, lp64)):
            g, y = R.triple(R.error_units(got, want)), R.triple(R.error_units(yard32, want))
            fig[name] = {"kernel_vs_f64": g, "numpy_f32_vs_f64": y}
            print(f"{key} {name}: kernel {g}, numpy f32 {y}")
            if not _ok(g, y):
                failures.append((key, name, g, y))
        _record("sample", key, fig)
        # the plain log_std (not symmetrised) is told apart
        if not np.array_equal(ls32, p.log_std):
            ya = fig["action"]["numpy_f32_vs_f64"]
            if _ok(R.triple(R.error_units(out["action"], R.sample64(out["mean"], p.log_std, eps)[0])), ya):
                failures.append((key, "the plain log_std passes"))
        det = _act(env, _device_rows(x[:n], False), act_dim, deterministic=True)
        if not (np.array_equal(_bits(det["action"]), _bits(det["mean"])) and np.array_equal(_bits(det["mean"]), _bits(out["mean"][:n]))):
            failures.append((key, "deterministic action != mean"))
    env.close()
    assert not failures, failures


def test_kernel_noise_is_the_plain_kernels_noise():
    """In default mode (action - mean) / exp(ls_sym) is the reference's noise for the handle's seed, env ids and counters within
    test_gpu_policy.py's tolerance for the plain kernel: 4 x the error of the reference's own float32 Box-Muller against its float64 plus
    1 ulp of |mean| / std.  The plain instance on the same handle state draws the same eps."""
    from mocca_envs_amd import model as M
    seed, A, n = R.NOISE_SEED, 21, 17
    p, tables = R.random_policy("ppo", 52, A, norm=True, seed=9), S.random_tables(52, 34, act_dim=A)
    env = _env(n, seed=seed)
    env.set_policy(S.device_policy(p, tables))
    env.reset()
    x = env.obs.clone()
    tk = env.get_task().cpu().numpy()
    t, ep = tk[:, M.TW.T], tk[:, M.TW.EPISODE]
    ref64, ref32 = R.noise(seed, np.arange(n), t, ep, A), R.noise(seed, np.arange(n), t, ep, A, dtype=np.float32)
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())

    def recovered(out, log_std32):
        std = np.exp(log_std32.astype(np.float64))
        eps = (out["action"].astype(np.float64) - out["mean"].astype(np.float64)) / std
        return eps, 4.0 * e_ref + np.spacing(np.abs(out["mean"]).astype(np.float32)).astype(np.float64) / std

    sym = _act(env, x, A)
    eps_s, tol_s = recovered(sym, S.log_std_sym(p, tables, np.float32))
    err = np.abs(eps_s - ref64)
    print(f"symmetric noise: reference f32 vs f64 max {e_ref:.3e}; kernel vs reference f64 max {err.max():.3e}, worst err / tol {np.max(err / tol_s):.3f}")
    assert np.all(err <= tol_s), (err.max(), e_ref)
    again = _act(env, x, A)
    assert all(np.array_equal(_bits(again[k]), _bits(sym[k])) for k in sym)
    env.set_policy_symmetry(None)                      # the plain instance, same handle state
    plain = _act(env, x, A)
    eps_p, tol_p = recovered(plain, p.log_std)
    assert np.all(np.abs(eps_p - ref64) <= tol_p) and np.all(np.abs(eps_p - eps_s) <= tol_p + tol_s)
    assert not np.array_equal(_bits(plain["mean"]), _bits(sym["mean"]))
    env.close()


def test_act_step_is_act_plus_step_and_replays_from_a_graph():
    """A: act_step with a symmetry attached.  B, a twin: act, then step on its action.  Action, logp, value, observation, reward and done are
    bit-identical.  Then ONE act_step captured in a torch.cuda.graph and replayed 3 times equals 3 eager steps of the twin."""
    import torch
    n = 17
    p = R.random_policy("ppo", 52, 21, norm=True, seed=4)
    A_, B_ = _env(n, seed=8), _env(n, seed=8)
    bufs = {}
    for name, e in (("A", A_), ("B", B_)):
        e.set_policy(e.symmetric_policy(S.device_policy(p)))
        e.reset()
        bufs[name] = {"action": torch.zeros(n, 21, device="cuda"), "logp": torch.zeros(n, device="cuda"), "value": torch.zeros(n, device="cuda")}
    a_step = lambda: A_.act_step(A_.obs, action_out=bufs["A"]["action"], logp_out=bufs["A"]["logp"], value_out=bufs["A"]["value"])

    def b_step():
        B_.act(B_.obs, out=bufs["B"])
        B_.step(bufs["B"]["action"])

    def same(tag):
        torch.cuda.synchronize()
        for k in bufs["A"]:
            assert np.array_equal(_bits(bufs["A"][k]), _bits(bufs["B"][k])), (tag, k)
        for k in ("obs", "rew", "done"):
            assert np.array_equal(_bits(getattr(A_, k)), _bits(getattr(B_, k))), (tag, k)

    for t in range(2):
        a_step(); b_step()
        same(("eager", t))
    assert float(bufs["A"]["action"].abs().max()) > 0 and float(bufs["A"]["logp"].abs().max()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a_step()                                       # warm-up ahead of the capture, as torch requires
    torch.cuda.current_stream().wait_stream(side)
    b_step()
    same("warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a_step()
    for t in range(3):
        before = bufs["A"]["action"].clone()
        graph.replay()
        b_step()
        same(("replay", t))
        assert not np.array_equal(_bits(before), _bits(bufs["A"]["action"]))
    A_.close(); B_.close()


def test_detach_gives_the_plain_policy_back():
    """after mocca_set_policy_symmetry(NULL ...) or a fresh set_policy, act is bit-identical to a handle that never had a symmetry"""
    n, A = 17, 21
    p, tables = R.random_policy("ppo", 52, A, norm=True, seed=14), S.random_tables(52, 35, act_dim=A)
    never, had = _env(n, seed=6), _env(n, seed=6)
    never.set_policy(S.device_policy(p))
    never.reset(); had.reset()
    x = never.obs.clone()
    want = _act(never, x, A)
    had.set_policy(S.device_policy(p, tables))
    sym = _act(had, x, A)
    assert not np.array_equal(_bits(sym["mean"]), _bits(want["mean"]))
    assert had.lib.mocca_set_policy_symmetry(had.h, None, None, None, None) == 0
    got = _act(had, x, A)
    assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want)
    had.set_policy(S.device_policy(p, tables))
    assert all(np.array_equal(_bits(v), _bits(sym[k])) for k, v in _act(had, x, A).items())
    had.update_policy(S.device_policy(p))              # new weights leave the symmetry alone
    assert all(np.array_equal(_bits(v), _bits(sym[k])) for k, v in _act(had, x, A).items())
    had.set_policy(S.device_policy(p))                 # a fresh set_policy drops it
    assert had.policy.symmetry is None
    got = _act(had, x, A)
    assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want)
    never.close(); had.close()


def test_bad_tables_are_errors_with_a_message_and_leave_the_state_usable():
    """argument checks only: nothing here launches a kernel on bad tables"""
    from mocca_envs_amd import lib as L
    n, A = 9, 21
    p, tables = R.random_policy("small", 52, A, norm=True, seed=15), S.random_tables(52, 36, act_dim=A)
    env = _env(n)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert env.lib.mocca_set_policy_symmetry(env.h, *[ptr(x) for x in tables]) == -1              # before set_policy
    assert "mocca_set_policy" in env.lib.mocca_last_error(env.h).decode()
    with pytest.raises(L.MoccaError):
        env.set_policy_symmetry(tables)
    env.set_policy(S.device_policy(p, tables))
    x = _device_rows(R.plausible_inputs(n, 52, seed=3), False)
    want = _act(env, x, A, deterministic=True)
    pair = next(k for k in range(52) if tables[0][k] != k)
    fixed = [k for k in range(52) if tables[0][k] == k][:3]
    act_pair = next(k for k in range(A) if tables[2][k] != k)

    def broken(which, fn):
        t = [np.array(v) for v in tables]
        fn(t[which])
        return t

    def three_cycle(perm):
        perm[fixed[0]], perm[fixed[1]], perm[fixed[2]] = fixed[1], fixed[2], fixed[0]

    cases = (("involution", broken(0, three_cycle)),
             ("swapped pair", broken(1, lambda s: s.__setitem__(pair, -s[pair]))),
             ("swapped pair", broken(3, lambda s: s.__setitem__(act_pair, -s[act_pair]))),
             ("+1 or -1", broken(1, lambda s: s.__setitem__(0, 0.5))),
             ("outside", broken(0, lambda q: q.__setitem__(0, 52))),
             ("outside", broken(2, lambda q: q.__setitem__(0, A))))
    for what, bad in cases:
        with pytest.raises(L.MoccaError, match=what.replace("+", r"\+")):
            env.set_policy_symmetry(bad)
        got = _act(env, x, A, deterministic=True)                   # the symmetry attached before is still the one that runs
        assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want), what
    assert env.lib.mocca_set_policy_symmetry(env.h, ptr(tables[0]), None, ptr(tables[2]), ptr(tables[3])) == -1
    with pytest.raises(ValueError):
        env.set_policy_symmetry(S.random_tables(36, 1, act_dim=A))  # tables of another in_dim never reach the library
    env.close()


def _trainer_env(env_id, n, seed=3, **kw):
    from mocca_envs_amd.trainer_api import make_vec_envs
    return make_vec_envs(env_id, seed=seed, num_processes=n, record_events=False, **kw)


@pytest.mark.parametrize("scan", [False, True])
def test_trainer_surface_acts_symmetrically_into_the_rollout_rows(scan):
    """TorchVecEnv.attach_policy(env.symmetric_policy(p)), then act_step into rollout rows, on Walker3DCustomEnv-v0; once more with a
    y-symmetric scan_grid attached (a wide input [obs | scan]).  The rows hold what the numpy call of the same policy gives."""
    import torch
    from mocca_envs_amd.perception import scan_grid
    n, T, env_id = 9, 3, "Walker3DCustomEnv-v0"
    kw = {}
    if scan:
        kw["height_scan"] = dict(points=scan_grid((-0.4, 1.2), (-0.5, 0.5), 5, 4), z_above=1.0, max_drop=2.0)
    env = _trainer_env(env_id, n, **kw)
    width = env.observation_space.shape[0]
    assert width == (72 if scan else 52)
    plain = S.device_policy(R.random_policy("ppo", width, 21, norm=True, seed=16))
    dp = env.symmetric_policy(plain)
    assert dp.symmetry is not None and plain.symmetry is None and dp.symmetry[0].size == width
    if scan:
        assert np.all(dp.symmetry[0][52:] >= 52) and np.any(dp.symmetry[0][52:] != np.arange(52, 72))
        with pytest.raises(ValueError):
            env.attach_policy(S.device_policy(R.random_policy("ppo", 52, 21, norm=True, seed=16), S.random_tables(52, 1, act_dim=21)))
    env.attach_policy(dp)
    z = lambda *s: torch.zeros(*s, device="cuda")
    S_ = {"obs": z(T + 1, n, width), "reward": z(T, n, 1), "masks": torch.ones(T + 1, n, 1, device="cuda"),
          "bad_masks": torch.ones(T + 1, n, 1, device="cuda"), "action": z(T, n, 21), "logp": z(T, n, 1), "value": z(T, n, 1)}
    S_["obs"][0].copy_(env.reset())
    for t in range(T):
        env.act_step(S_["obs"][t], into={"obs": S_["obs"][t + 1], "reward": S_["reward"][t], "masks": S_["masks"][t + 1],
                                         "bad_masks": S_["bad_masks"][t + 1], "action": S_["action"][t], "logp": S_["logp"][t], "value": S_["value"][t]})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(S_["action"]).all()) and float(S_["action"].abs().min(dim=2).values.max()) > 0 and float(S_["logp"].abs().max()) > 0
    assert float((S_["obs"][1:] - S_["obs"][:-1]).abs().max()) > 0
    # the value row is the symmetric value of the stored observation: the numpy call of the same policy, and invariant under the env's mirror
    obs1 = S_["obs"][1].cpu().numpy()
    v_np = dp(obs1)[2]
    v_dev = S_["value"][1].reshape(-1).cpu().numpy()
    assert np.abs(v_dev - v_np).max() <= 1e-4 * (1 + np.abs(v_np).max())
    vm = env.venv.act(torch.from_numpy(S.mirror(obs1, dp.symmetry[0], dp.symmetry[1])).cuda(), deterministic=True)["value"].cpu().numpy()
    assert np.all(vm == v_dev)
    env.close()
    cassie = _env(1, "CassieEnv-v0")                   # the reference publishes no indices for it
    with pytest.raises(NotImplementedError):
        cassie.symmetric_policy(plain)
    cassie.close()
