"""PPO with a privileged critic on the GPU (include/mocca.h mocca_set_policy_priv, mocca_set_critic_rows, mocca_ppo_grad_priv,
mocca_ppo_update_priv).  PPO's loss separates and every sum's order is a function of B and the shapes alone, so each side of the new path
is held, BIT FOR BIT, to the existing kernels on a plain policy: the actor's side to the plain policy with the same actor on the actor's
rows, the critic's side to the plain policy of in_dim = critic_in_dim with the same critic on the critic's rows.  What mixes both nets --
stats[5] -- and the whole gradient are held to float64 autograd (tests/ppo_priv_reference.py) under the project's rules; in the update's rows
stats[6], the clip coefficient formed from stats[5], is held to the update checker's (tests/ppo_update_reference.py) by bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import policy_reference as PR
import ppo_priv_reference as P
import ppo_reference as R
from ppo_grad_cases import B16, PPO_KW as KW, bits as _bits, same as _same
from policy_symmetry_reference import device_policy as _plain

pytestmark = pytest.mark.gpu
NETS = ("tiny", "ppo")            # 16-wide and 256-wide hidden layers
CASES = [(net, dims) for net in NETS for dims in P.DIMS]
NS = (1, 17, 63, 100)
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
WHAT = ("tests/test_gpu_ppo_priv.py: gradient errors per parameter tensor relative to that tensor's largest |g_f64|, pooled over a case's "
        "configurations, as [median, p99, max], kernel and float32 autograd yardstick; stats: errors of stats[0..3] in units of 1e-6 (1 + |x|); "
        "value: mocca_act's value against the float64 forward in the same units, yardstick torch CPU float32")


def _record(section, key, value):
    out = os.environ.get("MOCCA_TEST_OUT")
    if not out:
        return
    path = os.path.join(out, "ppo_grad_priv_parity.json")
    doc = json.load(open(path)) if os.path.exists(path) else {"what": WHAT, "grad": {}, "stats": {}, "value": {}}
    doc[section][key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def env_of():
    """handles of NS envs, made on first use"""
    from mocca_envs_amd.vec_env import VecEnv
    made = {}

    def get(n):
        if n not in made:
            made[n] = VecEnv("Walker3DCustomEnv-v0", n, device=0)
        return made[n]
    yield get
    for e in made.values():
        e.close()


_CASES = {}


def _case(net, dims, norm, n_rows):
    """(policy, storage, the actor side's storage, the critic side's storage), computed once and left unchanged"""
    key = (net, dims, norm, n_rows)
    if key not in _CASES:
        p = P.make_policy(net, in_dim=dims[0], critic_in_dim=dims[1], norm=norm, seed=1)
        _CASES[key] = (p,) + P.make_storage(p, n_rows, seed=2)
    return _CASES[key]


def _wide(x, extra):
    """x [n, d] on the device as a view of rows `extra` floats wider whose other floats are NaN"""
    import torch
    wide = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return wide[:, :x.shape[1]]


def _dev(st, strided=True):
    import torch
    d = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    if strided:
        for k, extra in (("obs", 13), ("critic_obs", 6)):
            if k in d:
                d[k] = _wide(st[k], extra)
    return d


def _grad(env, d, idx=None, value_clip=True, **kw):
    """env.ppo_grad on device storage `d` (critic_obs where it has it) -> (grad, stats) as numpy"""
    import torch
    extra = {"critic_obs": d["critic_obs"]} if "critic_obs" in d else {}
    out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], old_value=d["old_value"] if value_clip else None,
                       value_clip=value_clip, idx=None if idx is None else torch.from_numpy(idx).cuda(), **{**KW, **kw}, **extra)
    torch.cuda.synchronize()
    return out["grad"].cpu().numpy(), out["stats"].cpu().numpy()


def _idx(b, n_rows):
    idx = np.random.default_rng(b).permutation(n_rows)[:b].astype(np.int64)
    idx[-1] = idx[0]
    return idx


# ---- mocca_act ----

@pytest.mark.parametrize("net,dims", CASES)
def test_act_is_two_plain_policies_bit_for_bit(env_of, net, dims):
    """action, logp and mean are the bits of the plain policy with the same actor on the same rows; the value those of the plain policy of
    in_dim = critic_in_dim with the same critic on the privileged rows -- N = 1, 17, 63, 100, normalisation on and off, caller noise, both
    buffers views of wider rows whose other floats are NaN.  The value against the float64 forward: within 3 x torch CPU float32 at the
    median, the 99th percentile and the maximum, in units of 1e-6 (1 + |x|), pooled over the case."""
    import torch
    got, yard = [], []
    for n in NS:
        e = env_of(n)
        for norm in (True, False):
            p = P.make_policy(net, in_dim=dims[0], critic_in_dim=dims[1], norm=norm, seed=1)
            a = p.log_std.size
            x, xc = PR.plausible_inputs(n, dims[0], seed=n), PR.plausible_inputs(n, dims[1], seed=n + 1000)
            obs, rows = _wide(x, 19), _wide(xc, 5)
            eps = torch.from_numpy(np.random.default_rng(n).normal(0, 1, (n, a)).astype(np.float32)).cuda()
            e.set_policy(P.device_policy(p))
            with pytest.raises(Exception, match="mocca_set_critic_rows"):
                e.act(obs, eps=eps)                      # a value is asked for and no rows are bound
            e.set_critic_rows(rows)
            out = {k: v.clone() for k, v in e.act(obs, eps=eps, out={"mean": torch.empty(n, a, device="cuda")}).items()}
            e.set_policy(_plain(P.actor_side(p)))
            side_a = e.act(obs, eps=eps, out={"mean": torch.empty(n, a, device="cuda")})
            for k in ("action", "logp", "mean"):
                assert _same(out[k], side_a[k]), (n, norm, k)
            e.set_policy(_plain(P.critic_side(p)))
            side_c = e.act(rows, deterministic=True)
            assert _same(out["value"], side_c["value"]), (n, norm)
            want = P.forward64(p, x, xc)[1]
            got.append(R.stat_units(out["value"].cpu().numpy(), want))
            yard.append(R.stat_units(PR.torch32(P.critic_side(p), xc)[1], want))
    got, yard = R.triple(np.concatenate(got)), R.triple(np.concatenate(yard))
    print(f"{net} {dims} value: kernel {got}, torch f32 {yard}")
    _record("value", f"{net}:{dims[0]}-{dims[1]}", {"kernel_vs_f64": got, "torch_f32_vs_f64": yard})
    assert R.within(got, yard), (got, yard)


@pytest.mark.parametrize("dims", P.DIMS[2:])
def test_act_step_and_a_replayed_graph(dims):
    """act_step on an asymmetric policy: the policy's outputs are act's bits and the step's outputs step's bits (a twin handle steps on
    the action); the call captured in a graph replays, after an update_policy that flips the normalisation off and on, to the bits of
    the eager call on the twin"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    n = 63
    pn, pr = (P.device_policy(P.make_policy("ppo", in_dim=dims[0], critic_in_dim=dims[1], norm=norm, seed=1)) for norm in (True, False))
    x, xc = PR.plausible_inputs(n, dims[0], seed=5), PR.plausible_inputs(n, dims[1], seed=6)
    obs, rows = _wide(x, 3), _wide(xc, 7)
    E, G, T = (VecEnv("Walker3DCustomEnv-v0", n, device=0, seed=8) for _ in range(3))
    bufs = {}
    for name, e in (("E", E), ("G", G)):
        e.set_policy(pn)
        e.set_critic_rows(rows)
        e.reset()
        bufs[name] = {k: torch.zeros(n, 21 if k == "action" else 1, device="cuda") for k in ("action", "logp", "value")}
    T.reset()
    run = lambda e, o: e.act_step(obs, action_out=o["action"], logp_out=o["logp"], value_out=o["value"])
    alone = {k: v.clone() for k, v in E.act(obs).items()}          # the same noise: the step counter has not moved
    run(E, bufs["E"])
    T.step(bufs["E"]["action"])
    torch.cuda.synchronize()
    for k in ("action", "logp", "value"):
        assert _same(alone[k], bufs["E"][k]), k
    assert _same(E.obs, T.obs) and _same(E.rew, T.rew) and _same(E.done, T.done) and _same(E.info, T.info)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(G, bufs["G"])                     # warm-up ahead of the capture; G is now where E is
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(G, bufs["G"])
    seen = []
    for pol in (pn, pr, pn):
        E.update_policy(pol); G.update_policy(pol)
        graph.replay()
        run(E, bufs["E"])
        torch.cuda.synchronize()
        for k in bufs["E"]:
            assert _same(bufs["E"][k], bufs["G"][k]), k
        assert _same(E.obs, G.obs) and _same(E.rew, G.rew) and _same(E.done, G.done)
        seen.append(bufs["G"]["value"].clone())
    assert not _same(seen[0], seen[1])        # the flag word switched the critic's normalisation too
    for e in (E, G, T):
        e.close()


# ---- mocca_ppo_grad_priv ----

@pytest.mark.parametrize("net,dims", CASES)
def test_gradient_is_two_plain_gradients_bit_for_bit_and_float64_parity(env, net, dims):
    """B = 1, 16, 17, 100, 1100 (three row chunks), idx NULL and a slice of a permutation, normalisation on and off, value_clip cycling.
    By bits: the actor's tensors, log_std and stats[0, 2, 3, 4, 7] are plain mocca_ppo_grad's on the actor-side plain policy and the actor
    side's storage; the critic's tensors and stats[1] those on the critic-side plain policy over the privileged rows.  Against float64
    autograd, pooled over the case: the whole gradient within 3 x float32 autograd at the median, the 99th percentile and the maximum,
    stats[0..3] likewise; stats[5], the one statistic that mixes both nets, within 1e-5 of the f64 sum of squares of the returned
    gradient (ppo_grad_cases' rule) and of the sum of the two sides' own; stats[4] exact; stats[6] == stats[7] == 0."""
    pool_got, pool_yard, s_got, s_yard, n = [], [], [], [], 0
    for b in B16:
        for form in ("null", "perm"):
            for norm in (True, False):
                flag, n = n % 3 == 0, n + 1
                n_rows = b if form == "null" else b + 7
                p, st, st_a, st_c = _case(net, dims, norm, n_rows)
                idx = None if form == "null" else _idx(b, n_rows)
                env.set_policy(P.device_policy(p))
                grad, stats = _grad(env, _dev(st), idx, flag)
                env.set_policy(_plain(P.actor_side(p)))
                ga, sa = _grad(env, _dev(st_a), idx, flag)
                env.set_policy(_plain(P.critic_side(p)))
                gc, sc = _grad(env, _dev(st_c), idx, flag)
                key = (b, form, norm, flag)
                for (i, j), (k, l) in zip(P.actor_slices(p), P.actor_slices(P.actor_side(p))):
                    assert _same(grad[i:j], ga[k:l]), (key, "actor", i)
                for (i, j), (k, l) in zip(P.critic_slices(p), P.critic_slices(P.critic_side(p))):
                    assert _same(grad[i:j], gc[k:l]), (key, "critic", i)
                assert _same(stats[[0, 2, 3, 4, 7]], sa[[0, 2, 3, 4, 7]]) and _same(stats[1:2], sc[1:2]), (key, stats, sa, sc)
                batch = R.gather(st, idx, b)
                ref, f32 = (P.loss_autograd(p, batch, d, value_clip=flag, **KW) for d in ("float64", "float32"))
                pool_got.append(R.tensor_errors(p, grad, ref.grad)), pool_yard.append(R.tensor_errors(p, f32.grad, ref.grad))
                s_got.append(R.stat_units(stats[:4], ref.stats[:4])), s_yard.append(R.stat_units(f32.stats[:4], ref.stats[:4]))
                assert stats[4] == np.float32(round(ref.stats[4] * b)) / np.float32(b), key
                sq = float((grad.astype(np.float64) ** 2).sum())
                sides = sum(float((g[i:j].astype(np.float64) ** 2).sum()) for g, sl in ((ga, P.actor_slices(P.actor_side(p))), (gc, P.critic_slices(P.critic_side(p))))
                            for i, j in sl)
                assert abs(float(stats[5]) - sq) <= 1e-5 * sq and abs(float(stats[5]) - sides) <= 1e-5 * sides, (key, float(stats[5]), sq, sides)
                assert stats[6] == 0 and stats[7] == 0, key
    got, yard = R.triple(np.concatenate(pool_got)), R.triple(np.concatenate(pool_yard))
    sg, sy = R.triple(np.concatenate(s_got)), R.triple(np.concatenate(s_yard))
    print(f"{net} {dims}: kernel {got}, f32 autograd {yard}; stats kernel {sg}, f32 autograd {sy}")
    _record("grad", f"{net}:{dims[0]}-{dims[1]}", {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard, "elements": int(sum(map(len, pool_got)))})
    _record("stats", f"{net}:{dims[0]}-{dims[1]}", {"kernel_vs_f64": sg, "f32_autograd_vs_f64": sy})
    assert R.within(got, yard), (got, yard)
    assert R.within(sg, sy), (sg, sy)


def test_bit_stability_and_isolation(env):
    """the same bits twice; from NaN-filled outputs; with NaN beyond critic_in_dim in the privileged rows and beyond in_dim in the actor's
    (the storage here is always such views); with idx the identity; and plain ppo_grad, distill_grad and act on a plain policy give the
    same bits before and after a PPO_PRIV call that grows the shared scratch"""
    import torch
    plain = R.make_policy("tiny", norm=True, seed=1)
    pst = R.make_storage(plain, 17, seed=2)
    pd = {k: torch.from_numpy(v).cuda() for k, v in pst.items()}
    target = torch.from_numpy(np.random.default_rng(0).normal(0, 1, (17, 3)).astype(np.float32)).cuda()

    def plain_calls():
        env.set_policy(_plain(plain))
        g, s = _grad(env, pd)
        dg = env.distill_grad(pd["obs"], target, pd["returns"])
        act = env.act(pd["obs"][:4].contiguous(), deterministic=True)
        torch.cuda.synchronize()
        return [g, s, dg["grad"].cpu().numpy(), dg["stats"].cpu().numpy()] + [act[k].cpu().numpy() for k in ("action", "logp", "value")]

    before = plain_calls()
    p, st, _, _ = _case("ppo", (244, 95), True, 1100 + 7)          # by far the largest scratch this handle has seen
    env.set_policy(P.device_policy(p))
    d = _dev(st)
    first = _grad(env, d)
    again = _grad(env, d)
    grad, stats = torch.full((env.policy.n_head(),), float("nan"), device="cuda"), torch.full((8,), float("nan"), device="cuda")
    env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], old_value=d["old_value"], value_clip=True, grad=grad, stats=stats,
                 critic_obs=d["critic_obs"], **KW)
    ident = _grad(env, d, idx=np.arange(1107, dtype=np.int64))
    dense = _grad(env, _dev(st, strided=False))
    for other in (again, (grad, stats), ident, dense):
        assert _same(first[0], other[0]) and _same(first[1], other[1])
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
    after = plain_calls()
    for u, v in zip(before, after):
        assert _same(u, v)


# ---- mocca_ppo_update_priv ----

def test_update_is_the_loop_of_its_parts(env):
    """ppo_update (mocca_ppo_update_priv) over 3300 + 5 rows, minibatches of 1100 (three row chunks each), two epochs, against the Python loop
    of ppo_grad (mocca_ppo_grad_priv) + adam_step under the same permutation: the same bits in the parameters, Adam's state and every
    statistics row but [6]; [6], the second statistic that mixes both nets, is the checker's clip coefficient (ppo_update_reference) of
    that minibatch's whole gradient, by bits, and the clip binds; with the statistics tail the four arrays behind n_head are left alone"""
    import torch
    from mocca_envs_amd.rollout import AdamState
    import ppo_update_reference as U
    p, st, _, _ = _case("ppo", (65, 95), True, 3305)
    dp = P.device_policy(p)
    d = _dev(st)
    R_, B_, epochs, seed = 3305, 1100, 2, 77
    results = []
    for fused in (True, False):
        env.set_policy(dp)
        params = torch.from_numpy(dp.flat_params()).cuda()
        assert params.numel() == dp.n_head() + 2 * 65 + 2 * 95
        state = AdamState(dp.n_head(), env.device)
        if fused:
            stats = env.ppo_update(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], params, state, B_, epochs, old_value=d["old_value"],
                                   value_clip=True, seed=seed, critic_obs=d["critic_obs"], **KW, **ADAM)["stats"].clone()
        else:
            rows, coefs = [], []
            for ep in range(epochs):
                t = int(state.clock[0].item())
                perm = torch.from_numpy(U.permutation(R_, t, seed).astype(np.int64)).cuda()
                for u in range(R_ // B_):
                    out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=perm[u * B_:(u + 1) * B_].contiguous(),
                                       old_value=d["old_value"], value_clip=True, critic_obs=d["critic_obs"], **KW)
                    env.adam_step(params, out["grad"], state, **ADAM)
                    rows.append(out["stats"].clone())
                    coefs.append(U.clip_coef(out["grad"].cpu().numpy(), ADAM["max_grad_norm"]))
            stats = torch.stack(rows)
        torch.cuda.synchronize()
        results.append((params.clone(), state.moments.clone(), state.clock.clone(), stats))
    (pa, ma, ca, sa), (pb, mb, cb, sb) = results
    assert _same(pa, pb) and _same(ma, mb) and _same(ca, cb)
    assert sa.shape == (epochs * (R_ // B_), 8) and torch.isfinite(sa).all()
    assert _same(sa[:, [0, 1, 2, 3, 4, 5, 7]], sb[:, [0, 1, 2, 3, 4, 5, 7]])
    print("clip coefficients", [float(c) for c in coefs], sa[:, 6].tolist())
    assert _same(sa[:, 6], np.array(coefs, np.float32)), (sa[:, 6].tolist(), coefs)          # the loop's adam_step applies its own and reports none
    assert 0 < min(coefs) < 1          # the clip binds: a coefficient left at 1 does not pass
    assert _same(pa[dp.n_head():], dp.flat_params()[dp.n_head():]) and not _same(pa[:dp.n_head()], dp.flat_params()[:dp.n_head()])


# ---- the refusals ----

def test_every_refusal_leaves_outputs_and_handle_untouched(env):
    """every refusal the header lists for the new entry points and for the old ones on an asymmetric policy: MOCCA_E_ARG with a message
    naming the caller, the NaN-filled outputs still NaN, and the handle gives the bits it gave before"""
    import torch
    from mocca_envs_amd import lib as L
    p, st, st_a, _ = _case("tiny", (5, 9), True, 17)
    dp = P.device_policy(p)
    d, da = _dev(st, strided=False), _dev(st_a, strided=False)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    table = np.ascontiguousarray(dp.table(), np.int32)
    tp = table.ctypes.data_as(C.c_void_p)
    lib, h = env.lib, env.h
    err = lambda: (lib.mocca_last_error(h) or b"").decode()
    grad, stats = torch.full((dp.n_head(),), float("nan"), device="cuda"), torch.full((8,), float("nan"), device="cuda")
    value = torch.full((4,), float("nan"), device="cuda")
    untouched = lambda: bool(torch.isnan(grad).all() and torch.isnan(stats).all() and torch.isnan(value).all())

    def grad_priv(obs=d["obs"], stride=5, cobs=d["critic_obs"], cstride=9, action=d["action"], old_logp=d["old_logp"], adv=d["adv"], returns=d["returns"],
                  old_value=None, n=17, clip=0.2, vc=0.5, ec=0.0, value_clip=0, g=grad):
        return lib.mocca_ppo_grad_priv(h, ptr(obs), stride, ptr(cobs), cstride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value), None,
                                       n, clip, vc, ec, value_clip, ptr(g), ptr(stats), env._stream())

    env.set_policy(dp)
    rows, obs4 = d["critic_obs"][:4].contiguous(), d["obs"][:4].contiguous()
    env.set_critic_rows(rows)
    good = _grad(env, d, value_clip=False, entropy_coef=0.0)
    good_act = {k: v.clone() for k, v in env.act(obs4, deterministic=True).items()}

    def as_it_was():
        """the policy, its image and the binding of the critic's rows give the bits they gave before"""
        got, now = _grad(env, d, value_clip=False, entropy_coef=0.0), env.act(obs4, deterministic=True)
        return _same(got[0], good[0]) and _same(got[1], good[1]) and all(_same(now[k], good_act[k]) for k in good_act)

    # mocca_set_policy_priv's own: the policy in place, its weights and its binding stay
    for args, word in (((5, 0, 3, 5.0), "critic_in_dim"), ((5, 337, 3, 5.0), "critic_in_dim"), ((5, 8, 3, 5.0), "critic_in_dim = 8"),
                       ((4, 9, 3, 5.0), "in_dim = 4"), ((5, 9, 3, float("nan")), "clip"), ((5, 9, 2, 5.0), "act_dim")):
        assert lib.mocca_set_policy_priv(h, tp, table.shape[0], *args) != 0 and err().startswith("mocca_set_policy_priv:") and word in err(), (args, err())
        assert as_it_was(), args
    assert lib.mocca_set_policy_priv(None, tp, table.shape[0], 5, 9, 3, 5.0) != 0
    # mocca_set_critic_rows: the earlier binding stays
    other = torch.full((4, 9), float("nan"), device="cuda")
    assert lib.mocca_set_critic_rows(h, ptr(other), 8) != 0 and err().startswith("mocca_set_critic_rows:") and "row_stride" in err()
    assert lib.mocca_set_critic_rows(None, ptr(other), 9) != 0          # a NULL handle
    assert as_it_was()
    env.set_policy(None)                                                # no policy at all
    assert lib.mocca_set_critic_rows(h, ptr(other), 9) != 0 and "mocca_set_policy_priv" in err()
    env.set_policy(dp)                                                  # (which dropped the binding)
    # mocca_act: a value asked for and no rows bound
    act_out = torch.full((4, 3), float("nan"), device="cuda")
    act = lambda v: lib.mocca_act(h, ptr(obs4), 5, None, 1, ptr(act_out), None, ptr(v), None, env._stream())
    assert act(value) != 0 and err().startswith("mocca_act:") and "mocca_set_critic_rows" in err() and untouched() and bool(torch.isnan(act_out).all())
    assert act(None) == 0 and _same(act_out, good_act["action"])        # no value asked for: the critic is not run and no rows are needed
    env.set_critic_rows(rows)
    assert as_it_was()
    # the gradient call's own
    for kw in (dict(cobs=None), dict(cstride=8), dict(obs=None), dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(g=None),
               dict(value_clip=1), dict(n=0), dict(n=(1 << 22) + 1), dict(stride=4), dict(clip=float("nan")), dict(vc=-1.0), dict(ec=float("inf"))):
        assert grad_priv(**kw) != 0 and err().startswith("mocca_ppo_grad_priv:") and untouched(), (kw, err())
    # the old entry points on an asymmetric policy name the call to use
    old_args = (ptr(d["obs"]), 5, ptr(d["action"]), ptr(d["old_logp"]), ptr(d["adv"]), ptr(d["returns"]), None, None, 17, 0.2, 0.5, 0.0, 0, ptr(grad), ptr(stats),
                env._stream())
    for name in ("mocca_ppo_grad", "mocca_ppo_grad_sym", "mocca_ppo_grad_mirror", "mocca_ppo_grad_dup"):
        assert getattr(lib, name)(h, *old_args) != 0 and err().startswith(name + ":") and "mocca_ppo_grad_priv" in err() and untouched(), (name, err())
    assert lib.mocca_distill_grad(h, ptr(d["obs"]), 5, ptr(d["action"]), None, None, 17, 1.0, 0.5, ptr(grad), ptr(stats), env._stream()) != 0 \
        and "privileged critic" in err() and untouched()
    from mocca_envs_amd.rollout import AdamState
    params, state = torch.from_numpy(dp.flat_params()).cuda(), AdamState(dp.n_head(), env.device)
    keep = params.clone()
    upd_tail = (17, 8, 1, 0.2, 0.5, 0.0, 0, ptr(params), params.numel(), dp.n_head(), ptr(state.moments), ptr(state.clock), 3e-4, 0.9, 0.999, 1e-5, 0.5, 1,
                None, env._stream())
    assert lib.mocca_ppo_update(h, *old_args[:7], *upd_tail) != 0 and "mocca_ppo_update_priv" in err() and _same(params, keep)
    assert lib.mocca_distill_update(h, ptr(d["obs"]), 5, ptr(d["action"]), None, 17, 8, 1, 1.0, 0.5, *upd_tail[7:]) != 0 and "privileged critic" in err()
    assert lib.mocca_ppo_update_priv(h, ptr(d["obs"]), 5, None, 9, *old_args[2:7], *upd_tail) != 0 and err().startswith("mocca_ppo_update_priv:")
    assert lib.mocca_ppo_update_priv(h, ptr(d["obs"]), 5, ptr(d["critic_obs"]), 8, *old_args[2:7], *upd_tail) != 0 and "critic_stride" in err()
    # mocca_ppo_update_priv inherits every refusal of mocca_ppo_update (test_gpu_ppo_update.py's list): parameters, moments and clock stay
    n_floats, n_head, rows_out = params.numel(), dp.n_head(), torch.full((2, 8), float("nan"), device="cuda")
    held = [params.clone(), state.moments.clone(), state.clock.clone()]

    def update_priv(hh=h, obs=d["obs"], stride=5, cobs=d["critic_obs"], cstride=9, action=d["action"], old_logp=d["old_logp"], adv=d["adv"],
                    returns=d["returns"], old_value=None, n=17, batch=8, epochs=1, clip=0.2, vc=0.5, ec=0.0, value_clip=0, pr=params, nf=n_floats,
                    nh=n_head, m=state.moments, c=state.clock, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, mx=0.5):
        return lib.mocca_ppo_update_priv(hh, ptr(obs), stride, ptr(cobs), cstride, ptr(action), ptr(old_logp), ptr(adv), ptr(returns), ptr(old_value), n, batch,
                                         epochs, clip, vc, ec, value_clip, ptr(pr), nf, nh, ptr(m), ptr(c), lr, b1, b2, eps, mx, 3, ptr(rows_out), env._stream())

    nan, inf = float("nan"), float("inf")
    for kw in (dict(pr=None), dict(m=None), dict(c=None), dict(nf=n_head + 1), dict(nf=n_floats - 1), dict(nf=n_head + 10), dict(nh=0), dict(nh=n_head + 1),
               dict(nh=-3), dict(lr=nan), dict(lr=inf), dict(lr=-1e-3), dict(eps=nan), dict(eps=inf), dict(eps=-1e-5), dict(b1=1.0), dict(b1=-0.1),
               dict(b1=nan), dict(b2=1.0), dict(b2=-0.1), dict(b2=nan), dict(mx=nan), dict(mx=-0.5),
               dict(batch=0), dict(batch=18), dict(batch=-1), dict(epochs=0), dict(epochs=-2), dict(n=0), dict(n=(1 << 22) + 1), dict(obs=None),
               dict(action=None), dict(old_logp=None), dict(adv=None), dict(returns=None), dict(value_clip=1), dict(stride=4), dict(clip=nan),
               dict(clip=-0.1), dict(vc=inf), dict(vc=-1.0), dict(ec=nan), dict(ec=-0.5), dict(cobs=None), dict(cstride=8)):
        assert update_priv(**kw) != 0 and err().startswith("mocca_ppo_update_priv:"), (kw, err())
    assert update_priv(hh=None) != 0 and lib.mocca_last_error(None)
    torch.cuda.synchronize()
    assert _same(params, held[0]) and _same(state.moments, held[1]) and _same(state.clock, held[2]) and bool(torch.isnan(rows_out).all())
    short = params[:-1].contiguous()
    assert lib.mocca_update_policy(h, ptr(short), short.numel(), env._stream()) != 0 and "critic_mean" in err()
    half = params[:dp.n_head() + 10].contiguous()           # mean and inv_std alone: all four or none
    assert lib.mocca_update_policy(h, ptr(half), half.numel(), env._stream()) != 0
    assert _same(params, keep) and float(state.clock[0].item()) == 0.0
    # the mirror attachments and the privileged critic refuse each other, in both orders
    tables = (np.arange(5, dtype=np.int32), np.ones(5, np.float32), np.arange(3, dtype=np.int32), np.ones(3, np.float32))
    for setter, extra in ((env.set_policy_symmetry, ()), (env.set_policy_mirror_loss, (0.5,)), (env.set_policy_mirror_dup, ())):
        with pytest.raises(L.MoccaError, match="privileged critic"):
            setter(tables, *extra)
    assert _same(_grad(env, d, value_clip=False, entropy_coef=0.0)[0], good[0])          # the handle is as it was
    plain = _plain(P.actor_side(p))
    for setter, extra, word in ((env.set_policy_symmetry, (), "mocca_set_policy_symmetry"), (env.set_policy_mirror_loss, (0.5,), "mocca_set_policy_mirror_loss"),
                                (env.set_policy_mirror_dup, (), "mocca_set_policy_mirror_dup")):
        env.set_policy(plain)
        setter(tables, *extra)
        assert lib.mocca_set_policy_priv(h, tp, table.shape[0], 5, 9, 3, 5.0) != 0 and word in err()
        assert lib.mocca_set_critic_rows(h, ptr(rows), 9) != 0 and "mocca_set_policy_priv" in err()      # a binding on a plain policy
        setter(None, *extra)
    # a plain policy: the new calls refuse and name the plain ones; mocca_set_policy has returned the handle to a plain policy
    env.set_policy(plain)
    assert grad_priv() != 0 and "mocca_ppo_grad" in err() and untouched()
    pp, ps = torch.from_numpy(plain.flat_params()).cuda(), AdamState(plain.n_head(), env.device)
    assert update_priv(pr=pp, nf=pp.numel(), nh=plain.n_head(), m=ps.moments, c=ps.clock) != 0 and err().startswith("mocca_ppo_update_priv:") \
        and "mocca_ppo_update" in err().split(":", 1)[1]
    torch.cuda.synchronize()
    assert _same(pp, plain.flat_params()) and not ps.moments.any() and float(ps.clock[0].item()) == 0.0 and bool(torch.isnan(rows_out).all())
    ga = _grad(env, da, value_clip=False, entropy_coef=0.0)
    env.set_policy(dp)
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"])                       # critic_obs missing
    with pytest.raises(ValueError):
        env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], critic_obs=d["critic_obs"][:9])
    with pytest.raises(L.MoccaError):
        env.distill_grad(d["obs"], d["action"])
    with pytest.raises(ValueError):
        env.set_teacher(dp)
    env.set_policy(plain)
    with pytest.raises(ValueError):
        env.ppo_grad(da["obs"], da["action"], da["old_logp"], da["adv"], da["returns"], critic_obs=d["critic_obs"])
    assert _same(_grad(env, da, value_clip=False, entropy_coef=0.0)[0], ga[0])
    env.set_policy(dp)
    assert _same(_grad(env, d, value_clip=False, entropy_coef=0.0)[0], good[0])


@pytest.mark.parametrize("entry", ["mocca_act_step", "mocca_act_plan_step"])
def test_a_step_refuses_a_value_without_bound_rows(entry):
    """mocca_act_step and mocca_act_plan_step with value_dev asked for on an asymmetric policy and no rows bound: MOCCA_E_ARG naming the
    caller and mocca_set_critic_rows, nothing launched -- every output keeps its NaN -- and the handle then steps to the bits of a twin that
    saw no refused call"""
    import torch
    from types import SimpleNamespace
    from mocca_envs_amd.vec_env import VecEnv
    n, plan = 16, entry == "mocca_act_plan_step"
    kw, a = {}, 21
    if plan:
        rng, a = np.random.default_rng(3), 15
        kw = dict(base_controller=SimpleNamespace(actor=P._net(rng, 65, [48], ["tanh"], 21), critic=P._net(rng, 65, [16], ["softsign"], 1)))
    A, B = (VecEnv("Walker3DPlannerEnv-v0" if plan else "Walker3DCustomEnv-v0", n, device=0, seed=5, **kw) for _ in range(2))
    d = A.obs_dim
    dp = P.device_policy(P.make_policy("tiny", in_dim=d, critic_in_dim=d + 6, norm=True, seed=4, act_dim=a))
    rows = torch.from_numpy(PR.plausible_inputs(n, d + 6, seed=9)).cuda()
    for e in (A, B):
        e.set_policy(dp)
        e.reset()
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    buf = dict(action=f(n, a), logp=f(n), value=f(n), mean=f(n, a), obs=f(n, d), rew=f(n))
    done, info = torch.full((n,), 7, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = getattr(A.lib, entry)(A.h, ptr(A.obs), int(A.obs.stride(0)), None, 0, ptr(buf["action"]), ptr(buf["logp"]), ptr(buf["value"]), ptr(buf["mean"]), ptr(buf["obs"]),
                               ptr(buf["rew"]), ptr(done), ptr(info), A._stream())
    msg = (A.lib.mocca_last_error(A.h) or b"").decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith(entry + ":") and "mocca_set_critic_rows" in msg, (rc, msg)
    assert all(bool(torch.isnan(v).all()) for v in buf.values()) and int(done.min()) == 7 and int(info.min()) == 7
    step = (lambda e, **o: e.act_plan_step(e.obs, **o)) if plan else (lambda e, **o: e.act_step(e.obs, **o))
    for e in (A, B):
        e.set_critic_rows(rows)
    va, vb = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for t in range(2):
        (oa, ra, _, _), (ob, rb, _, _) = step(A, value_out=va), step(B, value_out=vb)
        torch.cuda.synchronize()
        assert _same(oa, ob) and _same(ra, rb) and _same(va, vb) and _same(A.last_action, B.last_action) and _same(A.get_state(), B.get_state()), t
    A.close(), B.close()


# ---- the trainer surface ----

def test_trainer_binds_the_privileged_row(tmp_path):
    """make_vec_envs(depth_camera=, privileged_scan=) with an asymmetric policy: attach_policy binds envs.privileged, act_step's value is
    DevicePolicy.__call__ on (obs, envs.privileged) within the policy test's rule, the step's outputs are step()'s bits on a twin, and
    act_step -> depth camera -> privileged scan is capturable as one graph that replays to the eager chain's bits"""
    import torch
    from mocca_envs_amd.perception import DepthCamera, scan_grid
    from mocca_envs_amd.trainer_api import make_vec_envs
    cam = DepthCamera(offset=(0.15, 0.0, 0.10), pitch=-35.0, fov_y=90.0, near=0.05, far=6.0, width=4, height=3)
    scan = dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), 3, 2), z_above=1.0, max_drop=2.0)
    n, T = 64, 4
    make = lambda **kw: make_vec_envs("Walker3DStepperEnv-v0", 5, n, None, depth_camera=cam, **kw)
    A_, G_, twin = make(privileged_scan=scan), make(privileged_scan=scan), make()
    d = A_.venv.obs_dim
    p = P.make_policy("ppo", in_dim=d + 12, critic_in_dim=d + 6, norm=True, seed=3)
    dp = P.device_policy(p)
    with pytest.raises(ValueError):
        twin.attach_policy(dp)                            # no privileged row to bind
    with pytest.raises(NotImplementedError):
        make_vec_envs("Walker3DStepperEnv-v0", 5, n, None, privileged_scan=scan, sub_batches=2)
    for e in (A_, G_):
        e.attach_policy(dp)
        assert e.venv.critic_rows is e.privileged
    oa, ot = A_.reset(), twin.reset()
    G_.reset()
    got, yard = [], []
    for t in range(T):
        rows, priv = oa.clone(), A_.privileged.clone()
        oa, ra, _, _ = A_.act_step(oa)
        value, action = A_.last_act["value"].clone(), A_.last_act["action"].clone()
        ot, rt, _, _ = twin.step(action)
        torch.cuda.synchronize()
        assert _same(oa, ot) and _same(ra, rt) and _same(A_.done, twin.done) and _same(A_.venv.info, twin.venv.info), t
        _, _, v32, _ = dp(rows.cpu().numpy(), critic_obs=priv.cpu().numpy())
        want = P.forward64(p, rows.cpu().numpy(), priv.cpu().numpy())[1]
        got.append(R.stat_units(value[:, 0].cpu().numpy(), want)), yard.append(R.stat_units(PR.torch32(P.critic_side(p), priv.cpu().numpy())[1], want))
        assert np.abs(v32 - want).max() < 1e-4
    got, yard = R.triple(np.concatenate(got)), R.triple(np.concatenate(yard))
    print(f"trainer value: kernel {got}, torch f32 {yard}")
    assert R.within(got, yard), (got, yard)
    vals, acts, obs_rows = (torch.zeros(T, n, k, device="cuda") for k in (1, 21, d + 12))

    def sink(t, ob, rw, m, bm, a):
        vals[t].copy_(G_.last_act["value"]), acts[t].copy_(a), obs_rows[t].copy_(ob)

    G_.act_step()         # one eager step on both: whatever a first call sets up is not inside the capture
    torch.cuda.synchronize()
    graph = G_.capture_rollout(None, T, sink=sink, warmup=0)
    graph.replay()
    torch.cuda.synchronize()
    E_ = make(privileged_scan=scan)
    E_.attach_policy(dp)
    E_.reset()
    o = E_.act_step()[0]
    for t in range(T):
        o = E_.act_step(o)[0]
        torch.cuda.synchronize()
        assert _same(vals[t], E_.last_act["value"]) and _same(acts[t], E_.last_act["action"]) and _same(obs_rows[t], o), t
    assert _same(E_.privileged, G_.privileged)
    for e in (A_, G_, twin, E_):
        e.close()


VERIFY_BOUND = 1e-2            # test_gpu_ppo_symmetry.py's bound on every verify_grad line: a wiring error leaves a difference of order 1


def test_ppo_demo_trains_with_a_privileged_critic(tmp_path, capsys):
    """tools/ppo_demo.py --privileged-critic, imported and driven, 64 envs x 8 steps, two iterations per arm: the device update, the
    device gradient with torch's Adam, the torch update behind device collection, and the torch loop alone.  Every arm runs and writes a
    policy file that holds the critic's statistics and loads as an asymmetric DevicePolicy; every --verify-grad line -- the kernel's
    gradient against autograd with vf on the privileged rows, scaled per tensor -- stays below VERIFY_BOUND."""
    import importlib.util
    from mocca_envs_amd.policy import DevicePolicy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ppo_demo", os.path.join(root, "tools", "ppo_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    common = ["--env-id", "Walker3DStepperEnv-v0", "--envs", "64", "--steps", "8", "--iters", "2", "--depth-camera", "4,3", "--privileged-scan", "3,2",
              "--privileged-critic"]
    arms = {"update": ["--device-policy", "--device-returns", "--device-grad", "--device-update", "--verify-grad"],
            "grad": ["--device-policy", "--device-returns", "--device-grad", "--verify-grad"],
            "torch-update": ["--device-policy", "--device-returns"], "torch": []}
    for tag, flags in arms.items():
        out = str(tmp_path / tag)
        demo.main(common + flags + ["--out", out])
        lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
        verify = [x["verify_grad"] for x in lines if "verify_grad" in x]
        print(tag, "verify_grad", verify)
        assert len(verify) == (2 if "--verify-grad" in flags else 0) and all(v < VERIFY_BOUND for v in verify), (tag, verify)
        assert all(np.isfinite(x["mean_return"]) for x in lines if "mean_return" in x)
        dp = DevicePolicy.from_npz(out + "_policy.npz")
        assert dp.asymmetric and dp.critic_in_dim == dp.in_dim - 12 + 6
    with pytest.raises(SystemExit):
        demo.main(common[:-3] + ["--privileged-critic", "--out", str(tmp_path / "x")])        # no --privileged-scan
