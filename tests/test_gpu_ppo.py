"""mocca_ppo_grad on the GPU (include/mocca.h): the gradient and the statistics against float64 autograd with float32 autograd as the
yardstick, and the call's contract -- fixed bits, overwritten outputs, graph capture, a read-only image, the argument errors.  The checker
is tests/ppo_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ppo_reference as R

pytestmark = pytest.mark.gpu
BATCHES = (1, 16, 17, 100, 1100)     # one row, the 16-row tile, one past it, several workgroups, three row chunks of launch 2 (512 rows at least each)
KW = dict(clip=R.CLIP, value_coef=0.5, entropy_coef=0.01)


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.close()


def _dp(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def _record(section, key, value):
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: measured figures are collected there (profiles/ppo_grad_parity.json)
    if not out:
        return
    path = os.path.join(out, "ppo_grad_parity.json")
    doc = json.load(open(path)) if os.path.exists(path) else {
        "what": "tests/test_gpu_ppo.py: gradient errors per parameter tensor relative to that tensor's largest |g_f64|, pooled, as [median, "
                "p99, max], kernel and float32 autograd yardstick; stats: errors of stats[0..3] in units of 1e-6 (1 + |x|)", "grad": {}, "stats": {},
        "adam": {}}
    doc[section][key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


_STORAGE = {}


def _storage(name, norm, n_rows):
    key = (name, norm, n_rows)
    if key not in _STORAGE:
        p = R.make_policy(name, norm=norm, seed=1)
        _STORAGE[key] = (p, R.make_storage(p, n_rows, seed=2))
    return _STORAGE[key]


def _device(st, strided):
    """the storage on the device; strided: obs is a view of wider rows whose other floats are NaN"""
    import torch
    d = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    if strided:
        wide = torch.full((st["obs"].shape[0], st["obs"].shape[1] + 13), float("nan"), device="cuda")
        wide[:, :st["obs"].shape[1]] = d["obs"]
        d["obs"] = wide[:, :st["obs"].shape[1]]
    return d


def _call(env, d, idx=None, value_clip=False, **kw):
    import torch
    out = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=None if idx is None else torch.from_numpy(idx).cuda(),
                       old_value=d["old_value"] if value_clip else None, value_clip=value_clip, **{**KW, **kw})
    torch.cuda.synchronize()
    return out["grad"].cpu().numpy(), out["stats"].cpu().numpy()


def _configs():
    """(B, idx form, norm, value_clip, strided): every batch size with both index forms and the normalisation on and off; value_clip and
    the strided obs cycle with periods 3 and 5, so that over the 20 configurations each meets both index forms and both normalisations"""
    n = 0
    for b in BATCHES:
        for form in ("null", "perm"):
            for norm in (True, False):
                yield b, form, norm, n % 3 == 0, n % 5 < 2
                n += 1


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_gradient_and_stats_parity(env, name):
    """The project's rule.  Per parameter tensor the error against the float64 gradient over that tensor's largest |g_f64|, pooled over the
    tensors of a configuration (configurations of fewer than 1000 elements are pooled with the next ones of the net: few samples give no
    stable ratio); the kernel stays within 3 x float32 autograd at the median, the 99th percentile and the maximum.  stats[0..3] by the same
    rule in units of 1e-6 (1 + |x|), pooled over the net's configurations; stats[4] exact; stats[5] within 1e-5 of the f64 sum over grad_dev.
    No row is left out: the storage avoids the loss's discrete ties by construction (ppo_reference.make_storage)."""
    failures, pool_got, pool_yard, pool_keys, s_got, s_yard = [], [], [], [], [], []

    def flush():
        got, yard = R.triple(np.concatenate(pool_got)), R.triple(np.concatenate(pool_yard))
        key = "+".join(pool_keys)
        print(f"{name} {key}: kernel {got}, f32 autograd {yard}")
        _record("grad", f"{name}:{key}", {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard, "elements": int(sum(map(len, pool_got)))})
        if not R.within(got, yard):
            failures.append((key, got, yard))
        pool_got.clear(), pool_yard.clear(), pool_keys.clear()

    configs = list(_configs())
    for i, (b, form, norm, value_clip, strided) in enumerate(configs):
        n_rows = b if form == "null" else b + 7
        p, st = _storage(name, norm, n_rows)
        env.set_policy(_dp(p))
        idx = None
        if form == "perm":      # a slice of a permutation, with one row repeated
            idx = np.random.default_rng(b).permutation(n_rows)[:b].astype(np.int64)
            idx[-1] = idx[0]
        grad, stats = _call(env, _device(st, strided), idx=idx, value_clip=value_clip)
        batch = R.gather(st, idx, b)
        ref = R.loss_autograd(p, batch, "float64", value_clip=value_clip, **KW)
        f32 = R.loss_autograd(p, batch, "float32", value_clip=value_clip, **KW)
        pool_got.append(R.tensor_errors(p, grad, ref.grad)), pool_yard.append(R.tensor_errors(p, f32.grad, ref.grad))
        pool_keys.append(f"B{b}-{form}-{'norm' if norm else 'raw'}{'-vclip' if value_clip else ''}")
        s_got.append(R.stat_units(stats[:4], ref.stats[:4])), s_yard.append(R.stat_units(f32.stats[:4], ref.stats[:4]))
        if stats[4] != np.float32(round(ref.stats[4] * b)) / np.float32(b):
            failures.append((pool_keys[-1], "clip fraction", float(stats[4]), ref.stats[4]))
        sq = float((grad.astype(np.float64) ** 2).sum())
        if abs(float(stats[5]) - sq) > 1e-5 * sq or stats[6] != 0 or stats[7] != 0:
            failures.append((pool_keys[-1], "sum of grad^2", float(stats[5]), sq))
        rest = sum(ref.grad.size for _ in configs[i + 1:])
        if sum(map(len, pool_got)) >= 1000 and (rest >= 1000 or rest == 0):
            flush()
    if pool_got:
        flush()
    got, yard = R.triple(np.concatenate(s_got)), R.triple(np.concatenate(s_yard))
    print(f"{name} stats: kernel {got}, f32 autograd {yard}")
    _record("stats", name, {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard})
    if not R.within(got, yard):
        failures.append(("stats", got, yard))
    assert not failures, failures


def test_same_bits_whatever_the_outputs_held_and_identity_idx(env):
    """two calls on the same inputs give the same bits; grad / stats pre-filled with NaN are fully overwritten; idx = identity is idx NULL"""
    import torch
    p, st = _storage("mixed", True, 100)
    env.set_policy(_dp(p))
    d = _device(st, False)
    first = _call(env, d, value_clip=True)
    grad, stats = torch.full((env.policy.n_head(),), float("nan"), device="cuda"), torch.full((8,), float("nan"), device="cuda")
    env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], old_value=d["old_value"], value_clip=True, grad=grad, stats=stats, **KW)
    ident = _call(env, d, idx=np.arange(100, dtype=np.int64), value_clip=True)
    for other in ((grad, stats), ident):
        assert np.array_equal(_bits(first[0]), _bits(other[0])) and np.array_equal(_bits(first[1]), _bits(other[1]))
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()


def test_zero_advantages_and_no_value_coef_give_zero_gradient(env):
    """actor and critic gradient exactly 0, log_std's exactly -entropy_coef"""
    p, st = _storage("ppo", True, 100)
    env.set_policy(_dp(p))
    st = dict(st, adv=np.zeros_like(st["adv"]))
    grad, _ = _call(env, _device(st, False), value_coef=0.0, entropy_coef=0.01)
    a = p.log_std.size
    assert np.all(grad[:-a] == 0) and np.all(grad[-a:] == -np.float32(0.01))


def test_graph_replay_sees_an_update_and_act_is_untouched(env):
    """a graph captured after a warm call replays to the eager bits, before and after an update_policy made between the replays; mocca_act's
    outputs after ppo_grad calls equal those before: the image is only read"""
    import torch
    p, st = _storage("ppo", True, 100)
    q = R.make_policy("ppo", norm=True, seed=9)
    env.set_policy(_dp(p))
    d = _device(st, False)
    obs4 = d["obs"][:4].contiguous()
    before = env.act(obs4, deterministic=True)
    before = {k: v.clone() for k, v in before.items()}
    grad, stats = torch.empty(env.policy.n_head(), device="cuda"), torch.empty(8, device="cuda")
    call = lambda g, s: env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], grad=g, stats=s, **KW)
    call(grad, stats)      # warm: the scratch is allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(grad, stats)
    for pol in (p, q):
        env.update_policy(_dp(pol))
        grad.fill_(float("nan"))
        graph.replay()
        eager_g, eager_s = torch.empty_like(grad), torch.empty_like(stats)
        call(eager_g, eager_s)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(grad), _bits(eager_g)) and np.array_equal(_bits(stats), _bits(eager_s))
        if pol is p:
            after = env.act(obs4, deterministic=True)
            assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in before)
            first = grad.clone()
    assert not np.array_equal(_bits(first), _bits(grad))


def test_one_adam_step_matches_autograd(env):
    """one torch.optim.Adam step from ppo_grad's gradient and one from float64 autograd's, on the 52 -> 256 -> 256 -> 21 policy: the
    parameters' difference, per tensor over that tensor's largest |step_f64|, stays within 3 x the difference a float32-autograd step leaves"""
    import torch
    p, st = _storage("ppo", True, 100)
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
    p, st = _storage("tiny", True, 17)
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
    p, st = _storage("ppo", True, 96)
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
