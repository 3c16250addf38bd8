"""One harness for the five instances of the PPO gradient kernel (ppo_rows_kernel<PPO_PLAIN> and so on; include/mocca.h): the table of
what differs between them (MODES), the acceptance loop that holds each to its float64 reference (parity), and the two contract tests whose
bodies are the same for all five.  tests/test_gpu_ppo.py, _symmetry, _mirror, _dup and test_gpu_distill.py drive it on the GPU;
tests/test_ppo_grad_cases.py drives parity on the CPU with gradients that are right and gradients that are wrong.

The project's rule, which parity applies.  Per parameter tensor the error against the float64 gradient over that tensor's largest |g_f64|,
pooled over the tensors of a configuration (configurations of fewer than 1000 elements are pooled with the next ones of the net: few
samples give no stable ratio); the kernel stays within 3 x float32 autograd at the median, the 99th percentile and the maximum.  The
statistics a mode picks (Mode.pick) by the same rule in units of 1e-6 (1 + |x|), pooled over the net's configurations; stats[4] exact: the
reference's count over the samples (B, or 2 B with the twins), divided in float32; stats[5] within 1e-5 of the f64 sum of squares of the
returned gradient; stats[6] == 0, and stats[7] == 0 where the mode puts nothing there.  No row is left out: every storage avoids the
loss's discrete ties by construction (ppo_reference.make_storage and its siblings)."""
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np

import distill_reference as D
import ppo_dup_reference as PD
import ppo_mirror_reference as PM
import ppo_reference as R
import ppo_symmetry_reference as PS
from policy_symmetry_reference import device_policy  # noqa: F401  (device_policy(p, tables=None); re-exported for the tests)

PPO_KW = dict(clip=R.CLIP, value_coef=0.5, entropy_coef=0.01)
DISTILL_KW = dict(distill_coef=0.7, value_coef=0.5)
B16 = (1, 16, 17, 100, 1100)        # one row, the 16-row tile, one past it, several workgroups, three row chunks of launch 2 (512 rows at least each)
B8 = (1, 8, 9, 17, 100, 1100)       # one row, the 8-row tile, one past it, across the 16-row scratch tile, several workgroups, several row chunks of launch 2
STAT7 = {"zero": lambda x: x == 0, "positive": lambda x: x > 0, "nonzero": lambda x: x != 0}      # what a good call leaves in stats[7]
GRAD_WHAT = "gradient errors per parameter tensor relative to that tensor's largest |g_f64|, pooled, as [median, p99, max], kernel and float32 autograd yardstick; "


def _swapped_and_negated_tables(name):
    """the first seed whose tables swap a pair and negate an entry on both sides"""
    for seed in range(3, 67):
        tables = PD.random_tables(R.NETS[name][0], seed, R.NETS[name][1])
        if all((np.asarray(perm) != np.arange(len(perm))).any() and (np.asarray(sign) < 0).any() for perm, sign in (tables[:2], tables[2:])):
            return tables
    raise AssertionError("no tables with a swapped pair and a negative sign on both sides")


def _ppo_run(env, d, flag, **kw):
    return env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], old_value=d["old_value"] if flag else None, value_clip=flag, **kw)


def _distill_checks(p, grad, stats, ref, flag):
    """A tensor whose f64 gradient is identically zero -- log_std's always, the critic's without value targets -- is not pooled
    (distill_reference.pooled_errors): it must be all +0.0f bits.  stats[0, 3, 4, 6] are +0.0f bits."""
    out = []
    if not D.zero_bits_ok(p, grad, ref.grad):
        out.append(("a tensor with an identically zero gradient is not all +0.0f bits",))
    if len(D.zero_tensors(p, ref.grad)) != (1 if flag else 1 + 2 * len(p.critic)):
        out.append(("the reference's zero tensors",))
    if stats[[0, 3, 4, 6]].view(np.uint32).any():
        out.append(("stats[0, 3, 4, 6]", stats.tolist()))
    return out


def _mode(name, file, what, sections, loss, **kw):
    """the plain PPO call's record with `kw` laid over it.  Fields:
    loss(p, tables, coef, batch, dtype, flag) the reference; make_policy, tables(net name), make_storage(net name, p, tables, n_rows);
    in_policy: the tables go into the DevicePolicy; setter(env, tables, coef): the attachment made after set_policy, or None -- a mode with
    one only reads the plain policy, and its graph test checks that act() stays the plain policy's; coefs: the setter's weights, cycled;
    run(env, d, flag, **kw) the env call and kw its keywords; flag(n) the fourth configuration flag with its key suffixes (off, on), and
    the flag the contract tests use (same bits, graph); pick(stats) the stats that go by ratio; errors the pooled gradient errors;
    samples: stats[4]'s denominator over B; stat7: a key of STAT7; checks(p, grad, stats, ref, flag): further per-configuration failures"""
    plain = dict(make_policy=R.make_policy, tables=lambda net: None, make_storage=lambda net, p, tables, n: R.make_storage(p, n, seed=2),
                 in_policy=False, setter=None, coefs=(None,), run=_ppo_run, kw=PPO_KW, batches=B16, flag=lambda n: n % 3 == 0, suffix=("", "-vclip"),
                 contract_flags=(True, False), pick=lambda s: s[:4], errors=R.tensor_errors, samples=1, stat7="zero", checks=None)
    return SimpleNamespace(name=name, file=file, what=what, sections=sections, loss=loss, **{**plain, **kw})


_random_tables = lambda net: PS.random_tables(R.NETS[net][0], 3, R.NETS[net][1])
_with_stat7 = lambda s: np.r_[s[:4], s[7]]
MODES = {m.name: m for m in (
    _mode("plain", "ppo_grad_parity.json", "tests/test_gpu_ppo.py: " + GRAD_WHAT + "stats: errors of stats[0..3] in units of 1e-6 (1 + |x|)",
          ("grad", "stats", "adam"), lambda p, t, c, batch, dtype, flag: R.loss_autograd(p, batch, dtype, value_clip=flag, **PPO_KW)),
    _mode("sym", "ppo_grad_sym_parity.json", "tests/test_gpu_ppo_symmetry.py: " + GRAD_WHAT + "stats: errors of stats[0..3] in units of 1e-6 (1 + |x|); "
          "mirror: the kernel on the mirrored minibatch against the original minibatch's float64 gradient", ("grad", "stats", "mirror", "adam", "demo"),
          lambda p, t, c, batch, dtype, flag: PS.loss_autograd_sym(p, t, batch, dtype, value_clip=flag, **PPO_KW),
          tables=_random_tables, make_storage=lambda net, p, t, n: PS.make_storage_sym(p, t, n, seed=2), in_policy=True, batches=B8),
    _mode("mirror", "ppo_grad_mirror_parity.json", "tests/test_gpu_ppo_mirror.py: " + GRAD_WHAT + "stats: errors of stats[0..3] and stats[7] in units "
          "of 1e-6 (1 + |x|); critic: the critic's tensors at coef 4 against the float64 gradient of the PLAIN loss", ("grad", "stats", "critic", "demo"),
          lambda p, t, c, batch, dtype, flag: PM.loss_autograd_mirror(p, t, c, batch, dtype, value_clip=flag, **PPO_KW),
          tables=_random_tables, setter=lambda env, t, c: env.set_policy_mirror_loss(t, c), coefs=(0.0, 0.5, 4.0), batches=B8,
          pick=_with_stat7, stat7="positive"),
    _mode("dup", "ppo_grad_dup_parity.json", "tests/test_gpu_ppo_dup.py: " + GRAD_WHAT + "stats: errors of stats[0..3] and stats[7] in units of 1e-6 "
          "(1 + |x|); doubled: mocca_ppo_grad_dup and the plain mocca_ppo_grad on duplicate_minibatch's 2 B rows against the same float64 gradient; "
          "critic: the critic's tensors with the advantages zeroed", ("grad", "stats", "doubled", "critic", "demo"),
          lambda p, t, c, batch, dtype, flag: PD.loss_autograd_dup(p, t, batch, dtype, value_clip=flag, **PPO_KW),
          make_policy=PD.make_policy, tables=_swapped_and_negated_tables, make_storage=lambda net, p, t, n: PD.make_storage_dup(p, t, n, seed=2),
          setter=lambda env, t, c: env.set_policy_mirror_dup(t), batches=B8, pick=_with_stat7, samples=2, stat7="nonzero"),
    _mode("distill", "distill_parity.json", "tests/test_gpu_distill.py: gradient errors per parameter tensor relative to that tensor's largest "
          "|g_f64|, pooled over the tensors whose f64 gradient is not identically zero, as [median, p99, max], kernel and float32 autograd "
          "yardstick; stats: errors of stats[1], stats[2], stats[7] in units of 1e-6 (1 + |x|)", ("grad", "stats"),
          lambda p, t, c, batch, dtype, flag: D.loss_autograd(p, batch, dtype, use_value=flag, **DISTILL_KW),
          make_storage=lambda net, p, t, n: D.make_storage(net, p, n, seed=2), kw=DISTILL_KW, flag=lambda n: n % 3 != 1,
          run=lambda env, d, flag, **kw: env.distill_grad(d["obs"], d["target"], d["value_target"] if flag else None, **kw),
          suffix=("-novalue", ""), contract_flags=(True, True), pick=lambda s: s[[1, 2, 7]], errors=D.pooled_errors, stat7="positive",
          checks=_distill_checks))}


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def record(mode, section, key, value):
    out = os.environ.get("MOCCA_TEST_OUT")     # a directory: measured figures are collected there (profiles/<mode.file>)
    if not out:
        return
    path = os.path.join(out, mode.file)
    doc = json.load(open(path)) if os.path.exists(path) else {"what": mode.what, **{s: {} for s in mode.sections}}
    doc[section][key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


_STORAGE = {}


def storage(mode, name, norm, n_rows):
    """(policy, tables or None, storage) of the net `name`, computed once per mode and left unchanged"""
    key = (mode.name, name, norm, n_rows)
    if key not in _STORAGE:
        p, tables = mode.make_policy(name, norm=norm, seed=1), mode.tables(name)
        _STORAGE[key] = (p, tables, mode.make_storage(name, p, tables, n_rows))
    return _STORAGE[key]


def to_device(st, strided=False):
    """the storage on the device; strided: obs is a view of wider rows whose other floats are NaN"""
    import torch
    d = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    if strided:
        wide = torch.full((st["obs"].shape[0], st["obs"].shape[1] + 13), float("nan"), device="cuda")
        wide[:, :st["obs"].shape[1]] = d["obs"]
        d["obs"] = wide[:, :st["obs"].shape[1]]
    return d


def attach(mode, env, p, tables, coef=None):
    """set_policy, then the mode's setter if it has one"""
    env.set_policy(device_policy(p, tables if mode.in_policy else None))
    if mode.setter:
        mode.setter(env, tables, coef)


def call(mode, env, d, idx=None, flag=False, **kw):
    """the mode's env call on the device storage `d` -> (grad, stats) as numpy"""
    import torch
    out = mode.run(env, d, flag, idx=None if idx is None else torch.from_numpy(idx).cuda(), **{**mode.kw, **kw})
    torch.cuda.synchronize()
    return out["grad"].cpu().numpy(), out["stats"].cpu().numpy()


def gpu_compute(mode, env):
    """parity's `compute` on the handle `env`"""
    def compute(p, tables, st, idx, flag, strided, coef):
        attach(mode, env, p, tables, coef)
        return call(mode, env, to_device(st, strided), idx, flag)
    return compute


def configs(mode, batches=None):
    """(B, idx form, norm, the fourth flag, strided, coef): every batch size with both index forms and the normalisation on and off; the
    flag and the strided obs cycle with periods 3 and 5, so that each meets both index forms and both normalisations; the setter's weight
    cycles over mode.coefs in runs of three configurations, so that every weight meets the flag on and off"""
    n = 0
    for b in batches or mode.batches:
        for form in ("null", "perm"):
            for norm in (True, False):
                yield b, form, norm, mode.flag(n), n % 5 < 2, mode.coefs[(n // 3) % len(mode.coefs)]
                n += 1


def parity(mode, name, compute, batches=None):
    """The acceptance loop of the module docstring on the net `name`.  compute(p, tables, st, idx, flag, strided, coef) -> (grad, stats)
    as float32 numpy is the code under test, and the only thing here that may touch a device.  -> the failures, [] when it passes"""
    failures, pool_got, pool_yard, pool_keys, s_got, s_yard = [], [], [], [], [], []

    def flush():
        got, yard = R.triple(np.concatenate(pool_got)), R.triple(np.concatenate(pool_yard))
        key = "+".join(pool_keys)
        print(f"{name} {key}: kernel {got}, f32 autograd {yard}")
        record(mode, "grad", f"{name}:{key}", {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard, "elements": int(sum(map(len, pool_got)))})
        if not R.within(got, yard):
            failures.append((key, got, yard))
        pool_got.clear(), pool_yard.clear(), pool_keys.clear()

    cfgs = list(configs(mode, batches))
    assert len(cfgs) == 4 * len(batches or mode.batches) and {c[4] for c in cfgs} == {False, True}
    assert {(c[3], c[5]) for c in cfgs} == set(itertools.product((False, True), mode.coefs))
    for i, (b, form, norm, flag, strided, coef) in enumerate(cfgs):
        n_rows = b if form == "null" else b + 7
        p, tables, st = storage(mode, name, norm, n_rows)
        idx = None
        if form == "perm":      # a slice of a permutation, with one row repeated
            idx = np.random.default_rng(b).permutation(n_rows)[:b].astype(np.int64)
            idx[-1] = idx[0]
        grad, stats = compute(p, tables, st, idx, flag, strided, coef)
        batch = R.gather(st, idx, b)
        ref, f32 = mode.loss(p, tables, coef, batch, "float64", flag), mode.loss(p, tables, coef, batch, "float32", flag)
        pool_got.append(mode.errors(p, grad, ref.grad)), pool_yard.append(mode.errors(p, f32.grad, ref.grad))
        pool_keys.append(f"B{b}-{form}-{'norm' if norm else 'raw'}{mode.suffix[flag]}{'' if coef is None else f'-c{coef:g}'}")
        s_got.append(R.stat_units(mode.pick(stats), mode.pick(ref.stats))), s_yard.append(R.stat_units(mode.pick(f32.stats), mode.pick(ref.stats)))
        samples = mode.samples * b
        if stats[4] != np.float32(round(ref.stats[4] * samples)) / np.float32(samples):
            failures.append((pool_keys[-1], "clip fraction", float(stats[4]), ref.stats[4]))
        sq = float((grad.astype(np.float64) ** 2).sum())
        if abs(float(stats[5]) - sq) > 1e-5 * sq:
            failures.append((pool_keys[-1], "sum of grad^2", float(stats[5]), sq))
        if stats[6] != 0 or (mode.stat7 == "zero" and stats[7] != 0):
            failures.append((pool_keys[-1], "stats[6], stats[7]", float(stats[6]), float(stats[7])))
        failures.extend((pool_keys[-1], *f) for f in (mode.checks(p, grad, stats, ref, flag) if mode.checks else ()))
        rest = sum(ref.grad.size for _ in cfgs[i + 1:])
        if sum(map(len, pool_got)) >= 1000 and (rest >= 1000 or rest == 0):
            flush()
    if pool_got:
        flush()
    got, yard = R.triple(np.concatenate(s_got)), R.triple(np.concatenate(s_yard))
    print(f"{name} stats: kernel {got}, f32 autograd {yard}")
    record(mode, "stats", name, {"kernel_vs_f64": got, "f32_autograd_vs_f64": yard})
    if not R.within(got, yard):
        failures.append(("stats", got, yard))
    return failures


def same_bits_contract(mode, env):
    """two calls on the same inputs give the same bits; grad / stats pre-filled with NaN are fully overwritten; idx = identity is idx NULL;
    the outputs are finite, stats[6] is 0 and stats[7] what the mode leaves there"""
    import torch
    p, tables, st = storage(mode, "mixed", True, 100)
    attach(mode, env, p, tables, 0.5)
    d, flag = to_device(st), mode.contract_flags[0]
    first = call(mode, env, d, flag=flag)
    again = call(mode, env, d, flag=flag)
    grad, stats = torch.full((env.policy.n_head(),), float("nan"), device="cuda"), torch.full((8,), float("nan"), device="cuda")
    mode.run(env, d, flag, grad=grad, stats=stats, **mode.kw)
    ident = call(mode, env, d, idx=np.arange(100, dtype=np.int64), flag=flag)
    for other in (again, (grad, stats), ident):
        assert same(first[0], other[0]) and same(first[1], other[1])
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and STAT7[mode.stat7](first[1][7]) and first[1][6] == 0


def graph_replay_contract(mode, env):
    """A graph captured after a warm call replays to the eager bits, before and after an update_policy made between the replays (a
    setter's attachment survives it).  mocca_act's outputs after gradient calls equal those before: the image is only read; and where the
    mode has a setter, act's bits with it attached are its bits with nothing attached: the attachment is for the gradient only"""
    import torch
    p, tables, st = storage(mode, "ppo", True, 100)
    q = mode.make_policy("ppo", norm=True, seed=9)
    env.set_policy(device_policy(p, tables if mode.in_policy else None))
    d = to_device(st)
    obs4 = d["obs"][:4].contiguous()
    before = {k: v.clone() for k, v in env.act(obs4, deterministic=True).items()}
    if mode.setter:
        mode.setter(env, tables, 4.0)
        attached = env.act(obs4, deterministic=True)
        assert all(same(before[k], attached[k]) for k in before)
    grad, stats = torch.empty(env.policy.n_head(), device="cuda"), torch.empty(8, device="cuda")
    run = lambda g, s: mode.run(env, d, mode.contract_flags[1], grad=g, stats=s, **mode.kw)
    run(grad, stats)      # warm: the scratch is allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(grad, stats)
    for pol in (p, q):
        env.update_policy(device_policy(pol))
        grad.fill_(float("nan"))
        graph.replay()
        eager_g, eager_s = torch.empty_like(grad), torch.empty_like(stats)
        run(eager_g, eager_s)
        torch.cuda.synchronize()
        assert same(grad, eager_g) and same(stats, eager_s) and STAT7[mode.stat7](eager_s[7].item())
        if pol is p:
            after = env.act(obs4, deterministic=True)
            assert all(same(before[k], after[k]) for k in before)
            first = grad.clone()
    assert not same(first, grad)
