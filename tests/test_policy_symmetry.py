"""The mirror-symmetric device policy off the GPU: the ABI's entry point, symmetry.mirror_tables / check_tables, the numpy call of a
`DevicePolicy(symmetry=)`, symmetry.SymmetricGaussian (the torch side of the PPO update) and the checker of the GPU tests itself
(tests/policy_symmetry_reference.py: every mutation is told apart from the definition)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import policy_reference as R
import policy_symmetry_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mocca_set_policy_symmetry"


def _ok(got, yard):
    """test_policy.py's rule: within 3 x the float32 yardstick at the median, the 99th percentile and the maximum"""
    return all(got[i] <= 3.0 * yard[i] + 1e-9 for i in range(3))


def _cat(m, v):
    return np.concatenate([np.asarray(m).ravel(), np.asarray(v).ravel()])


def test_header_and_binding_list_the_entry_point_and_a_null_handle_is_an_argument_error():
    from mocca_envs_amd import lib
    from mocca_envs_amd.build import build_lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocca.h")).read(), flags=re.S)
    assert NEW in set(re.findall(r"\b(mocca_[a-z_]+)\s*\(", src)) and NEW in lib.SYMBOLS
    assert "#define MOCCA_ABI_VERSION 8" in src and lib.ABI_VERSION == 8
    so = C.CDLL(build_lib())
    assert hasattr(so, NEW)
    assert lib.load().mocca_set_policy_symmetry(None, None, None, None, None) == -1


def _env_ids_with_six_lists():
    from mocca_envs_amd import model as M
    from mocca_envs_amd.vec_env import TASKS
    return sorted(k for k, t in TASKS.items() if t != M.TASK_CASSIE)


@pytest.mark.parametrize("env_id", _env_ids_with_six_lists())
def test_mirror_tables_of_every_env_are_valid_and_are_the_mirror_transforms(env_id):
    import torch
    from mocca_envs_amd import host_logic as H, model as M
    from mocca_envs_amd.symmetry import MirrorTransform, check_tables, mirror_tables
    from mocca_envs_amd.vec_env import TASKS, compile_model_for
    m, stepper = compile_model_for(env_id), TASKS[env_id] == M.TASK_WALKER3D_STEPPER
    obs_dim, act_dim = 6 + 2 * m.n_joints + m.n_feet + (5 * (m.lookbehind + 2) if stepper else 2), m.n_joints
    mi = H.mirror_indices(m, stepper=stepper)
    t = mirror_tables(mi, obs_dim, act_dim)
    assert [x.dtype for x in t] == [np.int32, np.float32, np.int32, np.float32] and [x.shape for x in t] == [(obs_dim,)] * 2 + [(act_dim,)] * 2
    check_tables(t, obs_dim, act_dim)
    mt = MirrorTransform(mi, obs_dim, act_dim)
    assert np.array_equal(t[0], mt.obs_perm.numpy()) and np.array_equal(t[1], mt.obs_sign.numpy())
    assert np.array_equal(t[2], mt.act_perm.numpy()) and np.array_equal(t[3], mt.act_sign.numpy())
    x = torch.randn(3, obs_dim)
    assert np.array_equal(S.mirror(x.numpy(), t[0], t[1]), mt.obs(x).numpy())
    assert len(mi[1]) > 0 and np.array_equal(t[0][np.asarray(mi[1])], np.asarray(mi[2])) and np.all(t[1][np.asarray(mi[0])] == -1.0)


def test_mirror_tables_with_a_scan_pattern():
    from mocca_envs_amd import host_logic as H, model as M
    from mocca_envs_amd.perception import scan_grid
    from mocca_envs_amd.symmetry import mirror_tables
    mi = H.mirror_indices(M.compile_walker3d(), stepper=False)
    pts = scan_grid((-0.5, 1.5), (-0.6, 0.6), 4, 5)                 # y in {-0.6, -0.3, 0, 0.3, 0.6}: symmetric, the middle column on the axis
    in_perm, in_sign, _, _ = mirror_tables(mi, 52, 21, scan_points=pts)
    assert in_perm.shape == (72,) and np.all(in_sign[52:] == 1.0)
    for p, (px, py) in enumerate(pts):
        q = in_perm[52 + p] - 52
        assert 0 <= q < 20 and pts[q][0] == px and abs(pts[q][1] + py) <= 1e-6, p
        if py == 0:
            assert q == p
    assert np.array_equal(in_perm[:52], mirror_tables(mi, 52, 21)[0])
    one_sided = scan_grid((0.0, 1.0), (0.0, 0.6), 3, 3)           # y in {0, 0.3, 0.6}: 0.3 has no reflection
    with pytest.raises(ValueError, match="reflection"):
        mirror_tables(mi, 52, 21, scan_points=one_sided)
    line = scan_grid((0.0, 1.0), (0.0, 0.0), 5, 1)                # all on the axis: every point its own image
    assert np.array_equal(mirror_tables(mi, 52, 21, scan_points=line)[0][52:], 52 + np.arange(5))
    with pytest.raises(ValueError):
        mirror_tables(mi, 52, 21, scan_points=np.zeros((4, 3)))
    with pytest.raises(ValueError):
        mirror_tables({"left_obs_inds": []}, 52, 21)


def test_check_tables_rejects_each_kind_of_bad_table():
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.symmetry import check_tables
    good = S.random_tables(36, 3, act_dim=10)
    check_tables(good, 36, 10)
    pair = next(k for k in range(36) if good[0][k] != k)

    def broken(which, fn):
        t = [x.copy() for x in good]
        fn(t[which])
        return tuple(t)

    def three_cycle(perm):
        a, b, c = [k for k in range(len(perm)) if perm[k] == k][:3]
        perm[a], perm[b], perm[c] = b, c, a

    def flip_one(sign):
        sign[pair] = -sign[pair]

    def half(sign):
        sign[0] = 0.5

    def out_of_range(perm):
        perm[0] = len(perm)

    def negative(perm):
        perm[0] = -1

    for what, bad in (("involution", broken(0, three_cycle)), ("swapped pair", broken(1, flip_one)), (r"\+1 or -1", broken(1, half)),
                      ("outside", broken(0, out_of_range)), ("outside", broken(0, negative)), ("involution", broken(2, three_cycle)),
                      (r"\+1 or -1", broken(3, half)), ("outside", broken(2, out_of_range))):
        with pytest.raises(ValueError, match=what):
            check_tables(bad, 36, 10)
    with pytest.raises(ValueError, match="entries"):
        check_tables(good, 37, 10)
    with pytest.raises(ValueError):
        check_tables(good[:3])
    with pytest.raises(ValueError, match="integers"):
        check_tables((good[0].astype(np.float32),) + good[1:])
    p = R.random_policy("small", 36, 10, norm=True, seed=1)
    with pytest.raises(ValueError):
        DevicePolicy(p.actor, p.critic, p.log_std, symmetry=S.random_tables(52, 3, act_dim=10))       # tables of another in_dim
    with pytest.raises(ValueError):
        S.device_policy(p, broken(1, half))


@pytest.mark.parametrize("kind,in_dim,act_dim", [("ppo", 52, 21), ("small", 142, 21), ("deep8", 36, 10)])
@pytest.mark.parametrize("norm", [True, False])
def test_the_numpy_call_is_the_f64_definition_and_every_mutation_is_told_apart(kind, in_dim, act_dim, norm):
    """The statistics of random_policy have non-zero means on negated features (mean ~ N(0, 1)): a mirror applied after the normalisation
    differs from the definition.  Without normalisation that mutation IS the definition and is not run."""
    p, tables = R.random_policy(kind, in_dim, act_dim, norm=norm, seed=21), S.random_tables(in_dim, 4, act_dim=act_dim)
    if norm:
        assert np.all(np.abs(p.obs_mean[tables[1] < 0]) > 0)
    dp = S.device_policy(p, tables)
    x = R.plausible_inputs(200, in_dim, seed=6)
    eps = np.random.default_rng(7).normal(size=(200, act_dim)).astype(np.float32)
    action, logp, value, mean = dp(x, eps)
    want = _cat(*S.sym_forward64(p, tables, x))
    yard = R.triple(R.error_units(_cat(*S.sym_torch32(p, tables, x)), want))
    got = R.triple(R.error_units(_cat(mean, value), want))
    assert _ok(got, yard), (got, yard)
    for how in S.MUTATIONS:
        if how == "mirror_after_norm" and not norm:
            continue
        wrong = _cat(*S.sym_forward64(p, tables, x, how))
        assert not _ok(R.triple(R.error_units(_cat(mean, value), wrong)), yard), how
        assert not _ok(R.triple(R.error_units(_cat(*S.sym_torch32(p, tables, x)), wrong)), yard), how      # the yardstick tells them apart too
    # the sample: the formula at the symmetric mean under the symmetrised log_std
    ls64, ls32 = S.log_std_sym(p, tables), S.log_std_sym(p, tables, np.float32)
    a64, lp64 = R.sample64(mean, ls64, eps)
    a32, lp32 = R.sample32(mean, ls32, eps)
    for got, y32, w in ((action, a32, a64), (logp, lp32, lp64)):
        assert _ok(R.triple(R.error_units(got, w)), R.triple(R.error_units(y32, w)))
    det = dp(x)
    assert np.array_equal(det[0], det[3]) and np.array_equal(det[3], mean)
    # the symmetry is not a parameter; without it the call is the plain one
    plain = S.device_policy(p)
    assert np.array_equal(dp.flat_params(), plain.flat_params()) and np.array_equal(dp.table(), plain.table())
    assert np.array_equal(dp.pack()[0], plain.pack()[0]) and dp.with_symmetry(None).symmetry is None
    for a, b in zip(dp.with_symmetry(None)(x, eps), plain(x, eps)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind,in_dim,act_dim", [("ppo", 52, 21), ("small", 36, 10)])
def test_numpy_equivariance(kind, in_dim, act_dim):
    """policy(M_o x) = (M_a mean, the same value), compared with == on floats: 1/2 (a + b) is commutative, but a sum that cancels to zero
    may come out as -0 on one side and +0 on the other"""
    p, tables = R.random_policy(kind, in_dim, act_dim, norm=True, seed=22), S.random_tables(in_dim, 5, act_dim=act_dim)
    dp = S.device_policy(p, tables)
    x = R.plausible_inputs(64, in_dim, seed=8)
    eps = np.random.default_rng(9).normal(size=(64, act_dim)).astype(np.float32)
    xm, em = S.mirror(x, tables[0], tables[1]), S.mirror(eps, tables[2], tables[3])
    assert np.array_equal(S.mirror(xm, tables[0], tables[1]), x)
    a, lp, v, m = dp(x, eps)
    am, lpm, vm, mm = dp(xm, em)
    assert np.all(mm == S.mirror(m, tables[2], tables[3])) and np.all(vm == v) and np.all(am == S.mirror(a, tables[2], tables[3]))
    assert np.allclose(lpm, lp, rtol=0, atol=1e-4)
    assert np.abs(S.mirror(m, tables[2], tables[3]) - m).max() > 1e-3          # the tables do something


def _gaussian(kind, in_dim, act_dim, norm, seed):
    import torch
    from mocca_envs_amd.symmetry import SymmetricGaussian
    p, tables = R.random_policy(kind, in_dim, act_dim, norm=norm, seed=seed), S.random_tables(in_dim, 6, act_dim=act_dim)
    actor, critic, log_std = S.sequentials(p, torch.float64)
    stats = {} if not norm else dict(obs_mean=torch.from_numpy(p.obs_mean).double(), inv_std=torch.from_numpy(p.inv_std).double())
    return p, tables, SymmetricGaussian(actor, critic, log_std, tables), dict(stats, clip=p.clip)


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
@pytest.mark.parametrize("norm", [True, False])
def test_symmetric_gaussian_in_f64_is_the_definition(kind, norm):
    import torch
    in_dim, act_dim = (52, 21) if kind == "ppo" else (36, 10)
    p, tables, g, kw = _gaussian(kind, in_dim, act_dim, norm, 23)
    assert g.log_std is [q for q in g.parameters() if q.shape == (act_dim,) and q.dim() == 1 and q is g.log_std][0]      # shared, registered
    assert g.actor[0].weight.data_ptr() in {q.data_ptr() for q in g.parameters()}
    x = R.plausible_inputs(50, in_dim, seed=10)
    mean, ls, value = g(torch.from_numpy(x).double(), **kw)
    m64, v64 = S.sym_forward64(p, tables, x)
    assert np.abs(mean.detach().numpy() - m64).max() <= 1e-12 and np.abs(value.detach().numpy() - v64).max() <= 1e-12
    assert np.abs(ls.detach().numpy() - S.log_std_sym(p, tables)).max() <= 1e-12
    eps = np.random.default_rng(11).normal(size=m64.shape)
    action, lp64 = R.sample64(m64, S.log_std_sym(p, tables), eps)
    logp, entropy, value2 = g.evaluate_actions(torch.from_numpy(x).double(), torch.from_numpy(action), **kw)
    assert np.abs(logp.detach().numpy() - lp64).max() <= 1e-10 and torch.equal(value2, value)
    closed = (S.log_std_sym(p, tables) + 0.5 + 0.5 * np.log(2 * np.pi)).sum()
    assert entropy.shape == logp.shape and np.abs(entropy.detach().numpy() - closed).max() <= 1e-12
    # float32 modules take float32 rows
    a32, c32, l32 = S.sequentials(p, torch.float32)
    from mocca_envs_amd.symmetry import SymmetricGaussian
    m32 = SymmetricGaussian(a32, c32, l32, tables)(torch.from_numpy(x), **({} if not norm else dict(
        obs_mean=torch.from_numpy(p.obs_mean), inv_std=torch.from_numpy(p.inv_std))), clip=p.clip)[0]
    assert m32.dtype == torch.float32 and np.abs(m32.detach().numpy() - m64).max() < 1e-3


def test_symmetric_gaussian_gradients():
    """gradcheck on the "small" shape (inputs away from the clip and from softsign's kink), and: mirroring the inputs leaves the loss gradient
    of the shared parameters unchanged"""
    import torch
    p, tables, g, kw = _gaussian("small", 36, 10, True, 24)
    mt = lambda t, perm, sign: t[..., torch.from_numpy(perm.astype(np.int64))] * torch.from_numpy(sign).double()
    rng = np.random.default_rng(12)
    x = torch.from_numpy(p.obs_mean.astype(np.float64) + rng.uniform(-1, 1, (3, 36)) / p.inv_std).requires_grad_(True)    # |normalised| <= 1 < clip
    action = torch.from_numpy(rng.normal(size=(3, 10))).requires_grad_(True)
    params = list(g.parameters())

    def fn(obs, act, *_):
        return g.evaluate_actions(obs, act, **kw)

    assert torch.autograd.gradcheck(fn, (x, action, *params), eps=1e-6, atol=1e-6, rtol=1e-5)

    def grads(obs, act):
        logp, entropy, value = g.evaluate_actions(obs, act, **kw)
        loss = (logp * torch.linspace(-1, 1, logp.numel()).double()).sum() + (value ** 2).sum() + 0.01 * entropy.mean() + torch.exp(0.1 * logp).sum()
        return torch.autograd.grad(loss, params)

    X = torch.from_numpy(R.plausible_inputs(40, 36, seed=13)).double()          # these reach the clip
    A = torch.from_numpy(rng.normal(size=(40, 10)))
    ga, gb = grads(X, A), grads(mt(X, tables[0], tables[1]), mt(A, tables[2], tables[3]))
    assert max(float(u.abs().max()) for u in ga) > 1e-2
    for u, v in zip(ga, gb):
        assert float((u - v).abs().max()) <= 1e-10


def test_from_torch_and_the_gaussian_share_one_definition():
    import torch
    from mocca_envs_amd.policy import DevicePolicy
    p, tables, g, kw = _gaussian("small", 36, 10, True, 25)
    dp = DevicePolicy.from_torch(g.actor, g.critic, g.log_std, obs_mean=p.obs_mean, obs_var=1.0 / p.inv_std.astype(np.float64) ** 2, eps=0.0,
                                 clip=p.clip, symmetry=tables)
    assert dp.symmetry is not None and np.array_equal(dp.symmetry[0], tables[0])
    x = R.plausible_inputs(20, 36, seed=14)
    mean, _, value = g(torch.from_numpy(x).double(), obs_mean=torch.from_numpy(dp.obs_mean).double(), inv_std=torch.from_numpy(dp.inv_std).double(),
                       clip=p.clip)
    _, _, v, m = dp(x)
    assert np.abs(m - mean.detach().numpy()).max() < 1e-4 and np.abs(v - value.detach().numpy()).max() < 1e-4
