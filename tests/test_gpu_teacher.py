"""The teacher's slot on the GPU (include/mocca.h mocca_set_teacher / mocca_update_teacher / mocca_teacher_act): the bits of mocca_act with the
same weights, parity with the float64 forward on row counts that are not the handle's, a student left as it was, and the refusals.  The
checker is tests/policy_reference.py."""
import ctypes as C

import numpy as np
import pytest

import policy_reference as R
import ppo_reference as P

pytestmark = pytest.mark.gpu
NS = (1, 17, 63, 100)      # one row, one past the 16-row tile, odd, several workgroups -- on a 4-env handle


@pytest.fixture(scope="module")
def env():
    from mocca_envs_amd.vec_env import VecEnv
    e = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    yield e
    e.set_teacher(None)
    e.close()


def _dp(p, **kw):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip, **kw)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).reshape(-1).view(np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ok(got, yard):
    return all(got[i] <= 3.0 * yard[i] for i in range(3))


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
def test_same_weights_give_the_bits_of_act(norm):
    """the SAME weights in both slots: teacher_act on n_envs rows gives mocca_act(deterministic = 1)'s mean and value, bit for bit"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    n = 37
    e = VecEnv("Walker3DCustomEnv-v0", n, device=0)
    p = R.random_policy("ppo", 52, 21, norm=norm, seed=11)
    e.set_policy(_dp(p))
    e.set_teacher(_dp(p))
    x = torch.from_numpy(R.plausible_inputs(n, 52, seed=3)).cuda()
    a = e.act(x, deterministic=True, out={"mean": torch.empty(n, 21, device="cuda")})
    t = e.teacher_act(x)
    torch.cuda.synchronize()
    assert _same(a["mean"], t["mean"]) and _same(a["value"], t["value"]) and _same(a["action"], t["mean"])
    mean_only = torch.full((n, 21), float("nan"), device="cuda")      # value_dev NULL: the critic is not run
    ptr = lambda v: C.c_void_p(v.data_ptr())
    assert e.lib.mocca_teacher_act(e.h, ptr(x), 52, n, ptr(mean_only), None, e._stream()) == 0
    torch.cuda.synchronize()
    assert _same(mean_only, t["mean"])
    e.close()


@pytest.mark.parametrize("n", NS)
def test_parity_on_row_counts_that_are_not_n_envs(env, n):
    """tests/test_gpu_policy.py's rule on n rows of a 4-env handle: mean and value within 3 x torch-CPU-f32 against the float64 forward, in
    units of 1e-6 (1 + |x|), at the median, the 99th percentile and the maximum; strided rows carry NaN beyond in_dim; the floats around
    the outputs are untouched"""
    import torch
    cat = lambda m, v: np.concatenate([np.asarray(m).ravel(), np.asarray(v).ravel()])
    failures = []
    for kind, in_dim, act_dim, norm in (("ppo", 52, 21, True), ("small", 36, 10, False), ("deep8", 142, 21, True)):
        p = R.random_policy(kind, in_dim, act_dim, norm=norm, seed=11)
        env.set_teacher(_dp(p))
        x = R.plausible_inputs(n, in_dim, seed=n)
        wide = torch.full((n, in_dim + 19), float("nan"), device="cuda")
        wide[:, :in_dim] = torch.from_numpy(x).cuda()
        mean, value = torch.full((n + 1, act_dim), 7.0, device="cuda"), torch.full((n + 1,), 7.0, device="cuda")
        env.teacher_act(wide[:, :in_dim], mean=mean[:n], value=value[:n])
        torch.cuda.synchronize()
        want = cat(*R.forward64(p, x))
        yard = R.triple(R.error_units(cat(*R.torch32(p, x)), want))
        got = R.triple(R.error_units(cat(mean[:n].cpu().numpy(), value[:n].cpu().numpy()), want))
        print(f"{kind}-n{n}: teacher vs f64 {got}, torch f32 vs f64 {yard}")
        if not _ok(got, yard):
            failures.append((kind, got, yard))
        if not ((mean[n] == 7.0).all() and value[n] == 7.0):
            failures.append((kind, "wrote past n_rows"))
    assert not failures, failures


def test_the_student_is_untouched_and_the_slots_may_differ(env):
    """a symmetric student of one shape, a teacher of another in_dim and other layers: setting, updating and detaching the teacher leaves
    act's bits, the attached symmetry and ppo_grad's bits as they were"""
    import torch
    import policy_symmetry_reference as PS
    sp = P.make_policy("tiny", norm=True, seed=1)
    st = P.make_storage(sp, 17, seed=2)
    d = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    tables = PS.random_tables(5, 3, 3)
    obs4 = d["obs"][:4].contiguous()
    grad = lambda: env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], clip=0.2, value_coef=0.5, entropy_coef=0.01)

    def snapshot():
        a = {k: v.clone() for k, v in env.act(obs4, deterministic=True).items()}
        g = grad()
        return [a["action"], a["value"], a["logp"], g["grad"].clone(), g["stats"].clone()]

    for sym in (None, tables):
        env.set_teacher(None)
        env.set_policy(_dp(sp, symmetry=sym))
        before = snapshot()
        tp = R.random_policy("deep8", 65, 3, norm=True, seed=4)
        env.set_teacher(_dp(tp))
        x = torch.from_numpy(R.plausible_inputs(9, 65, seed=1)).cuda()
        first = env.teacher_act(x)
        after_set = snapshot()
        tq = R.random_policy("deep8", 65, 3, norm=False, seed=5)
        env.update_teacher(_dp(tq))
        second = env.teacher_act(x)
        after_update = snapshot()
        env.set_teacher(None)
        after_detach = snapshot()
        torch.cuda.synchronize()
        for other in (after_set, after_update, after_detach):
            assert all(_same(a, b) for a, b in zip(before, other))
        assert (getattr(env.policy, "symmetry", None) is not None) == (sym is not None)
        m64, v64 = R.forward64(tq, x.cpu().numpy())
        assert np.abs(second["mean"].cpu().numpy() - m64).max() < 1e-4 and not _same(first["mean"], second["mean"])
        with pytest.raises(Exception):
            env.teacher_act(x)      # detached
    with pytest.raises(ValueError):
        env.set_teacher(_dp(sp, symmetry=tables))


def test_refusals(env):
    import torch
    from mocca_envs_amd import lib as L
    p = R.random_policy("small", 36, 10, norm=True, seed=2)
    dp = _dp(p)
    x = torch.from_numpy(R.plausible_inputs(5, 36, seed=1)).cuda()
    mean, value = torch.full((5, 10), 7.0, device="cuda"), torch.full((5,), 7.0, device="cuda")
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())

    def raw(rows=x, stride=36, n=5, m=mean):
        rc = env.lib.mocca_teacher_act(env.h, ptr(rows), stride, n, ptr(m), ptr(value), env._stream())
        return rc, (env.lib.mocca_last_error(env.h) or b"").decode()

    env.set_teacher(None)
    rc, msg = raw()
    assert rc != 0 and "mocca_set_teacher" in msg
    table = np.ascontiguousarray(dp.table(), np.int32)      # shapes only: the image is not filled until mocca_update_teacher
    assert env.lib.mocca_set_teacher(env.h, table.ctypes.data_as(C.c_void_p), table.shape[0], 36, 10, 5.0) == 0
    rc, msg = raw()
    assert rc != 0 and "mocca_update_teacher" in msg
    flat = torch.from_numpy(dp.flat_params()).cuda()
    assert env.lib.mocca_update_teacher(env.h, ptr(flat), flat.numel() - 1, env._stream()) != 0      # neither of the two lengths
    assert env.lib.mocca_update_teacher(env.h, None, flat.numel(), env._stream()) != 0
    assert env.lib.mocca_set_teacher(env.h, table.ctypes.data_as(C.c_void_p), table.shape[0], 35, 10, 5.0) != 0      # mocca_set_policy's shape checks
    env.set_teacher(dp)
    for kw in (dict(stride=35), dict(n=0), dict(n=-3), dict(rows=None), dict(m=None)):
        rc, msg = raw(**kw)
        assert rc != 0 and msg.startswith("mocca_teacher_act:"), (kw, rc, msg)
    torch.cuda.synchronize()
    assert (mean == 7.0).all() and (value == 7.0).all()
    assert raw()[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(mean).all() and not (mean == 7.0).any()
    with pytest.raises(ValueError):
        env.teacher_act(x.double())
    with pytest.raises(ValueError):
        env.teacher_act(x[:, :20])
    env.set_teacher(None)
    with pytest.raises(L.MoccaError):
        env.teacher_act(x)
