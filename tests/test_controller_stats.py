"""`controller.BaseController` with observation statistics, on the host: the callable, the files, and the policy files of tools/ppo_demo.py."""
import os

import numpy as np
import pytest

import controller_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(seed=0):
    rng = np.random.default_rng([seed, 65])
    return rng.normal(0, 1, 65).astype(np.float32), rng.uniform(0.3, 3.0, 65).astype(np.float32), 2.0


def _ok(got, yard):
    return all(got[i] <= 3.0 * yard[i] for i in range(3))


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_call_applies_the_statistics_within_the_f32_yardstick(kind):
    """__call__ against a float64 restatement (clamp((x - mean) * inv_std, +-clip), then the nets) in units of 1e-6 (1 + |x|): within 3 x what
    torch CPU float32 gives for the same chain, at the median, the 99th percentile and the maximum -- the yardstick of
    tests/test_gpu_planner_controller.py::test_controller_parity_with_the_f64_forward.  Without the statistics, or without the clamp, it is not."""
    import torch
    from mocca_envs_amd.controller import BaseController
    c = R.random_controller(kind, seed=7)
    mean, inv_std, clip = _stats(1)
    ctrl = BaseController(c.actor, c.critic, obs_mean=mean, obs_inv_std=inv_std, clip=clip)
    assert ctrl.obs_mean.dtype == np.float32 and ctrl.obs_inv_std.dtype == np.float32
    assert np.array_equal(ctrl.obs_mean, mean) and np.array_equal(ctrl.obs_inv_std, inv_std) and ctrl.clip == clip
    rs, plan = R.plausible_inputs(500, seed=3)
    x = R.base_obs(rs, plan)                                       # float32 values in float64
    z = (x - mean.astype(np.float64)) * inv_std.astype(np.float64)
    assert (np.abs(z) > clip).any() and (np.abs(z) < clip).any()      # the clamp binds on some entries, not on others
    cat = lambda a, v: np.concatenate([np.asarray(a).ravel(), np.asarray(v).ravel()])

    def f64(zz):
        return cat(R.net64(c.actor, zz), R.net64(c.critic, zz)[..., 0])

    want = f64(np.clip(z, -clip, clip))
    value, action = ctrl(x.astype(np.float32))
    assert value.dtype == np.float32 and action.dtype == np.float32 and value.shape == (500,) and action.shape == (500, 21)
    acts = {"relu": torch.relu, "tanh": torch.tanh, "softsign": torch.nn.functional.softsign, "identity": lambda t: t}

    def net32(layers, t):
        for w, b, a in layers:
            t = acts[a](torch.nn.functional.linear(t, torch.from_numpy(w), torch.from_numpy(b)))
        return t.numpy()

    x32 = ((torch.from_numpy(x.astype(np.float32)) - torch.from_numpy(mean)) * torch.from_numpy(inv_std)).clamp(-clip, clip)
    yard = R.triple(R.error_units(cat(net32(c.actor, x32), net32(c.critic, x32)[:, 0]), want))
    got = R.triple(R.error_units(cat(action, value), want))
    print(f"\n{kind}: __call__ vs f64 median/p99/max {got}, torch f32 vs f64 {yard}")
    assert _ok(got, yard), (got, yard)
    assert not _ok(R.triple(R.error_units(cat(action, value), f64(x))), yard)          # statistics dropped
    assert not _ok(R.triple(R.error_units(cat(action, value), f64(z))), yard)          # clamp dropped
    # one row, as the single-env class calls it
    v1, a1 = ctrl(x[3].astype(np.float32))
    assert np.allclose(v1, value[3], atol=1e-5) and a1.shape == (21,)


def test_constructor_checks_the_statistics():
    from mocca_envs_amd.controller import BaseController
    c = R.random_controller("small", seed=1)
    mean, inv_std, clip = _stats(2)
    plain = BaseController(c.actor, c.critic)
    assert plain.obs_mean is None and plain.obs_inv_std is None and plain.clip == 10.0
    bad = [dict(obs_mean=mean), dict(obs_inv_std=inv_std), dict(obs_mean=mean[:64], obs_inv_std=inv_std[:64]),
           dict(obs_mean=np.where(np.arange(65) == 5, np.nan, mean), obs_inv_std=inv_std), dict(obs_mean=mean, obs_inv_std=-inv_std),
           dict(obs_mean=mean, obs_inv_std=np.where(np.arange(65) == 9, np.inf, inv_std)), dict(obs_mean=mean, obs_inv_std=inv_std, clip=0.0),
           dict(obs_mean=mean, obs_inv_std=inv_std, clip=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            BaseController(c.actor, c.critic, **kw)


def test_npz_round_trip_keeps_the_statistics(tmp_path):
    from mocca_envs_amd.controller import BaseController
    c = R.random_controller("small", seed=1)
    mean, inv_std, clip = _stats(2)
    ctrl = BaseController(c.actor, c.critic, obs_mean=mean, obs_inv_std=inv_std, clip=clip)
    path = str(tmp_path / "ctrl.npz")
    ctrl.save_npz(path)
    back = BaseController.from_npz(path)
    assert np.array_equal(back.obs_mean, mean) and np.array_equal(back.obs_inv_std, inv_std) and back.clip == clip
    assert back.obs_mean.dtype == np.float32 and back.obs_inv_std.dtype == np.float32
    x = R.base_obs(*R.plausible_inputs(8, seed=1)).astype(np.float32)
    assert all(np.array_equal(u, v) for u, v in zip(ctrl(x), back(x)))
    assert all(np.array_equal(u, v) for u, v in zip(ctrl(x), BaseController.load(path)(x)))
    # a file without statistics loads as before
    plain = BaseController(c.actor, c.critic)
    plain.save_npz(path)
    with np.load(path) as z:
        assert "obs_mean" not in z.files
    back = BaseController.from_npz(path)
    assert back.obs_mean is None and back.obs_inv_std is None
    assert all(np.array_equal(u, v) for u, v in zip(plain(x), back(x)))


def test_from_policy_npz_reads_the_ppo_demos_files(tmp_path):
    """a synthetic file in tools/ppo_demo.py's key format: tanh hidden layers, identity heads, inv_std formed as DevicePolicy forms it"""
    from mocca_envs_amd.controller import BaseController
    from mocca_envs_amd.policy import DevicePolicy
    rng = np.random.default_rng(4)
    dims = [65, 32, 16]
    data = {}
    for prefix, out in (("pi", 21), ("vf", 1)):
        d = dims + [out]
        for i in range(3):
            data[f"{prefix}_{2 * i}_weight"] = rng.normal(0, d[i] ** -0.5, (d[i + 1], d[i])).astype(np.float32)
            data[f"{prefix}_{2 * i}_bias"] = rng.normal(0, 0.1, d[i + 1]).astype(np.float32)
    data["obs_mean"], data["obs_var"] = rng.normal(0, 1, 65).astype(np.float32), rng.uniform(0.01, 4.0, 65).astype(np.float32)
    data["log_std"] = np.full(21, -1.0, np.float32)
    path = str(tmp_path / "demo_policy.npz")
    np.savez(path, env_id=np.array("Walker3DStepperEnv-v0"), env_steps=np.array(0), **data)
    ctrl = BaseController.from_policy_npz(path, eps=1e-8, clip=10.0)
    assert [a for _, _, a in ctrl.actor] == ["tanh", "tanh", "identity"] and [a for _, _, a in ctrl.critic] == ["tanh", "tanh", "identity"]
    assert np.array_equal(ctrl.actor[1][0], data["pi_2_weight"]) and np.array_equal(ctrl.critic[2][1], data["vf_4_bias"])
    dp = DevicePolicy.from_npz(path, clip=10.0, eps=1e-8)
    assert np.array_equal(ctrl.obs_inv_std, dp.inv_std) and np.array_equal(ctrl.obs_mean, dp.obs_mean) and ctrl.clip == 10.0
    assert np.array_equal(ctrl.obs_inv_std, np.float32(1) / np.sqrt(data["obs_var"] + np.float32(1e-8)))
    x = R.base_obs(*R.plausible_inputs(8, seed=1)).astype(np.float32)
    value, action = ctrl(x)
    _, _, v_dp, mean_dp = dp(x)
    assert np.array_equal(action, mean_dp) and np.array_equal(value, v_dp)
    assert all(np.array_equal(u, v) for u, v in zip(ctrl(x), BaseController.load(path)(x)))
    assert BaseController.from_policy_npz(path, eps=1e-2).obs_inv_std.max() < ctrl.obs_inv_std.max()


def test_a_policy_file_without_its_critic_is_refused():
    """profiles/ppo_policy_stepper.npz predates the critic being saved"""
    from mocca_envs_amd.controller import BaseController
    with pytest.raises(ValueError, match="critic is missing"):
        BaseController.from_policy_npz(os.path.join(ROOT, "profiles", "ppo_policy_stepper.npz"))


def test_the_committed_stepper_policy_loads_as_a_base_controller():
    """tests/golden/ppo_policy_stepper_base_controller.npz: a five-minute run of tools/ppo_demo.py on Walker3DStepperEnv-v0 with the critic
    saved -- the base controller of profiles/ppo_demo_planner_*.jsonl"""
    from mocca_envs_amd.controller import BaseController
    from mocca_envs_amd.policy import DevicePolicy
    path = os.path.join(ROOT, "tests", "golden", "ppo_policy_stepper_base_controller.npz")
    ctrl = BaseController.load(path)
    assert [w.shape for w, _, _ in ctrl.actor] == [(256, 65), (256, 256), (21, 256)] and [w.shape for w, _, _ in ctrl.critic] == [(256, 65), (256, 256), (1, 256)]
    assert ctrl.obs_mean.shape == (65,) and np.isfinite(ctrl.obs_mean).all() and (ctrl.obs_inv_std > 0).all() and ctrl.clip == 10.0
    dp = DevicePolicy.from_npz(path)
    x = R.base_obs(*R.plausible_inputs(8, seed=2)).astype(np.float32)
    value, action = ctrl(x)
    _, _, v_dp, mean_dp = dp(x)
    assert np.array_equal(action, mean_dp) and np.array_equal(value, v_dp)
