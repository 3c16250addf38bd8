"""The device policy off the GPU: the ABI's new entry points, `policy.DevicePolicy` (image round trip, files, the numpy call) and the checker
of the GPU tests itself (tests/policy_reference.py: Philox known answers, the moments of the reference noise)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import policy_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mocca_set_policy", "mocca_update_policy", "mocca_act", "mocca_act_step")


def _as_device_policy(p):
    from mocca_envs_amd.policy import DevicePolicy
    return DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)


def test_header_and_binding_list_the_policy_entry_points_at_abi_8():
    from mocca_envs_amd import lib
    from mocca_envs_amd.build import build_lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocca.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocca_[a-z_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in lib.SYMBOLS, name
    assert "#define MOCCA_ABI_VERSION 8" in src and lib.ABI_VERSION == 8
    so = C.CDLL(build_lib())
    assert so.mocca_abi_version() == 8
    for name in NEW:
        assert hasattr(so, name), name


def test_null_handle_is_an_argument_error():
    from mocca_envs_amd import lib
    l = lib.load()
    assert l.mocca_set_policy(None, None, 0, 0, 0, 0.0) == -1
    assert l.mocca_update_policy(None, None, 0, None) == -1
    assert l.mocca_act(None, None, 0, None, 0, None, None, None, None, None) == -1
    assert l.mocca_act_step(None, None, 0, None, 0, *([None] * 9)) == -1


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
@pytest.mark.parametrize("norm", [True, False])
def test_pack_unpack_round_trip(kind, norm):
    from mocca_envs_amd.policy import DevicePolicy
    in_dim, act_dim = (142, 21) if kind == "small" else (52, 21) if kind == "ppo" else (36, 10)
    p = _as_device_policy(R.random_policy(kind, in_dim, act_dim, norm=norm, seed=3))
    image, table, off = p.pack()
    assert image.dtype == np.float32 and table.shape == (len(p.actor) + len(p.critic), 8) and image.size == off["inv_std"] + -(-in_dim // 16) * 16
    q = DevicePolicy.unpack(image, table, off)
    for a, b in zip(p.actor + p.critic, q.actor + q.critic):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(p.log_std, q.log_std) and q.clip == p.clip and (q.obs_mean is None) == (not norm)
    if norm:
        assert np.array_equal(p.obs_mean, q.obs_mean) and np.array_equal(p.inv_std, q.inv_std)
    assert np.array_equal(q.flat_params(), p.flat_params())
    n_base = sum(w.size + b.size for w, b, _ in p.actor + p.critic) + act_dim
    assert p.flat_params().size == n_base + (2 * in_dim if norm else 0)


def test_unpack_rejects_non_zero_padding():
    from mocca_envs_amd.policy import DevicePolicy
    p = _as_device_policy(R.random_policy("small", 36, 10, norm=True, seed=1))
    image, table, off = p.pack()
    DevicePolicy.unpack(image, table, off)
    spots = [int(table[-1][7]) + 1,                        # the critic head's bias, row 1 of 16 (out = 1)
             int(table[0][6]) + 256 * 2 + 4 * 4 + 1,       # first layer, block (0, 2), lane 4: row 4, column 32 + 1 = 33 < 36 is real ...
             off["log_std"] + 10, off["mean"] + 36, off["inv_std"] + 47, off["flags"] + 1]
    for k, pos in enumerate(spots):
        bad = image.copy()
        bad[pos] = 1.0
        if k == 1:
            DevicePolicy.unpack(bad, table, off)           # ... so a change there is a weight, not padding
            bad[int(table[0][6]) + 256 * 2 + 4 * (16 + 4) + 1] = 1.0     # lane 20: row 4, column 32 + 4 + 1 = 37 >= 36: padding
        with pytest.raises(ValueError):
            DevicePolicy.unpack(bad, table, off)


def test_from_npz_loads_the_trained_walker_policy_and_its_call_is_the_f64_forward():
    from mocca_envs_amd.policy import DevicePolicy
    p = DevicePolicy.from_npz(os.path.join(ROOT, "profiles", "ppo_policy_walker3d.npz"))
    assert (p.in_dim, p.act_dim) == (52, 21) and [w.shape for w, _, _ in p.actor] == [(256, 52), (256, 256), (21, 256)]
    assert [a for _, _, a in p.actor] == ["tanh", "tanh", "identity"] and p.obs_mean is not None
    x = R.plausible_inputs(200, 52, seed=4)
    eps = np.random.default_rng(5).normal(size=(200, 21)).astype(np.float32)
    action, logp, value, mean = p(x, eps)
    m64, v64 = R.forward64(p, x)
    # float32 rounding through three layers: the torch float32 forward is the yardstick, 3 x as in the GPU test
    m32, v32 = R.torch32(p, x)
    for got, yard, want in ((mean, m32, m64), (value, v32, v64)):
        g, y = R.triple(R.error_units(got, want)), R.triple(R.error_units(yard, want))
        assert all(g[i] <= 3.0 * y[i] + 1e-9 for i in range(3)), (g, y)
    a64, lp64 = R.sample64(mean, p.log_std, eps)
    a32, lp32 = R.sample32(mean, p.log_std, eps)
    for got, yard, want in ((action, a32, a64), (logp, lp32, lp64)):
        g, y = R.triple(R.error_units(got, want)), R.triple(R.error_units(yard, want))
        assert all(g[i] <= 3.0 * y[i] + 1e-9 for i in range(3)), (g, y)
    det = p(x)
    assert np.array_equal(det[0], det[3]) and np.array_equal(det[3], mean)
    assert np.allclose(det[1], -(p.log_std.astype(np.float64) + R.HALF_LOG_2PI).sum(), rtol=1e-6)


def test_from_torch_takes_the_controllers_grammar():
    import torch
    from torch import nn
    from mocca_envs_amd.policy import DevicePolicy
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(36, 32), nn.Tanh(), nn.Linear(32, 10))
    critic = nn.Sequential(nn.Linear(36, 16), nn.ReLU(), nn.Linear(16, 1))
    log_std = nn.Parameter(torch.full((10,), -0.5))
    p = DevicePolicy.from_torch(actor, critic, log_std, obs_mean=torch.zeros(36), obs_var=torch.ones(36), clip=7.0)
    assert [a for _, _, a in p.actor] == ["tanh", "identity"] and [a for _, _, a in p.critic] == ["relu", "identity"]
    assert p.clip == 7.0 and np.allclose(p.inv_std, 1.0 / np.sqrt(1.0 + 1e-8))
    x = torch.randn(5, 36)
    assert np.allclose(p(x.numpy())[3], actor(x).detach().numpy(), atol=1e-6)
    with pytest.raises(ValueError):
        DevicePolicy.from_torch(nn.Sequential(nn.Linear(36, 32), nn.Sigmoid(), nn.Linear(32, 10)), critic, log_std)
    with pytest.raises(ValueError):
        DevicePolicy.from_torch(nn.Sequential(nn.Linear(36, 24), nn.Tanh(), nn.Linear(24, 10)), critic, log_std)     # width 24


def test_reference_philox_known_answers():
    """Random123's kat_vectors for Philox4x32-10; the first is the one tests/test_oracle_physics.py checks through the oracle's draws."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32(np.array([ctr], np.uint64), key)[0]
        assert tuple(int(x) for x in got) == want


def test_reference_noise_moments_and_keying():
    n_env, A = 4096, 21
    zeros = np.zeros(n_env, np.int64)
    z = R.noise(R.NOISE_SEED, np.arange(n_env), zeros, zeros, A)
    n = z.size
    assert n == 86016
    print(f"\nreference noise, seed {R.NOISE_SEED}: mean {z.mean():.3e} (bound {4 / np.sqrt(n):.3e}), var - 1 {z.var() - 1:.3e} (bound {4 * np.sqrt(2 / n):.3e})")
    assert abs(z.mean()) <= 4.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)
    # a shard's rows are the whole batch's; step, episode and seed each change the noise; odd act_dim cuts the last pair
    assert np.array_equal(R.noise(R.NOISE_SEED, np.arange(40, 63), zeros[:23], zeros[:23], A), z[40:63])
    for other in (R.noise(R.NOISE_SEED, np.arange(8), zeros[:8] + 1, zeros[:8], A), R.noise(R.NOISE_SEED, np.arange(8), zeros[:8], zeros[:8] + 1, A),
                  R.noise(R.NOISE_SEED + 1, np.arange(8), zeros[:8], zeros[:8], A)):
        assert not np.any(other == z[:8])
    assert np.array_equal(R.noise(R.NOISE_SEED, np.arange(8), zeros[:8], zeros[:8], 10), z[:8, :10])
    z32 = R.noise(R.NOISE_SEED, np.arange(n_env), zeros, zeros, A, dtype=np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5


def test_mutations_change_the_forward():
    p = R.random_policy("ppo", 52, 21, norm=True, seed=2)
    x = R.plausible_inputs(64, 52)
    m, v = R.forward64(p, x)
    for how in ("no_norm", "no_clip", "activation"):
        mm, vm = R.forward64(R.mutated(p, how), x)
        assert np.abs(mm - m).max() > 1e-3 and np.abs(vm - v).max() > 1e-3, how
    eps = np.random.default_rng(0).normal(size=m.shape)
    a, lp = R.sample64(m, p.log_std, eps)
    for how in ("log_std_sign", "logp_no_log_std"):
        am, lpm = R.sample64_mutated(m, p.log_std, eps, how)
        assert np.abs(lpm - lp).max() > 1e-3, how
