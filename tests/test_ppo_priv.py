"""PPO with a privileged critic without a GPU (include/mocca.h mocca_set_policy_priv): the checker tests/ppo_priv_reference.py has teeth --
a float32 gradient that crosses the two nets' inputs in any of three ways misses the project's rule by orders of magnitude on the critic's
tensors, and the right one passes it --, and `DevicePolicy` carries the critic's width and statistics through every form it has, a plain
policy's forms staying what they were."""
import hashlib

import numpy as np
import pytest

import ppo_priv_reference as P
import ppo_reference as R

KW = dict(clip=R.CLIP, value_coef=0.5, entropy_coef=0.01)
# the nets of ppo_grad_cases with critic_in_dim above and below in_dim (`wide` sits at the bound of 336: below only)
CASES = [("tiny", 9), ("tiny", 3), ("ppo", 95), ("ppo", 36), ("mixed", 95), ("mixed", 36), ("wide", 95), ("single", 12), ("single", 4)]
B = 100


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, dc in CASES:
        p = P.make_policy(name, critic_in_dim=dc, norm=True, seed=1)
        out[name, dc] = (p, P.make_storage(p, B, seed=2)[0])
    return out


def _triples(p, slices, grad, ref, f32):
    return R.triple(P.side_errors(slices, grad, ref.grad)), R.triple(P.side_errors(slices, f32.grad, ref.grad))


@pytest.mark.parametrize("name,dc", CASES)
@pytest.mark.parametrize("value_clip", (False, True))
def test_the_right_float32_gradient_passes_the_rule(cases, name, dc, value_clip):
    """the rows the mutations are judged on are rows on which a right float32 gradient passes: the actor's and the critic's halves of the
    loss differentiated apart, in float32, against the float64 gradient of the whole loss with float32 autograd of the whole as the yardstick"""
    p, st = cases[name, dc]
    ref, f32 = (P.loss_autograd(p, st, d, value_clip=value_clip, **KW) for d in ("float64", "float32"))
    apart = P.loss_autograd(p, st, "float32", value_clip=value_clip, separately=True, **KW)
    for slices in (P.tensor_slices(p), P.critic_slices(p), P.actor_slices(p)):
        got, yard = _triples(p, slices, apart.grad, ref, f32)
        assert R.within(got, yard), (got, yard)
    assert R.within(R.triple(R.stat_units(apart.stats[:4], ref.stats[:4])), [max(x, 1e-3) for x in R.triple(R.stat_units(f32.stats[:4], ref.stats[:4]))])


@pytest.mark.parametrize("name,dc", CASES)
@pytest.mark.parametrize("how", P.MUTATIONS)
def test_crossed_inputs_miss_the_rule_by_orders_of_magnitude(cases, name, dc, how):
    """the critic fed the actor's rows, normalised with the actor's statistics, or its first-layer dW formed from the actor's normalised
    input: on the critic's tensors the float32 gradient's error leaves 3 x the yardstick by a factor of 100 at least, at the 99th percentile
    and at the maximum (the median too where the wrong elements are the majority); the actor's tensors do not move at all"""
    p, st = cases[name, dc]
    ref, f32 = (P.loss_autograd(p, st, d, **KW) for d in ("float64", "float32"))
    bad = P.loss_autograd(p, st, "float32", mutate=how, **KW)
    got, yard = _triples(p, P.critic_slices(p), bad.grad, ref, f32)
    assert got[1] > 100 * 3 * yard[1] and got[2] > 100 * 3 * yard[2], (how, got, yard)
    for a, b in P.actor_slices(p):
        assert np.array_equal(bad.grad[a:b], f32.grad[a:b])


def test_the_loss_separates_in_float64():
    p = P.make_policy("mixed", critic_in_dim=95, norm=True, seed=3)
    st = P.make_storage(p, 50, seed=4)[0]
    whole, apart = (P.loss_autograd(p, st, "float64", value_clip=True, separately=s, **KW) for s in (False, True))
    assert np.array_equal(whole.grad, apart.grad)


def test_each_side_is_a_plain_policy_on_its_own_rows():
    """the reference's form of the bit-for-bit claim: the actor's tensors are ppo_reference's on actor_side(p) and the actor's storage, the
    critic's those on critic_side(p) and the critic's storage -- at float64 to rounding, since the plain loss adds the two halves first"""
    p = P.make_policy("tiny", in_dim=9, critic_in_dim=5, norm=True, seed=5)
    st, st_a, st_c = P.make_storage(p, 40, seed=6)
    ref = P.loss_autograd(p, st, "float64", value_clip=True, **KW)
    pa, pc = P.actor_side(p), P.critic_side(p)
    ga, gc = R.loss_autograd(pa, st_a, "float64", value_clip=True, **KW), R.loss_autograd(pc, st_c, "float64", value_clip=True, **KW)
    for (a, b), (c, d) in zip(P.actor_slices(p), P.actor_slices(pa)):
        assert np.allclose(ref.grad[a:b], ga.grad[c:d], rtol=1e-12, atol=1e-15)
    for (a, b), (c, d) in zip(P.critic_slices(p), P.critic_slices(pc)):
        assert np.allclose(ref.grad[a:b], gc.grad[c:d], rtol=1e-12, atol=1e-15)
    assert np.allclose(ref.stats[[0, 2, 3, 4]], ga.stats[[0, 2, 3, 4]], rtol=1e-12) and np.isclose(ref.stats[1], gc.stats[1], rtol=1e-12)


# ---- DevicePolicy ----

@pytest.mark.parametrize("norm", (True, False))
@pytest.mark.parametrize("dims", P.DIMS)
def test_device_policy_round_trips(tmp_path, dims, norm):
    from mocca_envs_amd.policy import DevicePolicy
    p = P.make_policy("tiny", in_dim=dims[0], critic_in_dim=dims[1], norm=norm, seed=1)
    dp = P.device_policy(p)
    assert dp.asymmetric and (dp.in_dim, dp.critic_in_dim) == dims
    flat = dp.flat_params()
    assert flat.size == dp.n_head() + (dp.n_tail() if norm else 0) and dp.n_tail() == 2 * dims[0] + 2 * dims[1]
    assert np.array_equal(flat[:dp.n_head()], R.flat_params(p))
    if norm:
        assert np.array_equal(flat[dp.n_head():], np.concatenate([p.obs_mean, p.inv_std, p.critic_obs_mean, p.critic_inv_std]))
    parts = dp.split_grad(flat)
    assert parts["critic"][0][0].shape == (16, dims[1]) and parts["actor"][0][0].shape == (16, dims[0])
    assert np.array_equal(parts["critic"][0][0], p.critic[0][0]) and np.array_equal(parts["log_std"], p.log_std)
    image, table, offsets = dp.pack()
    assert table[len(p.actor), 1] == dims[1] and table[0, 1] == dims[0]
    pad = -(-dims[1] // 16) * 16
    assert offsets["critic_mean"] == offsets["inv_std"] + -(-dims[0] // 16) * 16 and image.size == offsets["critic_inv_std"] + pad
    back = DevicePolicy.unpack(image, table, offsets)
    assert back.asymmetric and np.array_equal(back.flat_params(), flat)
    spoiled = image.copy()
    spoiled[offsets["critic_mean"] + pad - 1] = 1.0
    if dims[1] % 16:
        with pytest.raises(ValueError):
            DevicePolicy.unpack(spoiled, table, offsets)
    # the callable: the actor on obs, the critic on its own rows
    rng = np.random.default_rng(0)
    obs, cobs = rng.normal(0, 2, (7, dims[0] + 3)).astype(np.float32), rng.normal(0, 2, (7, dims[1] + 2)).astype(np.float32)
    action, logp, value, mean = dp(obs, critic_obs=cobs)
    mean64, value64 = P.forward64(p, obs[:, :dims[0]], cobs[:, :dims[1]])
    assert np.allclose(mean, mean64, atol=1e-4) and np.allclose(value, value64, atol=1e-4) and np.array_equal(action, mean)
    with pytest.raises(ValueError):
        dp(obs)
    if norm:       # save() -> from_npz(): tanh nets; inv_std survives var = 1 / inv_std^2 - eps to a few ulp
        dp.save(str(tmp_path / "p.npz"))
        again = DevicePolicy.from_npz(str(tmp_path / "p.npz"), clip=p.clip)
        assert again.asymmetric and again.critic_in_dim == dims[1]
        assert np.array_equal(again.flat_params()[:dp.n_head()], flat[:dp.n_head()])
        assert np.allclose(again.flat_params()[dp.n_head():], flat[dp.n_head():], rtol=1e-6, atol=0)


def test_from_torch_carries_the_critic_statistics():
    import policy_symmetry_reference as PS
    from mocca_envs_amd.policy import DevicePolicy
    p = P.make_policy("tiny", in_dim=5, critic_in_dim=9, norm=True, seed=2)
    import torch
    actor, critic, log_std = PS.sequentials(p, torch.float32)
    var = lambda inv: 1.0 / (inv.astype(np.float64) ** 2) - 1e-8
    dp = DevicePolicy.from_torch(actor, critic, log_std, obs_mean=p.obs_mean, obs_var=var(p.inv_std), clip=p.clip,
                                 critic_obs_mean=p.critic_obs_mean, critic_obs_var=var(p.critic_inv_std))
    assert dp.asymmetric and dp.critic_in_dim == 9 and np.array_equal(dp.critic_obs_mean, p.critic_obs_mean)
    assert np.allclose(dp.critic_inv_std, p.critic_inv_std, rtol=1e-6)


def test_statistics_come_for_both_nets_or_for_neither_and_no_mirror_tables():
    from mocca_envs_amd.policy import DevicePolicy
    p = P.make_policy("tiny", in_dim=5, critic_in_dim=9, norm=True, seed=2)
    with pytest.raises(ValueError):
        DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std)
    with pytest.raises(ValueError):
        DevicePolicy(p.actor, p.critic, p.log_std, critic_obs_mean=p.critic_obs_mean, critic_inv_std=p.critic_inv_std)
    tables = (np.arange(5), np.ones(5), np.arange(3), np.ones(3))
    with pytest.raises(ValueError):
        DevicePolicy(p.actor, p.critic, p.log_std, symmetry=tables)
    with pytest.raises(ValueError):
        P.device_policy(p).with_symmetry(tables)
    same = DevicePolicy(p.actor, P.actor_side(p).critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, critic_obs_mean=p.obs_mean,
                        critic_inv_std=p.inv_std)
    assert same.asymmetric and same.critic_in_dim == same.in_dim     # equal widths, statistics of its own: still a privileged critic


# sha256 of a plain policy's pack() image, table and flat_params(), recorded on the commit before the privileged critic existed
PLAIN_SHA = {
    ("tiny", True): "3a4fa0f7a844c2638b3e6a04927afb4796bdaca87f2ff033c8b228264e34527c",
    ("tiny", False): "37e9acc09353cf4187e4230f5ca967ccdfb6d4dabf3d56bcc2a15e3ad99ae6c1",
    ("mixed", True): "e8f38ca884de42340ceee0c5cd92f8e3f64e09a64f3687c91d8726b26cbfbdac",
}


def _plain_digest(name, norm):
    import policy_symmetry_reference as PS
    dp = PS.device_policy(R.make_policy(name, norm=norm, seed=1))
    image, table, offsets = dp.pack()
    h = hashlib.sha256()
    for part in (image, np.ascontiguousarray(table, np.int32), dp.flat_params(), np.array([offsets[k] for k in ("log_std", "flags", "mean", "inv_std")], np.int64)):
        h.update(np.ascontiguousarray(part).tobytes())
    return dp, offsets, h.hexdigest()


@pytest.mark.parametrize("name,norm", sorted(PLAIN_SHA))
def test_a_plain_policy_packs_to_the_bytes_it_always_did(name, norm):
    dp, offsets, digest = _plain_digest(name, norm)
    assert not dp.asymmetric and dp.n_tail() == 2 * dp.in_dim and "critic_mean" not in offsets
    assert digest == PLAIN_SHA[name, norm]
