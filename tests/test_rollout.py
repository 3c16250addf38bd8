"""The end of a PPO rollout, the parts that need no GPU: the numpy references of mocca_gae / mocca_obs_stats against the demo's torch loop and
closed forms, `rollout.ObsStats`' host update, the Python layer's argument checks, the binding."""
import numpy as np
import pytest

import rollout_reference as R


def _bits(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("gamma,lam,scale", [(0.99, 0.95, 0.1), (1.0, 1.0, 1.0), (0.0, 0.95, 1.0), (0.99, 0.0, 1.0)])
def test_gae_f32_is_the_demos_torch_loop_bit_for_bit(gamma, lam, scale):
    """every operation of tools/ppo_demo.py's loop is one float32 torch kernel: the float32 restatement has the same bits"""
    import torch
    T, N = 11, 37
    rew, value, m, bm = R.storage(np.random.default_rng(5), T, N)
    S = {k: torch.from_numpy(v).unsqueeze(-1) for k, v in (("reward", rew), ("value", value), ("masks", m), ("bad_masks", bm))}
    adv_t, ret_t = R.torch_gae_loop(S, T, N, gamma, lam, scale)
    adv, ret = R.gae_f32(rew, value, m, bm, gamma, lam, scale)
    assert np.array_equal(_bits(adv), _bits(adv_t.numpy())) and np.array_equal(_bits(ret), _bits(ret_t.numpy()))
    assert np.abs(adv).max() > 0


def test_gae_f64_closed_forms():
    T, N, g, lam = 9, 3, 0.9, 0.8
    ones, zeros = np.ones((T + 1, N)), np.zeros((T + 1, N))
    # constant reward, value 0, no dones: adv[t] = sum_{k < T - t} (g lam)^k, the geometric series
    adv, ret = R.gae_f64(np.ones((T, N)), zeros, ones, ones, g, lam)
    q = g * lam
    want = np.array([(1 - q ** (T - t)) / (1 - q) for t in range(T)])
    assert np.allclose(adv, want[:, None], rtol=1e-13, atol=0) and np.allclose(ret, adv)
    rng = np.random.default_rng(0)
    rew, value = rng.standard_normal((T, N)), rng.standard_normal((T + 1, N))
    # lam = 0: one-step TD
    adv, ret = R.gae_f64(rew, value, ones, ones, g, 0.0, 0.5)
    assert np.allclose(adv, 0.5 * rew + g * value[1:] - value[:-1], rtol=1e-13, atol=1e-15) and np.allclose(ret, adv + value[:-1], rtol=1e-13)
    # m[t + 1] = 0 cuts the chain: steps <= t do not see anything later, step t does not bootstrap
    m = ones.copy(); m[5] = 0.0
    adv, _ = R.gae_f64(rew, value, m, ones, g, lam)
    head, _ = R.gae_f64(rew[:5], np.concatenate([value[:5], np.zeros((1, N))]), ones[:6], ones[:6], g, lam)
    tail, _ = R.gae_f64(rew[5:], value[5:], ones[:T - 4], ones[:T - 4], g, lam)
    assert np.allclose(adv[:5], head, rtol=1e-13, atol=1e-15) and np.allclose(adv[5:], tail, rtol=1e-13, atol=1e-15)
    # bm[t + 1] = 0 zeroes adv[t] and everything that would flow through it
    b = ones.copy(); b[5] = 0.0
    adv, ret = R.gae_f64(rew, value, ones, b, g, lam)
    head, _ = R.gae_f64(rew[:4], value[:5], ones[:5], ones[:5], g, 0.0)      # the last step before the cut sees only its own delta ...
    assert np.all(adv[4] == 0.0) and np.all(ret[4] == value[4]) and np.allclose(adv[3], head[3], rtol=1e-13, atol=1e-15)
    full, _ = R.gae_f64(rew, value, ones, ones, g, lam)
    assert np.allclose(adv[5:], full[5:], rtol=0, atol=0) and not np.allclose(adv[3], full[3])


@pytest.mark.parametrize("n_rows,dim", [(1, 1), (63, 52), (500, 7)])
@pytest.mark.parametrize("chunks", [1, 3, 7])
def test_obs_stats_update_in_chunks_is_the_one_shot_statistics(n_rows, dim, chunks):
    """ObsStats.update over 1, 3 or 7 chunks against obs_stats_f64 (two-pass, unshifted) of the concatenation from the fresh state.  The bound:
    the summation bound of the concatenation (rollout_reference.obs_stats_bound: n u mean|d| and n u mean(d^2), times 4), plus, because the
    chunked run CARRIES its state through `chunks` merges where the one-shot run merges once, the roundings of the carried terms: each merge
    rounds mean + delta n / tot and (var count + ...) / tot in at most 4 operations on numbers no larger than the result, 4 u |result| per
    merge.  (For the all-zero feature the summation bound is exactly 0 and that second term is all there is.)"""
    from mocca_envs_amd.rollout import ObsStats, initial_state
    rng = np.random.default_rng(3)
    total = n_rows * chunks
    x = R.obs_rows(rng, total, dim, dim + 2, 0)
    st = ObsStats(dim)
    assert float(st.count) == 1e-4 and np.all(st.mean.numpy() == 0) and np.all(st.var.numpy() == 1)
    for c in np.array_split(np.arange(total), chunks):
        st.update(x[c])
    want = R.obs_stats_f64(initial_state(dim), x, dim)
    bm, bv = R.obs_stats_bound(initial_state(dim), x, dim)
    bm, bv = bm + chunks * 4 * R.U64 * np.abs(want[1:1 + dim]), bv + chunks * 4 * R.U64 * np.abs(want[1 + dim:])
    got = st.state.numpy()
    assert abs(got[0] - want[0]) <= chunks * R.U64 * want[0]      # the count: one rounded addition per chunk
    assert np.all(np.abs(got[1:1 + dim] - want[1:1 + dim]) <= bm), np.abs(got[1:1 + dim] - want[1:1 + dim]) / np.maximum(bm, 1e-300)
    assert np.all(np.abs(got[1 + dim:] - want[1 + dim:]) <= bv), np.abs(got[1 + dim:] - want[1 + dim:]) / np.maximum(bv, 1e-300)
    mean, inv_std = st.normalisation()
    assert mean.dtype == np.float32 and np.array_equal(inv_std, np.float32(1) / np.sqrt(got[1 + dim:].astype(np.float32) + np.float32(1e-8)))
    st.reset()
    assert np.array_equal(st.state.numpy(), initial_state(dim))
    st.update(torch_rows(x))      # a tensor will do
    assert st.state.numpy()[0] == want[0]


def torch_rows(x):
    import torch
    return torch.from_numpy(x)


def test_python_layer_checks_its_arguments():
    import torch
    from mocca_envs_amd import rollout as ro
    cpu, T, N = torch.device("cpu"), 4, 6
    z = lambda *s, **kw: torch.zeros(*s, **kw)
    ok = dict(n_envs=N, device=cpu, reward=z(T, N, 1), value=z(T + 1, N, 1), masks=z(T + 1, N), bad_masks=z(T + 1, N, 1), gamma=0.99, lam=0.95,
              reward_scale=1.0, returns=None, adv=z(T, N), normalise=True, adv_eps=1e-8)
    assert ro.gae_args(**ok) == T
    for bad in (dict(reward=z(T, N + 1)), dict(reward=z(T, N).double()), dict(value=z(T, N, 1)), dict(masks=z(T + 1, N, 2)),
                dict(bad_masks=z(T + 1, 2 * N)[:, ::2]), dict(adv=z(T + 1, N)), dict(returns=z(T, N, dtype=torch.float64)), dict(gamma=float("nan")),
                dict(lam=float("inf")), dict(reward_scale=float("nan")), dict(adv_eps=-1.0), dict(adv_eps=float("inf")), dict(reward=z(0, N)),
                dict(reward=np.zeros((T, N), np.float32))):
        with pytest.raises(ValueError):
            ro.gae_args(**dict(ok, **bad))
    with pytest.raises(ValueError):
        ro.gae_args(**dict(ok, n_envs=1, reward=z(1, 1), value=z(2, 1), masks=z(2, 1), bad_masks=z(2, 1), adv=None))      # one advantage has no std
    assert ro.gae_args(**dict(ok, n_envs=1, reward=z(1, 1), value=z(2, 1), masks=z(2, 1), bad_masks=z(2, 1), adv=None, normalise=False)) == 1
    # rows of the statistics: [..., >= dim], contiguous last dimension, one stride between rows
    obs = z(T + 1, N, 10)
    assert ro.rows_2d(obs[1:], 10) == (T * N, 10) and ro.rows_2d(obs[1:], 7) == (T * N, 10) and ro.rows_2d(obs[0, 0], 10) == (1, 10)
    assert ro.rows_2d(obs[:, :, :8], 8) == ((T + 1) * N, 10) and ro.rows_2d(obs[2:3, 1:4], 10) == (3, 10)
    for bad in (obs[:, :3], obs[:, :, ::2], obs.double(), obs[:0]):
        with pytest.raises(ValueError):
            ro.rows_2d(bad, 5)
    with pytest.raises(ValueError):
        ro.rows_2d(obs, 11)
    with pytest.raises(ValueError):
        ro.stats_out("mean_out", z(9), 10, cpu)
    for bad in (dict(dim=0), dict(dim=337), dict(dim=4, eps=-1.0)):
        with pytest.raises(ValueError):
            ro.ObsStats(**bad)


def test_binding_lists_the_rollout_entry_points():
    from mocca_envs_amd import lib
    assert len(lib.SYMBOLS["mocca_gae"][1]) == 15 and len(lib.SYMBOLS["mocca_obs_stats"][1]) == 10
    from mocca_envs_amd.trainer_api import TorchVecEnv
    from mocca_envs_amd.vec_env import VecEnv
    for cls in (VecEnv, TorchVecEnv):
        assert callable(cls.finish_rollout) and callable(cls.update_obs_stats)
