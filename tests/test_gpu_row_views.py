"""The row-view rule on the device (rollout.row_view): a sensor call that writes into a view of wider storage writes the same bits as into
a contiguous tensor and leaves the floats of a row beyond its width alone.  One env is the shape at which the single-row stride rule can
go wrong (the stride handed on is never used to index, only checked); three envs are the smallest batch with a real row stride."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL, SPARE = -12345.0, 5


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [1, 3])
def test_a_view_of_wider_storage_gets_the_same_bits(n):
    from mocca_envs_amd.history import History
    from mocca_envs_amd.randomisation import Randomisation
    from mocca_envs_amd.vec_env import VecEnv
    env = VecEnv("Walker2DCustomEnv-v0", n, auto_reset=True, seed=3)
    env.set_height_scan([[0.0, 0.0], [0.3, 0.0], [0.6, 0.1]])
    env.set_history(History(2))
    env.set_randomisation(Randomisation(strength=(0.7, 1.0), latency=(0, 2), obs_noise=0.05))
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = env.reset()
    for _ in range(2):
        act = torch.rand(n, env.act_dim, generator=g, device="cuda") * 2 - 1
        obs = env.step(act)[0]
    obs = obs.clone()

    def wider(t):
        """`t`'s values as a view of storage SPARE floats wider, the rest the sentinel"""
        store = torch.full((n, t.shape[1] + SPARE), SENTINEL, dtype=torch.float32, device="cuda")
        store[:, :t.shape[1]].copy_(t)
        return store, store[:, :t.shape[1]]

    def out_of(width):
        return wider(torch.full((n, width), SENTINEL, dtype=torch.float32, device="cuda"))

    d, p, h = env.obs_dim, env.scan_dim, env.history_dim
    assert (p, h) == (3, 2 * (d + env.act_dim))
    calls = {   # name -> (width written, the call into a contiguous tensor, the same call into -- and, where it reads rows, from -- views)
        "height_scan": (p, lambda: env.height_scan(), lambda out: env.height_scan(out=out)),
        "height_scan(obs)": (d + p, lambda: env.height_scan(obs=obs), lambda out: env.height_scan(out=out, obs=obs)),
        "sensor_noise": (d, lambda: env.sensor_noise(obs, out=torch.empty_like(obs)), lambda out: env.sensor_noise(wider(obs)[1], out=out)),
        "randomisation_record": (4, lambda: env.randomisation_record(), lambda out: env.randomisation_record(out=out)),
        "history": (h, lambda: env.history(obs, act), lambda out: env.history(wider(obs)[1], wider(act)[1], out=out)),
    }
    for name, (width, plain, viewed) in calls.items():
        want = plain()
        assert want.shape == (n, width) and want.is_contiguous(), name
        store, view = out_of(width)
        got = viewed(view)
        torch.cuda.synchronize()
        assert got.shape == (n, width) and got.data_ptr() == store.data_ptr(), name
        assert torch.equal(_bits(got), _bits(want)), name                                  # the same bits
        assert bool((store[:, width:] == SENTINEL).all()), name                            # and nothing beyond the width
        assert not bool((want == SENTINEL).any()), name                                    # (the call wrote every column it owns)
    env.close()
