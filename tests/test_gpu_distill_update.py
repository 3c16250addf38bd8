"""mocca_distill_update on the GPU (include/mocca.h): the update against a Python loop of its parts -- the checker's permutation
(tests/ppo_update_reference.py), distill_grad, adam_step --, eager and from a graph, and a regression that goes down on a fixed storage."""
import numpy as np
import pytest

import distill_reference as D
import ppo_reference as R
import ppo_update_reference as U

pytestmark = pytest.mark.gpu
KW = dict(distill_coef=1.0, value_coef=0.5)
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
N_ROWS, N_BATCH, EPOCHS, SEED = 100, 17, 2, 77      # 5 minibatches an epoch, 15 rows dropped


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


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _state(env, n_head):
    from mocca_envs_amd.rollout import AdamState
    return AdamState(n_head, env.device)


def _device(st):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in st.items()}


def _by_hand(env, d, params, state, use_value, n_calls=1):
    """`n_calls` updates as a loop of their parts -> the stats rows, with [6] the checker's clip coefficient"""
    import torch
    rows = []
    for _ in range(n_calls):
        for ep in range(EPOCHS):
            perm = U.permutation(N_ROWS, int(state.clock[0].item()), SEED)
            for u in range(N_ROWS // N_BATCH):
                idx = torch.from_numpy(perm[u * N_BATCH:(u + 1) * N_BATCH].copy()).cuda()
                out = env.distill_grad(d["obs"], d["target"], d["value_target"] if use_value else None, idx=idx, **KW)
                env.adam_step(params, out["grad"], state, **ADAM)
                row = out["stats"].cpu().numpy().copy()
                row[6] = U.clip_coef(out["grad"].cpu().numpy(), ADAM["max_grad_norm"])
                rows.append(row)
    return np.array(rows)


@pytest.mark.parametrize("name,use_value", [("tiny", True), ("mixed", False)])
def test_distill_update_is_its_parts_eager_and_from_a_graph(env, name, use_value):
    """one distill_update equals [the checker's permutation at the clock's t -> distill_grad(idx) -> adam_step] from the same start, bit
    for bit in params, moments, clock and stats ([6] the checker's clip coefficient); a graph captured after that warm call, replayed
    twice, equals two more rounds of the loop"""
    import torch
    p = R.make_policy(name, norm=True, seed=1)
    st = D.make_storage(name, p, N_ROWS, seed=2)
    dp = _dp(p)
    env.set_policy(dp)
    d, n_head, per_epoch = _device(st), dp.n_head(), N_ROWS // N_BATCH
    vt = d["value_target"] if use_value else None
    start = torch.from_numpy(dp.flat_params()).cuda()
    params, state, stats = start.clone(), _state(env, n_head), torch.full((EPOCHS * per_epoch, 8), float("nan"), device="cuda")
    call = lambda: env.distill_update(d["obs"], d["target"], params, state, N_BATCH, EPOCHS, value_target=vt, seed=SEED, stats=stats, **KW, **ADAM)
    call()
    params2, state2 = start.clone(), _state(env, n_head)
    env.update_policy(params2)
    want = _by_hand(env, d, params2, state2, use_value)
    torch.cuda.synchronize()
    assert _same(params, params2) and _same(state.moments, state2.moments) and _same(state.clock, state2.clock)
    assert state.clock.tolist()[0] == EPOCHS * per_epoch and not _same(params, start)
    assert _same(stats, want) and np.isfinite(want).all()
    a = dp.act_dim
    assert _same(params[n_head - a:n_head], start[n_head - a:n_head])      # log_std: a zero gradient moves nothing
    # from a graph: the image holds params2's weights now, which are params' bit for bit
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    graph.replay()
    first = stats.clone()
    graph.replay()
    env.update_policy(params2)
    want = _by_hand(env, d, params2, state2, use_value, n_calls=2)
    torch.cuda.synchronize()
    assert _same(params, params2) and _same(state.moments, state2.moments) and _same(state.clock, state2.clock)
    assert _same(first, want[:EPOCHS * per_epoch]) and _same(stats, want[EPOCHS * per_epoch:])
    assert state.clock.tolist()[0] == 3 * EPOCHS * per_epoch


def test_a_fixed_storage_is_learned(env):
    """1024 rows labelled by a frozen random net of the student's shape, 4 epochs x 8 minibatches: the last epoch's mean L_d lies below the
    first epoch's (how far is printed)"""
    import torch
    name = "ppo"
    p = R.make_policy(name, norm=True, seed=1)
    st = D.make_storage(name, p, 1024, seed=3)
    dp = _dp(p)
    env.set_policy(dp)
    d = _device(st)
    params, state = torch.from_numpy(dp.flat_params()).cuda(), _state(env, dp.n_head())
    stats = env.distill_update(d["obs"], d["target"], params, state, 128, 4, value_target=d["value_target"], seed=5, lr=1e-3, **KW)["stats"]
    torch.cuda.synchronize()
    l_d = stats[:, 7].cpu().numpy().reshape(4, 8).mean(1)
    print("L_d per epoch:", l_d.tolist())
    assert np.isfinite(l_d).all() and l_d[-1] < l_d[0], l_d.tolist()
