"""The device policy where it is wired into other features: the `[obs | scan]` input row of a height-scanning trainer env (eager and from a
graph), and tools/ppo_demo.py's `--device-policy` collection path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy()).reshape(-1).view(np.uint8)


def test_height_scan_row_is_the_policys_input():
    """With `height_scan=` the attached policy reads the wide row [obs | scan] (65 + 77 = 142 inputs).  A: act_step.  B, a twin: step(A's
    actions).  Wide observation, reward and done are bit-identical in each step; A's action is what act() gives for the row the step started
    from; capture_rollout() with the attached policy replays like the eager loop."""
    import torch
    from mocca_envs_amd.perception import scan_grid
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.trainer_api import make_vec_envs
    n, T = 63, 3
    hs = dict(points=scan_grid((-0.45, 1.05), (-0.45, 0.45), 11, 7), z_above=1.0, max_drop=2.0)
    make = lambda: make_vec_envs("Walker3DStepperEnv-v0", 7, n, None, height_scan=hs, record_events=False)
    A, B, G = make(), make(), make()
    od = A.observation_space.shape[0]
    assert od == 65 + 77
    ref = R.random_policy("ppo", od, 21, norm=True, seed=3)
    p = DevicePolicy(ref.actor, ref.critic, ref.log_std, obs_mean=ref.obs_mean, inv_std=ref.inv_std, clip=ref.clip)
    narrow = R.random_policy("small", 65, 21, norm=False)
    with pytest.raises(ValueError):
        A.attach_policy(DevicePolicy.from_layers(narrow.actor, narrow.critic, narrow.log_std))      # 65 inputs: not this env's row
    for e in (A, G):
        e.attach_policy(p)
    oa, ob = A.reset(), B.reset()
    G.reset()
    assert np.array_equal(_bits(oa), _bits(ob)) and float(oa[:, 65:].abs().max()) > 0
    for t in range(T):
        row = oa.clone()
        oa, ra, _, _ = A.act_step()
        act = A.last_act["action"].clone()
        want = A.venv.act(row, deterministic=True)      # (the step has moved the noise's counters: the value is what can be compared)
        assert np.array_equal(_bits(want["value"]), _bits(A.last_act["value"].reshape(-1))), t
        ob, rb, _, _ = B.step(act)
        for name, u, v in (("obs", oa, ob), ("reward", ra, rb), ("done", A.done, B.done)):
            assert np.array_equal(_bits(u), _bits(v)), (t, name)
    graph = G.capture_rollout(num_steps=T, warmup=0)      # G still holds the state after reset
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(G._wide), _bits(oa)) and np.array_equal(_bits(G.last_act["action"]), _bits(A.last_act["action"]))
    for e in (A, B, G):
        e.close()


def test_ppo_demo_collects_through_the_device_policy(tmp_path):
    """tools/ppo_demo.py --device-policy runs two whole iterations (update_policy, act_step collection, the torch update) and saves a policy
    that DevicePolicy.from_npz loads, critic included."""
    from mocca_envs_amd.policy import DevicePolicy
    out = str(tmp_path / "demo")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ppo_demo.py"), "--device-policy", "--envs", "64", "--steps", "4", "--iters", "2", "--epochs", "1",
           "--minibatches", "2", "--out", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(open(out + ".jsonl").readline())
    assert line["env_steps"] == 64 * 4 and np.isfinite(line["log_std"])
    p = DevicePolicy.from_npz(out + "_policy.npz")
    assert (p.in_dim, p.act_dim) == (52, 21) and len(p.critic) == 3 and np.abs(p.critic[0][0]).max() > 0
