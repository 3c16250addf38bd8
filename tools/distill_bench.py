#!/usr/bin/env python3
"""Timing of `mocca_distill_grad` and of what the distillation pull request could have slowed down, on one GPU: fills profiles/distill.json.
Everything here is reported; nothing is a gate.

  python tools/distill_bench.py grad   [--out profiles/distill.json]
      B = 16384 rows gathered from 131072 of the student of tools/ppo_demo.py --depth-camera 16,12, 52 + 192 -> 256 -> 256 -> {21, 1} tanh:
      `VecEnv.distill_grad` (targets and value targets given), the same loss through torch eager (forward, loss, zero_grad, backward) and
      `VecEnv.ppo_grad` on the same shape, all in one process; HIP events, 5 blocks of 200 warm calls (tools/ppo_grad_bench.py's protocol).
  python tools/distill_bench.py ab --key NAME [--package-root DIR] [--out ...]
      `ppo_grad` at 4096 rows and `act` at 4096 envs of the 52 -> 256 -> 256 -> {21, 1} policy, 7 blocks of 200 warm calls, stored under
      "ab"[NAME].  --package-root: the tree whose mocca_envs_amd (with its built library) is imported -- a checkout of the parent commit
      gives the A/B; run the two alternately, several times each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ppo_grad_bench import merge, random_net, timed  # noqa: E402

B, ROWS = 16384, 131072


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("grad", "ab"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill.json"))
    ap.add_argument("--key", default="this")
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch
    import torch.nn as nn
    import mocca_envs_amd
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.vec_env import VecEnv
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).cuda()

    def policy(in_dim):
        return DevicePolicy(random_net(rng, [in_dim, 256, 256, 21]), random_net(rng, [in_dim, 256, 256, 1]), np.full(21, -1.0, np.float32),
                            obs_mean=np.zeros(in_dim, np.float32), obs_var=np.ones(in_dim, np.float32))

    if args.mode == "ab":
        n = 4096
        env = VecEnv("Walker3DCustomEnv-v0", n, device=0)
        dp = policy(52)
        env.set_policy(dp)
        obs = env.reset()
        out = env.act(obs)
        rows, act, olp, adv, ret = f(n, 52) * 3, f(n, 21), f(n) - 20, f(n), f(n)
        grad, stats = torch.empty(dp.n_head(), device="cuda"), torch.empty(8, device="cuda")
        res = {"package": os.path.relpath(os.path.dirname(mocca_envs_amd.__file__), ROOT),
               "ppo_grad_4096_rows": timed(torch, lambda: env.ppo_grad(rows, act, olp, adv, ret, grad=grad, stats=stats), blocks=7),
               "act_4096_envs": timed(torch, lambda: env.act(obs, out=out), blocks=7)}
        doc = json.load(open(args.out)).get("ab", {}) if os.path.exists(args.out) else {}
        doc.setdefault(args.key, []).append(res)
        merge(args.out, "ab", doc)
        print(json.dumps({args.key: res}))
        env.close()
        return
    in_dim = 52 + 192
    env = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    dp = policy(in_dim)
    env.set_policy(dp)
    obs, target, vt = f(ROWS, in_dim) * 3, f(ROWS, 21), f(ROWS)
    olp, adv = f(ROWS) - 20, f(ROWS)
    idx = torch.randperm(ROWS, device="cuda")[:B]
    grad, stats = torch.empty(dp.n_head(), device="cuda"), torch.empty(8, device="cuda")
    res = {"what": f"B = {B} rows gathered from {ROWS}, policy {in_dim} -> 256 -> 256 -> {{21, 1}} tanh, HIP events, 5 blocks of 200 warm calls; "
                   "torch eager: the same regression loss, forward, zero_grad and backward; mocca_ppo_grad: PPO's loss on the same rows and shape"}
    res["mocca_distill_grad"] = timed(torch, lambda: env.distill_grad(obs, target, vt, idx=idx, grad=grad, stats=stats))
    res["mocca_ppo_grad"] = timed(torch, lambda: env.ppo_grad(obs, target, olp, adv, vt, idx=idx, grad=grad, stats=stats))
    res["mocca_distill_grad_again"] = timed(torch, lambda: env.distill_grad(obs, target, vt, idx=idx, grad=grad, stats=stats))

    def mlp(o):
        return nn.Sequential(nn.Linear(in_dim, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, o)).cuda()
    pi, vf = mlp(21), mlp(1)
    log_std = nn.Parameter(torch.full((21,), -1.0, device="cuda"))
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)
    o_all, vt_all = obs.clamp(-10, 10), vt.reshape(-1, 1)

    def eager():
        l_d = (pi(o_all[idx]) - target[idx]).pow(2).mean()
        l_v = 0.5 * (vf(o_all[idx]) - vt_all[idx]).pow(2).mean()
        opt.zero_grad(set_to_none=True)
        (l_d + 0.5 * l_v).backward()

    res["torch_eager"] = timed(torch, eager)
    res["speedup"] = round(res["torch_eager"]["us_per_call_median"] / res["mocca_distill_grad"]["us_per_call_median"], 2)
    merge(args.out, "minibatch", res)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
