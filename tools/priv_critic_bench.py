#!/usr/bin/env python3
"""Timing of PPO with a privileged critic on one GPU, and the check that the plain calls did not move: fills profiles/priv_critic.json.

  python tools/priv_critic_bench.py ab --key NAME [--package-root DIR]
      plain `mocca_ppo_grad` at B = 16384 (tools/ppo_grad_bench.py's minibatch, the 52 -> 256 -> 256 -> {21, 1} policy) and `mocca_act` at 4096
      envs, HIP events, 5 blocks of 200 warm calls; appended to "ab"[NAME].  --package-root: the tree whose mocca_envs_amd (with its built
      library) is imported -- a checkout of the parent commit gives the A/B; run the two alternately in one session.
  python tools/priv_critic_bench.py verdict
      "no_regression": for each of the two calls, do NAME = "this"'s block medians lie inside the spread of "parent"'s own blocks, and at
      or below their maximum?
  python tools/priv_critic_bench.py cost
      `mocca_ppo_grad_priv` at the 244 -> 256 -> 256 -> {21, 1} actor (the [obs | 16 x 12 depth] row) with a 95 -> 256 -> 256 -> 1 critic (the
      [obs | 6 x 5 scan] row) against plain `mocca_ppo_grad` at 244 for both nets, and the same two losses through torch eager, all in one
      process; `mocca_act` at 4096 envs for both policies.
Each mode merges its figures into the json; nothing else is touched."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ppo_grad_bench import B, ROWS, merge, random_net, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("ab", "verdict", "cost"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priv_critic.json"))
    ap.add_argument("--key", default="this")
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.mode == "verdict":
        ab, res = doc["ab"], {"rule": "pass: this build's median of every round lies inside [min, max] of the parent's own blocks of the session; "
                                       "not_slower: at or below the parent's maximum"}
        for call in ("mocca_ppo_grad_16384_rows", "mocca_act_4096_envs"):
            blocks = [x for r in ab["parent"] for x in r[call]["us_per_call_blocks"]]
            med = [r[call]["us_per_call_median"] for r in ab["this"]]
            res[call] = {"parent_blocks_min_max": [min(blocks), max(blocks)], "parent_medians": [r[call]["us_per_call_median"] for r in ab["parent"]],
                         "this_medians": med, "inside": all(min(blocks) <= m <= max(blocks) for m in med), "not_slower": all(m <= max(blocks) for m in med)}
        merge(args.out, "no_regression", res)
        print(json.dumps(res))
        return
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch
    import torch.nn as nn
    import mocca_envs_amd
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.vec_env import VecEnv
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).cuda()

    def policy(in_dim, critic_in_dim):
        stats = lambda d: dict(zip(("mean", "var"), (np.zeros(d, np.float32), np.ones(d, np.float32))))
        kw = {}
        if critic_in_dim != in_dim:
            kw = dict(critic_obs_mean=stats(critic_in_dim)["mean"], critic_obs_var=stats(critic_in_dim)["var"])
        return DevicePolicy(random_net(rng, [in_dim, 256, 256, 21]), random_net(rng, [critic_in_dim, 256, 256, 1]), np.full(21, -1.0, np.float32),
                            obs_mean=stats(in_dim)["mean"], obs_var=stats(in_dim)["var"], **kw)

    def grad_call(env, dp, obs, cobs=None):
        act, olp, adv, ret = f(ROWS, 21), f(ROWS) - 20, f(ROWS), f(ROWS)
        idx = torch.randperm(ROWS, device="cuda")[:B]
        grad, stats = torch.empty(dp.n_head(), device="cuda"), torch.empty(8, device="cuda")
        kw = {} if cobs is None else {"critic_obs": cobs}
        return lambda: env.ppo_grad(obs, act, olp, adv, ret, idx=idx, grad=grad, stats=stats, **kw), (act, olp, adv, ret, idx)

    if args.mode == "ab":
        dp = policy(52, 52)
        env = VecEnv("Walker3DCustomEnv-v0", 4096, device=0)
        env.set_policy(dp)
        obs = env.reset()
        out = env.act(obs)
        call, _ = grad_call(env, dp, f(ROWS, 52) * 3)
        own = os.path.samefile(os.path.dirname(os.path.dirname(mocca_envs_amd.__file__)), ROOT)      # which build ran, not where it lay
        res = {"package": "this tree's" if own else "--package-root's", "mocca_ppo_grad_16384_rows": timed(torch, call),
               "mocca_act_4096_envs": timed(torch, lambda: env.act(obs, out=out))}
        ab = doc.get("ab", {"what": f"plain mocca_ppo_grad at B = {B} rows gathered from {ROWS} (52 -> 256 -> 256 -> {{21, 1}} tanh) and mocca_act at 4096 "
                                    "envs, HIP events, 5 blocks of 200 warm calls per round; parent build and this build alternating in one session"})
        ab.setdefault(args.key, []).append(res)
        merge(args.out, "ab", ab)
        print(json.dumps({args.key: res}))
        env.close()
        return

    env = VecEnv("Walker3DCustomEnv-v0", 4096, device=0)
    res = {"what": f"B = {B} rows gathered from {ROWS}; actor 244 -> 256 -> 256 -> 21, critic 95 -> 256 -> 256 -> 1 on its own rows (mocca_ppo_grad_priv) "
                   "against both nets on the 244-wide rows (mocca_ppo_grad); the same two losses through torch eager (forward, loss, zero_grad, "
                   "backward); mocca_act at 4096 envs for both; HIP events, 5 blocks of 200 warm calls, one process"}
    obs, cobs = f(ROWS, 244) * 3, f(ROWS, 95) * 3
    plain, priv = policy(244, 244), policy(244, 95)
    env.set_policy(plain)
    call, data = grad_call(env, plain, obs)
    res["mocca_ppo_grad_244_244"] = timed(torch, call)
    rows, crow = obs[:4096].contiguous(), cobs[:4096].contiguous()
    out = env.act(rows)
    res["mocca_act_244_244"] = timed(torch, lambda: env.act(rows, out=out))
    env.set_policy(priv)
    env.set_critic_rows(crow)
    call, _ = grad_call(env, priv, obs, cobs)
    res["mocca_ppo_grad_priv_244_95"] = timed(torch, call)
    res["mocca_act_priv_244_95"] = timed(torch, lambda: env.act(rows, out=out))
    act, olp, adv, ret, idx = data

    def mlp(i, o):
        return nn.Sequential(nn.Linear(i, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, o)).cuda()
    log_std = nn.Parameter(torch.full((21,), -1.0, device="cuda"))
    lp_all, adv_all, ret_all = olp.reshape(-1, 1), adv.reshape(-1, 1), ret.reshape(-1, 1)
    logprob = lambda mu, a: (-0.5 * ((a - mu) / log_std.exp()) ** 2 - log_std - 0.9189385332046727).sum(-1, keepdim=True)
    for key, c_all in (("torch_eager_244_244", obs.clamp(-10, 10)), ("torch_eager_priv_244_95", cobs.clamp(-10, 10))):
        pi, vf = mlp(244, 21), mlp(c_all.shape[1], 1)
        opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)
        o_all = obs.clamp(-10, 10)

        def eager():
            ratio = (logprob(pi(o_all[idx]), act[idx]) - lp_all[idx]).exp()
            surr = torch.min(ratio * adv_all[idx], ratio.clamp(0.8, 1.2) * adv_all[idx]).mean()
            v_loss = 0.5 * (vf(c_all[idx]) - ret_all[idx]).pow(2).mean()
            opt.zero_grad(set_to_none=True)
            (-surr + 0.5 * v_loss).backward()
        res[key] = timed(torch, eager)
    m = lambda k: res[k]["us_per_call_median"]
    res["priv_over_plain"] = round(m("mocca_ppo_grad_priv_244_95") / m("mocca_ppo_grad_244_244"), 4)
    res["speedup_over_torch_eager"] = round(m("torch_eager_priv_244_95") / m("mocca_ppo_grad_priv_244_95"), 2)
    merge(args.out, "cost", res)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
