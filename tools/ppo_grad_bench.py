#!/usr/bin/env python3
"""Timing of `mocca_ppo_grad` and of what it touches, on one GPU: fills profiles/ppo_grad.json.

  python tools/ppo_grad_bench.py grad   [--out profiles/ppo_grad.json]
      B = 16384 rows gathered from 131072 of the 52 -> 256 -> 256 -> {21, 1} tanh policy: `VecEnv.ppo_grad` against the same minibatch
      through torch eager as tools/ppo_demo.py's learn loop does it (forward, loss, zero_grad, backward); HIP events, 5 blocks of 200 warm calls.
  python tools/ppo_grad_bench.py grad --symmetric   [--out profiles/ppo_grad_sym.json]
      the same for the mirror-symmetric policy (the env's own mirror tables): mocca_ppo_grad_sym against the minibatch through
      `symmetry.SymmetricGaussian` in torch eager, as tools/ppo_demo.py --symmetric does it; both in one process.
  python tools/ppo_grad_bench.py grad --mirror-loss   [--out profiles/ppo_grad_mirror.json]
      the same for the plain policy with the mirror-symmetry loss attached (the env's own mirror tables, coef 4): mocca_ppo_grad_mirror
      against the plain minibatch plus `symmetry.mirror_loss` in torch eager, as tools/ppo_demo.py --mirror-loss does it; both in one process.
  python tools/ppo_grad_bench.py grad --mirror-dup   [--out profiles/ppo_grad_dup.json]
      the same for the plain policy with duplicated rows attached (the env's own mirror tables): mocca_ppo_grad_dup on the B rows against
      the plain minibatch of `symmetry.duplicate_minibatch`'s 2 B rows in torch eager, as tools/ppo_demo.py --mirror-dup does it; then, in
      the same process, mocca_ppo_grad_sym (the same layout) and the plain mocca_ppo_grad on the same rows.
  python tools/ppo_grad_bench.py act --key NAME [--package-root DIR] [--out ...]
      `update_policy` and `act` at 4096 envs, 7 blocks of 200 warm calls, stored under "act_update"[NAME].  --package-root: the tree whose
      mocca_envs_amd (with its built library) is imported -- a checkout of the parent commit gives the A/B; run the two alternately.
  rocprofv3 --kernel-trace -d DIR -o ppo -- python tools/ppo_grad_bench.py trace        (30 calls, nothing written)
  python tools/ppo_grad_bench.py per-launch --kernel-db DIR/ppo_results.db [--out ...]
      medians of the four launches' durations in that trace, stored under "per_launch_us_kernel_trace".
Each mode merges its figures into the json; nothing else is touched."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, ROWS = 16384, 131072


def merge(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def timed(torch, fn, reps=200, blocks=5, warm=30):
    import numpy as np
    for _ in range(warm):
        fn()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b) * 1e3 / reps, 2))
    return {"us_per_call_blocks": out, "us_per_call_median": round(float(np.median(out)), 2)}


def random_net(rng, dims):
    import numpy as np
    return [(rng.normal(0, 1 / np.sqrt(i), (o, i)).astype(np.float32), rng.normal(0, 0.1, o).astype(np.float32),
             "tanh" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("grad", "act", "trace", "per-launch"))
    ap.add_argument("--out")
    ap.add_argument("--symmetric", action="store_true", help="grad: the mirror-symmetric policy (mocca_ppo_grad_sym against SymmetricGaussian)")
    ap.add_argument("--mirror-loss", action="store_true", help="grad: the mirror-symmetry loss (mocca_ppo_grad_mirror against symmetry.mirror_loss)")
    ap.add_argument("--mirror-dup", action="store_true", help="grad: duplicated rows (mocca_ppo_grad_dup against symmetry.duplicate_minibatch's 2 B rows)")
    ap.add_argument("--key", default="this")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--kernel-db")
    args = ap.parse_args()
    if (args.symmetric or args.mirror_loss or args.mirror_dup) and args.mode != "grad":
        ap.error("--symmetric, --mirror-loss and --mirror-dup go with the grad mode")
    if args.symmetric + args.mirror_loss + args.mirror_dup > 1:
        ap.error("--symmetric, --mirror-loss or --mirror-dup, one of them")
    args.out = args.out or os.path.join(ROOT, "profiles", "ppo_grad_sym.json" if args.symmetric else "ppo_grad_mirror.json" if args.mirror_loss
                                        else "ppo_grad_dup.json" if args.mirror_dup else "ppo_grad.json")
    if args.mode == "per-launch":
        import sqlite3
        import statistics
        rows = sqlite3.connect(args.kernel_db).execute("select name, duration from kernels where name like '%mocca_ppo%'").fetchall()
        by = {}
        for name, ns in rows:
            by.setdefault(name.split("(")[0].split("::")[-1], []).append(ns)
        merge(args.out, "per_launch_us_kernel_trace", {"what": "median duration of each launch in a rocprofv3 kernel trace of 30 calls at B = 16384 "
              "(the profiler adds to every launch; the HIP-event total is the figure to compare)",
              **{k: {"median": round(statistics.median(v) / 1e3, 2), "calls": len(v)} for k, v in sorted(by.items())}})
        return
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch
    import torch.nn as nn
    import mocca_envs_amd
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.vec_env import VecEnv
    rng = np.random.default_rng(0)
    dp = DevicePolicy(random_net(rng, [52, 256, 256, 21]), random_net(rng, [52, 256, 256, 1]), np.full(21, -1.0, np.float32),
                      obs_mean=np.zeros(52, np.float32), obs_var=np.ones(52, np.float32))
    if args.mode == "act":
        env = VecEnv("Walker3DCustomEnv-v0", 4096, device=0)
        env.set_policy(dp)
        obs = env.reset()
        flat = torch.from_numpy(dp.flat_params()).cuda()
        out = env.act(obs)
        res = {"package": os.path.relpath(os.path.dirname(mocca_envs_amd.__file__), ROOT),
               "update_policy": timed(torch, lambda: env.update_policy(flat), blocks=7), "act_4096_envs": timed(torch, lambda: env.act(obs, out=out), blocks=7)}
        doc = json.load(open(args.out)).get("act_update", {}) if os.path.exists(args.out) else {}
        doc[args.key] = res
        merge(args.out, "act_update", doc)
        print(json.dumps({args.key: res}))
        env.close()
        return
    env = VecEnv("Walker3DCustomEnv-v0", 4, device=0)
    if args.symmetric:
        dp = env.symmetric_policy(dp)
    env.set_policy(dp)
    if args.mirror_loss:
        env.set_policy_mirror_loss(env.policy_mirror_tables(dp), 4.0)
    if args.mirror_dup:
        env.set_policy_mirror_dup(env.policy_mirror_tables(dp))
    f = lambda *s: torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)).cuda()
    obs, act, olp, adv, ret = f(ROWS, 52) * 3, f(ROWS, 21), f(ROWS) - 20, f(ROWS), f(ROWS)
    idx = torch.randperm(ROWS, device="cuda")[:B]
    grad, stats = torch.empty(dp.n_head(), device="cuda"), torch.empty(8, device="cuda")
    call = lambda: env.ppo_grad(obs, act, olp, adv, ret, idx=idx, grad=grad, stats=stats)
    if args.mode == "trace":
        for _ in range(30):
            call()
        torch.cuda.synchronize()
        env.close()
        return
    res = {"what": f"B = {B} rows gathered from {ROWS}, policy 52 -> 256 -> 256 -> {{21, 1}} tanh, HIP events, 5 blocks of 200 warm calls"}
    name = "mocca_ppo_grad_sym" if args.symmetric else "mocca_ppo_grad_mirror" if args.mirror_loss else "mocca_ppo_grad_dup" if args.mirror_dup else "mocca_ppo_grad"
    if args.mirror_dup:
        res["what"] += ("; the plain policy on the B rows and their B mirror images (the env's mirror tables), torch eager on "
                        "symmetry.duplicate_minibatch's 2 B rows; mocca_ppo_grad_sym and mocca_ppo_grad on the same B rows in the same process")
    if args.mirror_loss:
        res["what"] += "; the plain policy with the mirror-symmetry loss of the env's mirror tables at coef 4, torch eager through symmetry.mirror_loss"
    if args.symmetric:
        res["what"] += "; the mirror-symmetric policy of the env's mirror tables, torch eager through symmetry.SymmetricGaussian"
    res[name] = timed(torch, call)
    if args.mirror_dup:      # the same layout, and the plain call, in this process
        env.set_policy_mirror_dup(None)
        env.set_policy_symmetry(env.policy_mirror_tables(dp))
        res["mocca_ppo_grad_sym"] = timed(torch, call)
        env.set_policy_symmetry(None)
        res["mocca_ppo_grad"] = timed(torch, call)

    def mlp(o):
        return nn.Sequential(nn.Linear(52, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, o)).cuda()
    pi, vf = mlp(21), mlp(1)
    log_std = nn.Parameter(torch.full((21,), -1.0, device="cuda"))
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)
    o_all = obs.clamp(-10, 10)
    lp_all, adv_all, ret_all = olp.reshape(-1, 1), adv.reshape(-1, 1), ret.reshape(-1, 1)
    logprob = lambda mu, a: (-0.5 * ((a - mu) / log_std.exp()) ** 2 - log_std - 0.9189385332046727).sum(-1, keepdim=True)

    if args.symmetric:
        from mocca_envs_amd.symmetry import SymmetricGaussian
        sym = SymmetricGaussian(pi, vf, log_std, dp.symmetry).cuda()
        zero, one = torch.zeros(52, device="cuda"), torch.ones(52, device="cuda")

    def eager_sym():
        logp, _, value = sym.evaluate_actions(obs[idx], act[idx], zero, one, 10.0)
        ratio = (logp.unsqueeze(-1) - lp_all[idx]).exp()
        surr = torch.min(ratio * adv_all[idx], ratio.clamp(0.8, 1.2) * adv_all[idx]).mean()
        v_loss = 0.5 * (value.unsqueeze(-1) - ret_all[idx]).pow(2).mean()
        opt.zero_grad(set_to_none=True)
        (-surr + 0.5 * v_loss).backward()

    if args.mirror_loss:
        from mocca_envs_amd.symmetry import MirrorTransform, mirror_loss
        tf = MirrorTransform(env.get_mirror_indices(), 52, 21, device="cuda")

    def eager_mirror():
        mu = pi(o_all[idx])
        ratio = (logprob(mu, act[idx]) - lp_all[idx]).exp()
        surr = torch.min(ratio * adv_all[idx], ratio.clamp(0.8, 1.2) * adv_all[idx]).mean()
        v_loss = 0.5 * (vf(o_all[idx]) - ret_all[idx]).pow(2).mean()
        l_m = mirror_loss(lambda x: pi(x.clamp(-10, 10)), obs[idx], tf)
        opt.zero_grad(set_to_none=True)
        (-surr + 0.5 * v_loss + 4.0 * l_m).backward()

    if args.mirror_dup:
        from mocca_envs_amd.symmetry import MirrorTransform, duplicate_minibatch
        tf = MirrorTransform(env.get_mirror_indices(), 52, 21, device="cuda")

    def eager_dup():
        o2, a2, lp2, adv2, ret2, _ = duplicate_minibatch(obs[idx], act[idx], lp_all[idx], adv_all[idx], ret_all[idx], None, tf)
        o2 = o2.clamp(-10, 10)
        ratio = (logprob(pi(o2), a2) - lp2).exp()
        surr = torch.min(ratio * adv2, ratio.clamp(0.8, 1.2) * adv2).mean()
        v_loss = 0.5 * (vf(o2) - ret2).pow(2).mean()
        opt.zero_grad(set_to_none=True)
        (-surr + 0.5 * v_loss).backward()

    def eager():
        mu = pi(o_all[idx])
        ratio = (logprob(mu, act[idx]) - lp_all[idx]).exp()
        surr = torch.min(ratio * adv_all[idx], ratio.clamp(0.8, 1.2) * adv_all[idx]).mean()
        v_loss = 0.5 * (vf(o_all[idx]) - ret_all[idx]).pow(2).mean()
        opt.zero_grad(set_to_none=True)
        (-surr + 0.5 * v_loss).backward()

    res["torch_eager"] = timed(torch, eager_sym if args.symmetric else eager_mirror if args.mirror_loss else eager_dup if args.mirror_dup else eager)
    res["speedup"] = round(res["torch_eager"]["us_per_call_median"] / res[name]["us_per_call_median"], 2)
    merge(args.out, "minibatch", res)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
