#!/usr/bin/env python3
"""Timing of one whole PPO update on one GPU, three ways: fills profiles/ppo_update.json.

  python tools/ppo_update_bench.py update   [--out profiles/ppo_update.json]
      tools/ppo_demo.py's default shapes -- 4096 envs x 32 steps = 131072 rollout rows collected with the policy kernel, 4 epochs of 8
      minibatches of 16384 rows, the 52 -> 256 -> 256 -> {21, 1} tanh policy -- and one full update per call:
        (a) "python_loop": the path before mocca_ppo_update, written out here: torch.randperm per epoch; per minibatch `ppo_grad`, the
            global-norm clip in torch from stats[5], torch.optim.Adam on the flat parameter, `update_policy`;
        (b) "ppo_update": `VecEnv.ppo_update`, eager;
        (c) "ppo_update_graph": the same call replayed from a graph captured after one warm call.
      Every call starts from the same parameters (one copy_ ahead of each, in all three); HIP events, 5 blocks of 10 updates.
  rocprofv3 --kernel-trace --stats -d DIR -o upd -- python tools/ppo_update_bench.py trace        (3 updates, nothing written)
  python tools/ppo_update_bench.py per-launch --kernel-db DIR/upd_results.db [--out ...]
      medians of every launch's duration in that trace, stored under "per_launch_us_kernel_trace".
Each mode merges its figures into the json; nothing else is touched."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, EPOCHS, MINIBATCHES = 4096, 32, 4, 8


def merge(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def timed(torch, fn, reps=10, blocks=5, warm=3):
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
        out.append(round(a.elapsed_time(b) * 1e3 / reps, 1))
    return {"us_per_update_blocks": out, "us_per_update_median": round(float(np.median(out)), 1)}


def random_net(rng, dims, gain):
    import numpy as np
    return [(rng.normal(0, (gain if k == len(dims) - 2 else 1.0) / np.sqrt(i), (o, i)).astype(np.float32), np.zeros(o, np.float32),
             "tanh" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("update", "trace", "per-launch"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update.json"))
    ap.add_argument("--kernel-db")
    args = ap.parse_args()
    if args.mode == "per-launch":
        import sqlite3
        import statistics
        rows = sqlite3.connect(args.kernel_db).execute("select name, duration from kernels where name like '%mocca_%'").fetchall()
        by = {}
        for name, ns in rows:
            by.setdefault(name.split("(")[0].split("::")[-1].split("<")[0], []).append(ns)
        merge(args.out, "per_launch_us_kernel_trace", {"what": f"median duration of each launch in a rocprofv3 kernel trace of 3 updates of {EPOCHS} x "
              f"{MINIBATCHES} minibatches of {N * T // MINIBATCHES} rows (the profiler adds to every launch; the HIP-event totals are the figures to compare)",
              **{k: {"median": round(statistics.median(v) / 1e3, 2), "calls": len(v)} for k, v in sorted(by.items())}})
        return
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.rollout import AdamState
    from mocca_envs_amd.vec_env import VecEnv
    rng = np.random.default_rng(0)
    dp = DevicePolicy(random_net(rng, [52, 256, 256, 21], 0.01), random_net(rng, [52, 256, 256, 1], 1.0), np.full(21, -1.0, np.float32),
                      obs_mean=np.zeros(52, np.float32), obs_var=np.ones(52, np.float32))
    env = VecEnv("Walker3DCustomEnv-v0", N, device=0)
    env.set_policy(dp)
    f32 = dict(dtype=torch.float32, device="cuda")
    obs, act, logp = torch.zeros(T + 1, N, env.obs_dim, **f32), torch.zeros(T, N, dp.act_dim, **f32), torch.zeros(T, N, **f32)
    value, rew = torch.zeros(T, N, **f32), torch.zeros(T, N, **f32)
    obs[0].copy_(env.reset())
    for t in range(T):      # a real rollout: the stored log-probabilities are the policy's own, the ratios start at 1
        env.act_step(obs[t], action_out=act[t], logp_out=logp[t], value_out=value[t], obs_out=obs[t + 1], rew_out=rew[t])
    adv = torch.randn(T, N, **f32)
    ret = value + 0.5 * torch.randn(T, N, **f32)
    rows, n_head = N * T, dp.n_head()
    start = torch.from_numpy(dp.flat_params()).cuda()
    flat, state = start.clone(), AdamState(n_head, env.device)
    stats = torch.zeros(EPOCHS * MINIBATCHES, 8, **f32)

    def device_update():
        with torch.no_grad():
            flat.copy_(start)
        env.ppo_update(obs[:T], act, logp, adv, ret, flat, state, rows // MINIBATCHES, EPOCHS, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=1, stats=stats)

    if args.mode == "trace":
        for _ in range(3):
            device_update()
        torch.cuda.synchronize()
        env.close()
        return
    res = {"what": f"one PPO update: {rows} rollout rows, {EPOCHS} epochs x {MINIBATCHES} minibatches of {rows // MINIBATCHES}, policy 52 -> 256 -> 256 "
                   "-> {21, 1} tanh; HIP events, 5 blocks of 10 updates, every update from the same parameters"}
    w_flat = flat[:n_head].requires_grad_()
    opt = torch.optim.Adam([w_flat], lr=3e-4, eps=1e-5)
    g_buf, s_buf = torch.zeros(n_head, **f32), torch.zeros(8, **f32)

    def python_loop():
        with torch.no_grad():
            flat.copy_(start)
        for _ in range(EPOCHS):
            perm = torch.randperm(rows, device="cuda")
            for mb in perm.chunk(MINIBATCHES):
                env.ppo_grad(obs[:T], act, logp, adv, ret, idx=mb, grad=g_buf, stats=s_buf)
                with torch.no_grad():
                    g_buf.mul_((0.5 / (s_buf[5].sqrt() + 1e-6)).clamp(max=1.0))
                w_flat.grad = g_buf
                opt.step()
                env.update_policy(flat)

    res["python_loop"] = timed(torch, python_loop)
    env.update_policy(flat)
    res["ppo_update"] = timed(torch, device_update)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_update()
    res["ppo_update_graph"] = timed(torch, graph.replay)
    res["skipped_steps"] = float(state.clock[3].item())
    res["launches_per_update"] = EPOCHS * (1 + 7 * MINIBATCHES)
    a, b, c = (res[k]["us_per_update_median"] for k in ("python_loop", "ppo_update", "ppo_update_graph"))
    res["speedup_eager"], res["speedup_graph"] = round(a / b, 2), round(a / c, 2)
    merge(args.out, "update", res)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
