#!/usr/bin/env python3
"""What a SymmetricRL / ALLSTEPS-style PPO collection loop gets out of mocca_envs_amd.trainer_api.TorchVecEnv on one MI355X.
Policy: MLP obs-64-act on the GPU; every loop writes the masked observation into a rollout buffer as the PPO storage does.
  trainer_loop_verbatim       the trainers' own loop, habits included: a Python list comprehension over `done` for the masks, a loop over the
                              N info dicts (both force the lazy `done` / `infos` of THIS step: one wait per step, then ~3 x N Python iterations)
  trainer_loop_device_masks   `envs.masks` / `envs.bad_masks` from the device, episode returns from `infos.episodes()` (arrays, no dict per env)
                              read ONE STEP LATE (after the next step has been issued: the wait never lets the GPU run dry)
  trainer_loop_device_totals  the same without `infos`: episode statistics from `envs.episode_totals` (device) at the end; built with
                              `record_events=False` (no per-step event record: nothing ever waits for a step)
  trainer_loop_graphed        policy -> mocca_step -> rollout write of `--chunk` consecutive steps captured in ONE torch.cuda.CUDAGraph
                              (`TorchVecEnv.capture_rollout`) and replayed: the collection phase without the host
  trainer_loop_in_place       PPO's own structure: the policy reads rollouts.obs[t]; the step kernel writes observation, reward, masks and
                              bad_masks of step t STRAIGHT into rows t + 1 / t of the storage (`step(action, into=...)`), the policy its action
                              into rollouts.actions[t]: `rollouts.insert` without a copy kernel; `_graphed`: the same from one CUDA graph
  trainer_loop_device_policy  the same storage, the policy on the device too (`attach_policy`, `act_step(into=...)`): the policy kernel writes action,
                              log-probability and value into rows t, the step kernel the rest -- two launches per step and no torch op;
                              `_graphed`: `capture_rollout()` with the attached policy.  It does MORE than the torch policy of the other rows
                              (critic, noise, log-probability, observation normalisation)
  --finish: ONLY the `finish` section -- what a PPO iteration does between collection and learning, T = --finish-steps (32) at each of
                              --finish-envs (4096,8192), HIP events around the phase, the two paths alternating in one process:
                              `torch`  tools/ppo_demo.py's default path restated: the running observation statistics from row 0 of the storage
                                       (a handful of reductions) and the GAE loop over t, returns, advantage normalisation;
                              `device` `finish_rollout` + `update_obs_stats` over ALL T x N observation rows: 4 launches
  --net ppo: every loop's policy is tools/ppo_demo.py's obs-256-256-act tanh MLP instead of obs-64-act
  python tools/trainer_loop_bench.py [--envs 4096] [--steps 300] [--env-id Walker3DCustomEnv-v0] [--sub-batches 1] [--chunk 10] [--net bench|ppo]
  python tools/trainer_loop_bench.py --finish [--finish-envs 4096,8192] [--finish-steps 32] [--finish-rounds 200]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def finish_section(args):
    """returns, advantages, their normalisation and the observation statistics of one PPO iteration: torch (the demo's default path) against
    the rollout kernels, on a storage a random policy filled"""
    import statistics
    import torch
    from mocca_envs_amd.rollout import ObsStats
    from mocca_envs_amd.trainer_api import make_vec_envs
    T, gamma, lam, scale = args.finish_steps, 0.99, 0.95, 0.1
    out = {"section": "finish", "env_id": args.env_id, "steps": T, "rounds": args.finish_rounds, "timer": "HIP events around the phase, ms",
           "protocol": "20 warm rounds, then the two paths alternate for `rounds` rounds in one process; median, min and the 10 % / 90 % quantiles", "rows": []}
    for N in [int(x) for x in args.finish_envs.split(",")]:
        envs = make_vec_envs(args.env_id, seed=0, num_processes=N, record_events=False)
        dev, od, ad = envs.device, envs.observation_space.shape[0], envs.action_space.shape[0]
        S = {"obs": torch.zeros(T + 1, N, od, device=dev), "reward": torch.zeros(T, N, 1, device=dev), "masks": torch.ones(T + 1, N, 1, device=dev),
             "bad_masks": torch.ones(T + 1, N, 1, device=dev), "value": torch.randn(T + 1, N, 1, device=dev)}
        S["obs"][0].copy_(envs.reset())
        for t in range(T):      # a real rollout: rewards, masks and time limits as the step kernel writes them
            envs.step(torch.randn(N, ad, device=dev).clamp(-1, 1), into={"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1],
                                                                       "bad_masks": S["bad_masks"][t + 1]})
        state = {"mean": torch.zeros(od, device=dev), "var": torch.ones(od, device=dev), "count": 1e-4}

        def torch_path():      # tools/ppo_demo.py's default path: the statistics update, then the GAE loop, returns, normalisation
            mean, var, count = state["mean"], state["var"], state["count"]
            flat = S["obs"][0]
            bm, bv, bn = flat.mean(0), flat.var(0, unbiased=False), flat.shape[0]
            d = bm - mean
            tot = count + bn
            state["mean"] = mean + d * bn / tot
            state["var"] = (var * count + bv * bn + d * d * count * bn / tot) / tot
            state["count"] = tot
            adv = torch.zeros(T, N, 1, device=dev)
            gae = torch.zeros(N, 1, device=dev)
            rew = S["reward"] * scale
            for t in reversed(range(T)):
                delta = rew[t] + gamma * S["value"][t + 1] * S["masks"][t + 1] - S["value"][t]
                gae = (delta + gamma * lam * S["masks"][t + 1] * gae) * S["bad_masks"][t + 1]
                adv[t] = gae
            ret = adv + S["value"][:T]
            return (adv - adv.mean()) / (adv.std() + 1e-8), ret

        stats = ObsStats(od, dev)
        bufs = {k: torch.zeros(T, N, 1, device=dev) for k in ("returns", "adv")}
        moments, tail = torch.zeros(2, device=dev), torch.zeros(2 * od, device=dev)

        def device_path():
            envs.finish_rollout(S["reward"], S["value"], S["masks"], S["bad_masks"], gamma, lam, scale, returns=bufs["returns"], adv=bufs["adv"],
                                normalise=True, adv_eps=1e-8, moments=moments)
            envs.update_obs_stats(stats, S["obs"][1:], mean_out=tail[:od], inv_std_out=tail[od:])
            return bufs["adv"], bufs["returns"]

        with torch.no_grad():
            for _ in range(20):
                a_t, r_t = torch_path(); a_d, r_d = device_path()
            same = lambda u, v: bool((u.view(torch.int32) == v.view(torch.int32)).all().item())
            times = {"torch": [], "device": []}
            ev = lambda: torch.cuda.Event(enable_timing=True)
            for _ in range(args.finish_rounds):
                for name, fn in (("torch", torch_path), ("device", device_path)):
                    e0, e1 = ev(), ev()
                    e0.record(); fn(); e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
        q = lambda xs, f: sorted(xs)[min(len(xs) - 1, int(f * len(xs)))]
        row = {"envs": N, "returns_bit_identical": same(r_t, r_d), "normalised_adv_max_abs_diff": float((a_t - a_d).abs().max().item())}
        for name, xs in times.items():
            row[name + "_ms"] = {"median": statistics.median(xs), "min": min(xs), "p10": q(xs, 0.1), "p90": q(xs, 0.9)}
        # launches, counted from the code above: per step 8 elementwise kernels and the copy into adv[t]; two fills, the reward scale, the
        # returns, mean, std (one kernel each) and three elementwise kernels of the normalisation; 2 reductions and 9 elementwise kernels of
        # the statistics.  The device path: gae, moments / normalise, statistics partials, statistics merge.
        row["torch_launches"] = 9 * T + 2 + 1 + 1 + 5 + 11
        row["device_launches"] = 4
        row["torch_obs_rows_seen"], row["device_obs_rows_seen"] = N, T * N
        row["speedup_median"] = row["torch_ms"]["median"] / row["device_ms"]["median"]
        out["rows"].append(row)
        envs.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--env-id", default="Walker3DCustomEnv-v0")
    ap.add_argument("--sub-batches", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--skip-verbatim", action="store_true")
    ap.add_argument("--net", choices=("bench", "ppo"), default="bench")
    ap.add_argument("--finish", action="store_true")
    ap.add_argument("--finish-envs", default="4096,8192")
    ap.add_argument("--finish-steps", type=int, default=32)
    ap.add_argument("--finish-rounds", type=int, default=200)
    args = ap.parse_args()
    if args.finish:
        return finish_section(args)
    import torch
    from mocca_envs_amd.trainer_api import make_vec_envs
    envs = make_vec_envs(args.env_id, seed=0, num_processes=args.envs, sub_batches=args.sub_batches)
    # the totals loop never looks at `done` / `infos`: its envs are built without the per-step event record (1 us of GPU time per step)
    envs_totals = make_vec_envs(args.env_id, seed=0, num_processes=args.envs, sub_batches=args.sub_batches, record_events=False)
    dev = envs.device
    g = torch.Generator(device=dev).manual_seed(1)
    w1 = torch.randn(envs.observation_space.shape[0], 64, device=dev, generator=g) * 0.3
    w2 = torch.randn(64, envs.action_space.shape[0], device=dev, generator=g) * 0.3
    policy = lambda o: torch.tanh(torch.tanh(o @ w1) @ w2)
    if args.net == "ppo":       # ppo_demo's actor: obs-256-256-act, tanh between the layers
        v1 = torch.randn(envs.observation_space.shape[0], 256, device=dev, generator=g) * 0.1
        v2 = torch.randn(256, 256, device=dev, generator=g) * 0.06
        v3 = torch.randn(256, envs.action_space.shape[0], device=dev, generator=g) * 0.06
        policy = lambda o: torch.tanh(torch.tanh(o @ v1) @ v2) @ v3
    steps = (args.steps // args.chunk) * args.chunk
    rollouts = torch.zeros(max(steps, 50) + 1, args.envs, envs.observation_space.shape[0], device=dev)

    def verbatim(steps):
        obs = envs.reset(); ep = []
        for t in range(steps):
            with torch.no_grad():
                action = policy(obs)
            obs, reward, done, infos = envs.step(action)
            for info in infos:
                if "episode" in info.keys():
                    ep.append(info["episode"]["r"])
            masks = torch.FloatTensor([[0.0] if d else [1.0] for d in done]).to(dev)
            bad_masks = torch.FloatTensor([[0.0] if "bad_transition" in info.keys() else [1.0] for info in infos]).to(dev)
            rollouts[t + 1].copy_(obs * masks * bad_masks.clamp(min=1.0))
        return len(ep)

    def lean(steps):
        obs = envs.reset(); ep = []; prev = None
        for t in range(steps):
            with torch.no_grad():
                action = policy(obs)
            obs, reward, done, infos = envs.step(action)
            if prev is not None:      # logging one step late: waits for the launch BEFORE the one just issued
                ep.append(prev.episodes()["r"])
            prev = infos
            rollouts[t + 1].copy_(obs * envs.masks * envs.bad_masks.clamp(min=1.0))
        ep.append(prev.episodes()["r"])
        return sum(len(x) for x in ep)

    def totals(steps):
        e = envs_totals
        obs = e.reset(); e.episode_totals.zero_()
        for t in range(steps):
            with torch.no_grad():
                action = policy(obs)
            obs, reward, done, infos = e.step(action)
            rollouts[t + 1].copy_(obs * e.masks * e.bad_masks.clamp(min=1.0))
        return int(e.episode_totals[2].item())

    graph = None

    def graphed(steps):
        nonlocal graph
        if graph is None:       # (a trainer captures its whole num_steps rollout; the chunk writes rollout rows 1 .. chunk)
            graph = envs.capture_rollout(policy, args.chunk, sink=lambda t, obs, rew, masks, bad, act: rollouts[t + 1].copy_(obs * masks * bad.clamp(min=1.0)))
        envs.reset(); envs.episode_totals.zero_()
        for _ in range(steps // args.chunk):
            graph.replay()
        return int(envs.episode_totals[2].item())

    # ---- the kernel writes straight into the trainer's storage (TorchVecEnv.step(into=...)): PPO's rollouts.insert without copy kernels.
    # Storage like a2c-ppo-acktr's RolloutStorage: obs [T + 1], rewards [T], masks / bad_masks [T + 1], actions [T]; the policy reads obs[t].
    T = args.chunk
    od, ad = envs.observation_space.shape[0], envs.action_space.shape[0]
    S = {"obs": torch.zeros(T + 1, args.envs, od, device=dev), "reward": torch.zeros(T, args.envs, 1, device=dev),
         "masks": torch.ones(T + 1, args.envs, 1, device=dev), "bad_masks": torch.ones(T + 1, args.envs, 1, device=dev),
         "act": torch.zeros(T, args.envs, ad, device=dev)}
    row = lambda t: {"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1], "bad_masks": S["bad_masks"][t + 1]} if t >= 0 else {"obs": S["obs"][0]}
    policy_into = lambda o, t: torch.tanh(torch.tanh(o @ w1) @ w2, out=S["act"][t])
    if args.net == "ppo":
        policy_into = lambda o, t: torch.matmul(torch.tanh(torch.tanh(o @ v1) @ v2), v3, out=S["act"][t])

    def in_place(steps):
        e = envs_totals
        S["obs"][0].copy_(e.reset()); e.episode_totals.zero_()
        for r in range(steps // T):
            for t in range(T):
                with torch.no_grad():
                    action = policy_into(S["obs"][t], t)
                e.step(action, into=row(t))
            S["obs"][0].copy_(S["obs"][T]); S["masks"][0].copy_(S["masks"][T]); S["bad_masks"][0].copy_(S["bad_masks"][T])   # rollouts.after_update()
        return int(e.episode_totals[2].item())

    graph_ip = None

    def in_place_graphed(steps):
        nonlocal graph_ip
        e = envs_totals
        if graph_ip is None:
            graph_ip = e.capture_rollout(policy_into, T, into=row)
        S["obs"][0].copy_(e.reset()); e.episode_totals.zero_()
        for r in range(steps // T):
            graph_ip.replay()
            S["obs"][0].copy_(S["obs"][T]); S["masks"][0].copy_(S["masks"][T]); S["bad_masks"][0].copy_(S["bad_masks"][T])
        return int(e.episode_totals[2].item())

    # ---- the policy on the device as well: the same nets as a DevicePolicy (plus a critic of the actor's shape, log_std, normalisation)
    def device_policy():
        from mocca_envs_amd.policy import DevicePolicy
        cpu = lambda w: w.t().contiguous().cpu().numpy()
        if args.net == "ppo":
            ws, acts = [v1, v2, v3], ["tanh", "tanh", "identity"]
        else:
            ws, acts = [w1, w2], ["tanh", "tanh"]
        actor = [(cpu(w), torch.zeros(w.shape[1]).numpy(), a) for w, a in zip(ws, acts)]
        critic = actor[:-1] + [(actor[-1][0][:1], actor[-1][1][:1], "identity")]
        return DevicePolicy(actor, critic, torch.full((ad,), -1.0).numpy(), obs_mean=torch.zeros(od).numpy(), obs_var=torch.ones(od).numpy())

    S["logp"], S["value"] = torch.zeros(T, args.envs, 1, device=dev), torch.zeros(T, args.envs, 1, device=dev)
    row_dp = lambda t: dict(row(t), action=S["act"][t], logp=S["logp"][t], value=S["value"][t]) if t >= 0 else row(t)

    def dev_policy(steps):
        e = envs_totals
        if getattr(e, "_pol_bufs", None) is None:
            e.attach_policy(device_policy())
        S["obs"][0].copy_(e.reset()); e.episode_totals.zero_()
        for r in range(steps // T):
            for t in range(T):
                e.act_step(S["obs"][t], into=row_dp(t))
            S["obs"][0].copy_(S["obs"][T]); S["masks"][0].copy_(S["masks"][T]); S["bad_masks"][0].copy_(S["bad_masks"][T])
        return int(e.episode_totals[2].item())

    graph_dp = None

    def dev_policy_graphed(steps):
        nonlocal graph_dp
        e = envs_totals
        if graph_dp is None:
            if getattr(e, "_pol_bufs", None) is None:
                e.attach_policy(device_policy())
            graph_dp = e.capture_rollout(num_steps=T, into=row_dp)
        S["obs"][0].copy_(e.reset()); e.episode_totals.zero_()
        for r in range(steps // T):
            graph_dp.replay()
            S["obs"][0].copy_(S["obs"][T]); S["masks"][0].copy_(S["masks"][T]); S["bad_masks"][0].copy_(S["bad_masks"][T])
        return int(e.episode_totals[2].item())

    out = {"env_id": args.env_id, "envs": args.envs, "sub_batches": args.sub_batches, "steps": steps, "graph_chunk": args.chunk, "net": args.net}
    loops = [("trainer_loop_verbatim", verbatim), ("trainer_loop_device_masks", lean), ("trainer_loop_device_totals", totals)]
    if args.sub_batches == 1:
        loops += [("trainer_loop_graphed", graphed), ("trainer_loop_in_place", in_place), ("trainer_loop_in_place_graphed", in_place_graphed),
                  ("trainer_loop_device_policy", dev_policy), ("trainer_loop_device_policy_graphed", dev_policy_graphed)]
    for name, fn in loops:
        if args.skip_verbatim and fn is verbatim:
            continue
        fn(50); torch.cuda.synchronize()
        t0 = time.perf_counter(); n_ep = fn(steps); torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        out[name] = {"ms_per_step": 1e3 * dt, "env_steps_per_s": args.envs / dt, "episodes": n_ep}
    print(json.dumps(out))
    envs.close(); envs_totals.close()


if __name__ == "__main__":
    main()
