"""Does a planner policy trained on a terrain bank carry over to terrain it has not seen?  Deterministic evaluation of policies that
tools/ppo_demo.py saved (`<out>_policy.npz`, a planner id with --base-controller and --height-scan) on the shipped map and on held-out
generated fields.

    python tools/terrain_bank_eval.py --policy NAME=FILE [--policy NAME=FILE ...] --base-controller FILE [--height-scan 8,5]
                                      [--envs 1024] [--held-out 64] [--held-out-seed 100000] [--out FILE.jsonl]

Per policy and terrain -- "shipped": every env on the shipped height_field_map_0; "held_out": env e on field e mod K of a bank of K fields
generated on the device from a seed no training run uses -- every env plays ONE episode with the mean action (no noise): mean return and
mean length over the envs, one JSON line per cell, appended to --out.  Reported, not gated.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", action="append", required=True, metavar="NAME=FILE")
    ap.add_argument("--env-id", default="Walker3DPlannerEnv-v0")
    ap.add_argument("--base-controller", required=True)
    ap.add_argument("--height-scan", default="8,5")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--held-out", type=int, default=64)
    ap.add_argument("--held-out-seed", type=int, default=100000)
    ap.add_argument("--terrain-gain", type=float, default=1.0)
    ap.add_argument("--max-steps", type=int, default=1001)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mocca_envs_amd.controller import BaseController
    from mocca_envs_amd.perception import scan_grid
    from mocca_envs_amd.trainer_api import make_vec_envs
    nx, ny = (int(v) for v in args.height_scan.split(","))
    n = args.envs
    for spec in args.policy:
        name, path = spec.split("=", 1)
        z = np.load(path)
        dev = torch.device("cuda", 0)
        w = {k: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith("pi_")}
        mean, var = torch.from_numpy(z["obs_mean"]).to(dev), torch.from_numpy(z["obs_var"]).to(dev)

        def act(obs):      # ppo_demo's actor: 256-256 tanh MLP on the normalised, clipped observation; the mean action
            x = ((obs - mean) / torch.sqrt(var + 1e-8)).clamp(-10.0, 10.0)
            x = torch.tanh(x @ w["pi_0_weight"].T + w["pi_0_bias"])
            x = torch.tanh(x @ w["pi_2_weight"].T + w["pi_2_bias"])
            return x @ w["pi_4_weight"].T + w["pi_4_bias"]
        for terrain in ("shipped", "held_out"):
            extra = dict(base_controller=BaseController.load(args.base_controller), height_scan=dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), nx, ny)))
            if terrain == "held_out":
                extra["terrain_bank"] = dict(n_fields=args.held_out, seed=args.held_out_seed, gain=args.terrain_gain, redraw_at_reset=False)
            envs = make_vec_envs(args.env_id, seed=12345, num_processes=n, record_events=False, **extra)
            if terrain == "held_out":
                envs.venv.set_env_fields(np.arange(n) % args.held_out, redraw_at_reset=False)
            obs = envs.reset()
            alive = torch.ones(n, device=dev)
            ret, length = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            with torch.no_grad():
                for t in range(args.max_steps):
                    obs, rew, _, _ = envs.step(act(obs))
                    ret += alive * rew.reshape(-1)
                    length += alive
                    alive = alive * envs.masks.reshape(-1)
                    if t % 100 == 99 and float(alive.sum()) == 0.0:
                        break
            line = {"policy": name, "terrain": terrain, "envs": n, "mean_return": float(ret.mean()), "mean_length": float(length.mean()),
                    "unfinished": int(alive.sum()), "trained_env_steps": int(z["env_steps"])}
            if terrain == "held_out":
                line.update(held_out_fields=args.held_out, held_out_seed=args.held_out_seed, terrain_gain=args.terrain_gain)
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            envs.close()


if __name__ == "__main__":
    main()
