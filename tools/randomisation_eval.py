"""Does a policy survive a plant it was not trained on?  Deterministic evaluation of policies that tools/ppo_demo.py saved
(`<out>_policy.npz`) under a given domain randomisation (mocca_envs_amd/randomisation.py): weaker motors, late commands, pushes, noisy
sensors -- or none, the plain plant.

    python tools/randomisation_eval.py --policy NAME=FILE [--policy NAME=FILE ...] [--env-id Walker3DCustomEnv-v0] [--envs 1024]
                                       [--rand-strength LO,HI] [--rand-latency LO,HI] [--rand-push INTERVAL,MAX] [--obs-noise SCALE]
                                       [--curriculum K[,K ...]] [--condition LABEL] [--out FILE.jsonl]

Per policy every env plays ONE episode with the mean action (no action noise; the sensor noise of the condition is applied): mean return and
mean length over the envs, one JSON line per policy, appended to --out, with the condition and the randomisation the policy's file says it
was trained under.  A policy trained with an observation-action history (ppo_demo.py --history; its file records the `History`) plays on
an env rebuilt with the same history: its rows are [obs | hist] again.  --curriculum K[,K ...] (Stepper ids): one cell per level, every
env on the terrain of the fixed level K (e.g. 0,5,9 for a policy trained with ppo_demo.py --curriculum / --adaptive-curriculum); each line
then carries `curriculum` and `mean_steps_reached`, the mean of steps_reached over the episodes.  Reported, not gated.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", action="append", required=True, metavar="NAME=FILE")
    ap.add_argument("--env-id", default="Walker3DCustomEnv-v0")
    ap.add_argument("--envs", type=int, default=1024, help="episodes played: one per env")
    ap.add_argument("--rand-strength", default=None, metavar="LO,HI")
    ap.add_argument("--rand-latency", default=None, metavar="LO,HI")
    ap.add_argument("--rand-push", default=None, metavar="INTERVAL,MAX")
    ap.add_argument("--obs-noise", type=float, default=None, metavar="SCALE")
    ap.add_argument("--curriculum", default=None, metavar="K[,K ...]", help="Stepper ids: evaluate at each of these fixed curriculum levels, one line per level")
    ap.add_argument("--condition", default=None, help="a label for the lines written (default: 'randomised' with any --rand-* / --obs-noise flag, else 'plain')")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--max-steps", type=int, default=1001)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from mocca_envs_amd.randomisation import Randomisation
    from mocca_envs_amd.trainer_api import make_vec_envs
    pair = lambda text, kind, default: default if text is None else tuple(k(v) for k, v in zip(kind, text.split(",")))
    randomised = any(v is not None for v in (args.rand_strength, args.rand_latency, args.rand_push, args.obs_noise))
    rand = Randomisation(strength=pair(args.rand_strength, (float, float), (1.0, 1.0)), latency=pair(args.rand_latency, (int, int), (0, 0)),
                         push=pair(args.rand_push, (int, float), (0, 0.0)), obs_noise=args.obs_noise) if randomised else None
    condition = args.condition or ("randomised" if randomised else "plain")
    n = args.envs
    levels = [None] if args.curriculum is None else [int(v) for v in args.curriculum.split(",")]
    if args.curriculum is not None and ("Stepper" not in args.env_id or not all(0 <= k <= 9 for k in levels)):
        ap.error("--curriculum takes levels 0 .. 9 of a Stepper id")
    for spec, level in ((s, k) for s in args.policy for k in levels):
        name, path = spec.split("=", 1)
        z = np.load(path, allow_pickle=False)
        dev = torch.device("cuda", 0)
        w = {k: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith("pi_")}
        mean, var = torch.from_numpy(z["obs_mean"]).to(dev), torch.from_numpy(z["obs_var"]).to(dev)

        def act(obs):      # ppo_demo's actor: 256-256 tanh MLP on the normalised, clipped observation; the mean action
            x = ((obs - mean) / torch.sqrt(var + 1e-8)).clamp(-10.0, 10.0)
            x = torch.tanh(x @ w["pi_0_weight"].T + w["pi_0_bias"])
            x = torch.tanh(x @ w["pi_2_weight"].T + w["pi_2_bias"])
            return x @ w["pi_4_weight"].T + w["pi_4_bias"]
        hist = None
        if "history" in z.files:     # the sensor setting stored beside the policy
            from mocca_envs_amd.history import History
            hist = History.from_dict(json.loads(str(z["history"])))
        envs = make_vec_envs(args.env_id, seed=args.seed, num_processes=n, record_events=False, **({} if rand is None else dict(randomisation=rand)),
                             **({} if hist is None else dict(history=hist)))
        if level is not None:
            envs.set_env_params({"curriculum": level})      # (before the reset, which lays the terrain out)
        obs = envs.reset()
        alive = torch.ones(n, device=dev)
        ret, length, reached = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        with torch.no_grad():
            for t in range(args.max_steps):
                obs, rew, _, _ = envs.step(act(obs))
                ret += alive * rew.reshape(-1)
                length += alive
                reached += alive * (1.0 - envs.masks.reshape(-1)) * envs.venv.info      # the info word of the step that ends the episode
                alive = alive * envs.masks.reshape(-1)
                if t % 100 == 99 and float(alive.sum()) == 0.0:
                    break
        line = {"policy": name, "condition": condition, "envs": n, "mean_return": float(ret.mean()), "mean_length": float(length.mean()),
                "unfinished": int(alive.sum()), "trained_env_steps": int(z["env_steps"]),
                "evaluated_under": None if rand is None else rand.as_dict(),
                "trained_under": json.loads(str(z["randomisation"])) if "randomisation" in z.files else None,
                "history": None if hist is None else hist.as_dict()}
        if level is not None:
            line.update(curriculum=level, mean_steps_reached=float(reached.mean()))
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        envs.close()


if __name__ == "__main__":
    main()
