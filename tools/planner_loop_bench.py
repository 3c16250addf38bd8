"""Time per step of the planner env with its base controller, 4096 envs of MikePlannerEnv-v0, reference-sized random controller, plans
resident on the device, HIP events around >= 1000 steps after a pre-roll, three repeats each:
  (a) floor        step(actions) alone on pre-computed joint actions
  (b) torch        the same controller composed from torch ops (cat, F.linear + activations), step(), reward add -- the yardstick
  (c) plan_step    the controller kernel + the step kernel (VecEnv.plan_step)
Prints one JSON line per leg; --out FILE also writes them, with the controller's share (c) - (a), as one JSON document
(profiles/planner_controller_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mocca_envs_amd.controller import BaseController  # noqa: E402
from mocca_envs_amd.vec_env import VecEnv  # noqa: E402


def timed(fn, steps, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(steps):
            fn(t)
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="abc")
    args = ap.parse_args()
    n = args.envs
    # reference-sized nets (65-256x5-21 softsign, 65-256x4-1 relu), weights ~ N(0, 1 / fan_in)
    rng = np.random.default_rng(0)

    def net(dims, acts):
        return [(rng.normal(0, dims[i] ** -0.5, (dims[i + 1], dims[i])).astype(np.float32), rng.normal(0, 0.1, dims[i + 1]).astype(np.float32), a)
                for i, a in enumerate(acts)]

    ctrl = BaseController(net([65] + [256] * 5 + [21], ["softsign"] * 5 + ["identity"]), net([65] + [256] * 4 + [1], ["relu"] * 4 + ["identity"]))
    results = []
    plans = torch.randn(64, n, 15, device="cuda")
    acts = {"relu": torch.relu, "tanh": torch.tanh, "softsign": F.softsign, "identity": lambda t: t}
    nets = [[(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), acts[a]) for w, b, a in net] for net in (ctrl.actor, ctrl.critic)]

    def forward(net, x):
        for w, b, a in net:
            x = a(F.linear(x, w, b))
        return x

    for leg in args.legs:
        env = VecEnv("MikePlannerEnv-v0", n, seed=1, base_controller=ctrl if leg == "c" else None)
        env.reset()
        if leg == "a":
            actions = torch.rand(64, n, 21, device="cuda") * 2 - 1
            fn = lambda t: env.step(actions[t % 64])
        elif leg == "b":
            def fn(t):
                with torch.no_grad():
                    x = torch.cat((env.obs[:, :50], plans[t % 64] * 2.0), dim=1)
                    action, value = forward(nets[0], x), forward(nets[1], x)
                    env.step(action)
                    env.rew.add_(torch.log(torch.clamp(value[:, 0], min=1.0)) / 3)
        else:
            fn = lambda t: env.plan_step(plans[t % 64])
        for t in range(args.preroll):
            fn(t)
        torch.cuda.synchronize()
        us = timed(fn, args.steps, args.repeats)
        results.append({"leg": {"a": "step(actions) floor", "b": "torch composition + step", "c": "plan_step"}[leg], "envs": n, "steps": args.steps,
                        "us_per_step": [round(u, 2) for u in us], "median_us": round(float(np.median(us)), 2), "spread_us": round(max(us) - min(us), 2)})
        print(json.dumps(results[-1]), flush=True)
        env.close()
    if args.out:
        doc = {"what": "tools/planner_loop_bench.py: MikePlannerEnv-v0, reference-sized random controller, HIP-event time per step in us, "
                       f"{args.repeats} repeats of {args.steps} steps after {args.preroll}", "legs": results}
        med = {r["leg"]: r["median_us"] for r in results}
        if "plan_step" in med and "step(actions) floor" in med:
            doc["plan_step_minus_floor_us"] = round(med["plan_step"] - med["step(actions) floor"], 2)
            doc["f32_matrix_peak_us"] = 26
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
