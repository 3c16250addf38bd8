"""Time per step of the planner env with its base controller, 4096 envs of MikePlannerEnv-v0 (--env-id), reference-sized random controller,
plans resident on the device, HIP events around >= 1000 steps after a pre-roll, three repeats each:
  (a) floor        step(actions) alone on pre-computed joint actions
  (b) torch        the same controller composed from torch ops (cat, F.linear + activations), step(), reward add -- the yardstick
  (c) plan_step    the controller kernel + the step kernel (VecEnv.plan_step)
  (d) torch policy a trainer's high-level policy in torch (normalisation, 52-256-256-15 tanh actor, 52-256-256-1 critic, the sample and
                   its log-probability), then plan_step on its plan -- what collection on a planner env costs without a device policy
  (e) act_plan_step the same policy attached as a DevicePolicy: policy kernel + controller kernel + step kernel in one call
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
    ap.add_argument("--env-id", default="MikePlannerEnv-v0")
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

    # the high-level policy of legs d and e: a2c-ppo-acktr's shapes on the 52-float observation, plans out
    from mocca_envs_amd.policy import DevicePolicy  # noqa: E402
    policy = DevicePolicy(net([52, 256, 256, 15], ["tanh", "tanh", "identity"]), net([52, 256, 256, 1], ["tanh", "tanh", "identity"]),
                          np.full(15, -1.0, np.float32), obs_mean=rng.normal(0, 0.1, 52), obs_var=rng.uniform(0.5, 2.0, 52))
    pnets = [[(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), acts[a]) for w, b, a in net] for net in (policy.actor, policy.critic)]
    p_mean, p_inv_std, p_log_std = (torch.from_numpy(x).cuda() for x in (policy.obs_mean, policy.inv_std, policy.log_std))
    p_plan, p_logp, p_value = torch.zeros(n, 15, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")

    for leg in args.legs:
        env = VecEnv(args.env_id, n, seed=1, base_controller=ctrl if leg in "cde" else None)
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
        elif leg == "d":
            def fn(t):
                with torch.no_grad():
                    x = ((env.obs - p_mean) * p_inv_std).clamp(-10.0, 10.0)
                    mu, value = forward(pnets[0], x), forward(pnets[1], x)
                    eps = torch.randn_like(mu)
                    torch.addcmul(mu, p_log_std.exp(), eps, out=p_plan)
                    torch.sum(-0.5 * eps * eps - p_log_std - 0.9189385332046727, dim=1, out=p_logp)
                    p_value.copy_(value[:, 0])
                    env.plan_step(p_plan)
        elif leg == "e":
            env.set_policy(policy)
            env.update_policy(policy)
            fn = lambda t: env.act_plan_step(env.obs, plan_out=p_plan, logp_out=p_logp, value_out=p_value)
        else:
            fn = lambda t: env.plan_step(plans[t % 64])
        for t in range(args.preroll):
            fn(t)
        torch.cuda.synchronize()
        us = timed(fn, args.steps, args.repeats)
        results.append({"leg": {"a": "step(actions) floor", "b": "torch composition + step", "c": "plan_step", "d": "torch policy + plan_step",
                                "e": "act_plan_step"}[leg], "env_id": args.env_id, "envs": n, "steps": args.steps,
                        "us_per_step": [round(u, 2) for u in us], "median_us": round(float(np.median(us)), 2), "spread_us": round(max(us) - min(us), 2)})
        print(json.dumps(results[-1]), flush=True)
        env.close()
    if args.out:
        doc = {"what": f"tools/planner_loop_bench.py: {args.env_id}, reference-sized random controller, HIP-event time per step in us, "
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
