"""What the terrain height scan costs next to the step kernel, measured on the GPU: HIP events, warm-up, one process.

    python tools/height_scan_bench.py [--envs 4096] [--steps 200] [--rounds 5] [--out profiles/height_scan_bench.json]
                                      [--headline-this FILE --headline-parent FILE]

Per env id (Walker3DStepperEnv-v0, Walker3DPlannerEnv-v0) and pattern size (P = 77, 256), after a pre-roll of random-action steps:
  step_us         time per step of `step` alone
  step_scan_us    time per step of `step` + the fused scan launch (row [obs | scan])
  scan_us         the scan launch on its own (fused form), back to back
Each figure is the median over `rounds` windows of `steps` launches, the three kinds of window alternating inside a round so that drift
hits them alike; min and max of the windows are kept.  The files named by --headline-this / --headline-parent hold `bench.py` result
lines (one JSON object per line) of this commit and of its parent from the same machine; they are copied into the output together with
the scan's cost as a share of the parent's step time.  There is no threshold: the figures are reported.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, steps, torch):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for t in range(steps):
        fn(t)
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / steps      # microseconds per call


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure(env_id, n_points, envs, steps, rounds, preroll):
    import numpy as np
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    env = VecEnv(env_id, envs, device=0, auto_reset=True, seed=1)
    env.reset()
    side = int(np.ceil(np.sqrt(n_points)))
    xs, ys = np.meshgrid(np.linspace(-0.6, 1.5, side), np.linspace(-0.9, 0.9, side), indexing="ij")
    pts = np.stack([xs.ravel(), ys.ravel()], 1)[:n_points].astype(np.float32)
    env.set_height_scan(pts, 1.0, 2.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.rand(steps, envs, env.act_dim, device="cuda", generator=g) * 2 - 1
    wide = torch.zeros(envs, env.obs_dim + n_points, device="cuda")
    step = lambda t: env.step(acts[t % steps])
    both = lambda t: env.height_scan(out=wide, obs=env.step(acts[t % steps])[0])
    scan = lambda t: env.height_scan(out=wide, obs=env.obs)
    for t in range(preroll):          # warm-up of every launch the windows use; the batch reaches its steady mix of episode phases
        both(t)
    torch.cuda.synchronize()
    out = {"step_us": [], "step_scan_us": [], "scan_us": []}
    for _ in range(rounds):
        out["step_us"].append(_window(step, steps, torch))
        out["step_scan_us"].append(_window(both, steps, torch))
        out["scan_us"].append(_window(scan, steps, torch))
    env.close()
    res = {"env_id": env_id, "envs": envs, "n_points": n_points, "steps_per_window": steps, "rounds": rounds}
    res.update({k: _stats(v) for k, v in out.items()})
    res["scan_share_of_step"] = res["scan_us"]["median"] / res["step_us"]["median"]
    res["fused_overhead_share"] = res["step_scan_us"]["median"] / res["step_us"]["median"] - 1.0
    return res


def _lines(path):
    if not path or not os.path.exists(path):
        return []
    out = []
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith("{"):
            out.append(json.loads(ln))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "height_scan_bench.json"))
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("height_scan_bench needs a GPU: there is nothing to measure without one")
    cases = [measure(env_id, p, args.envs, args.steps, args.rounds, args.preroll)
             for env_id in ("Walker3DStepperEnv-v0", "Walker3DPlannerEnv-v0") for p in (77, 256)]
    for c in cases:
        print(json.dumps(c), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "cases": cases}
    this, parent = _lines(args.headline_this), _lines(args.headline_parent)
    if this or parent:
        doc["bench_headline"] = {"this_commit": this, "parent_commit": parent}
        vals = [r["value"] for r in parent if "value" in r]
        if vals:      # bench.py's headline: env-steps/s of the flagship workload, and its wall time per step of the batch
            step_us = 1e3 * statistics.median(r["ms_per_step"] for r in parent if "value" in r)
            doc["bench_headline"]["parent_step_us"] = step_us
            doc["bench_headline"]["parent_spread"] = (max(vals) - min(vals)) / statistics.median(vals)
            mine = [r["value"] for r in this if "value" in r]
            if mine:
                doc["bench_headline"]["this_over_parent"] = statistics.median(mine) / statistics.median(vals)
            doc["scan_share_of_parent_step"] = {f'{c["env_id"]}:{c["n_points"]}': c["scan_us"]["median"] / step_us for c in cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
