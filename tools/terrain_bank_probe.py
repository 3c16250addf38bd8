"""What the planner envs' terrain bank costs, measured on the GPU: HIP events, warm-up, the arms alternating in one process.

    python tools/terrain_bank_probe.py [--envs 4096] [--steps 1000] [--repeats 3] [--out profiles/terrain_bank.json]
                                       [--deviation FILE] [--headline-this FILE --headline-parent FILE]

Arms, each a handle of `envs` Walker3DPlannerEnv-v0 envs under auto-reset, stepped with the same seeded random actions:
  shared      the shipped grid through mocca_set_heightfield: one grid for all envs
  bank1       the same grid as a bank of one (mocca_set_heightfield_bank)
  bank64 / bank256 / bank1024   generated banks, every env on a field of its own draw, redrawn at every reset
Per arm: microseconds per step over `steps` launches, `repeats` times, the arms taking turns inside a repeat so that drift hits them alike.
GATE: the bank of one is no slower than the shared grid by more than the spread (max - min) between the repeats of the shared-grid arm
itself; the exit status says so.  The larger banks are reported, not gated: a bank of 1024 fields is 64 MB (128 MB with the pooled copy the
walker's pelvis sphere needs) and no longer fits the L2.  Also recorded: the event time to generate 256 fields of 128 x 128 on the device
and, beside it, the host route's wall time on the same box -- host_logic.random_height_field x 256 plus the upload.
--deviation: the file test_gpu_terrain_bank.py writes under MOCCA_TEST_OUT (the generator's largest deviation from the f64 reference);
--headline-*: files of bench.py result lines of this commit and its parent from the same session.  Both are copied into the output.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _lines(path):
    if not path or not os.path.exists(path):
        return []
    return [json.loads(ln) for ln in map(str.strip, open(path)) if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_bank.json"))
    ap.add_argument("--deviation", default=None)
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("terrain_bank_probe needs a GPU: there is nothing to measure without one")
    from mocca_envs_amd import host_logic as H
    from mocca_envs_amd.terrain import load_height_field
    from mocca_envs_amd.vec_env import VecEnv
    n = args.envs
    field, scale = load_height_field()
    rows, cols = field.shape

    def make(kind):
        env = VecEnv("Walker3DPlannerEnv-v0", n, device=0, auto_reset=True, seed=1)
        if kind == "bank1":
            env.set_heightfield_bank(field[None], scale)
        elif kind.startswith("bank"):
            env.set_heightfield_bank(int(kind[4:]), scale, rows=rows, cols=cols)
            env.generate_heightfields(7)
            env.set_env_fields(None, redraw_at_reset=True)
        env.reset()
        return env
    arms = {k: make(k) for k in ("shared", "bank1", "bank64", "bank256", "bank1024")}
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.rand(64, n, 21, device="cuda", generator=g) * 2 - 1
    for env in arms.values():
        for t in range(args.warmup):
            env.step(acts[t % 64])
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, env in arms.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for t in range(args.steps):
                env.step(acts[t % 64])
            ev1.record()
            ev1.synchronize()
            us[k].append(ev0.elapsed_time(ev1) * 1e3 / args.steps)
    doc = {"device": torch.cuda.get_device_name(0), "env_id": "Walker3DPlannerEnv-v0", "envs": n, "steps_per_window": args.steps,
           "repeats": args.repeats, "warmup_steps": args.warmup, "field": [rows, cols, scale]}
    doc["step_us"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": v} for k, v in us.items()}
    doc["env_steps_per_s"] = {k: n / (statistics.median(v) * 1e-6) for k, v in us.items()}
    doc["fields_in_use"] = {k: int(torch.unique(env.env_fields()).numel()) for k, env in arms.items() if k != "shared"}
    spread = max(us["shared"]) - min(us["shared"])
    excess = statistics.median(us["bank1"]) - statistics.median(us["shared"])
    doc["gate"] = {"shared_repeat_spread_us": spread, "bank1_minus_shared_us": excess, "pass": bool(excess <= spread)}
    doc["over_shared"] = {k: statistics.median(v) / statistics.median(us["shared"]) for k, v in us.items()}
    # the generator: 256 fields on the device (events around the call, after a warm call) against the host route on this box
    env = arms["bank256"]
    env.generate_heightfields(8)
    torch.cuda.synchronize()
    times = []
    for r in range(5):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        env.generate_heightfields(9 + r)
        ev1.record()
        ev1.synchronize()
        times.append(ev0.elapsed_time(ev1))
    t0 = time.perf_counter()
    host = np.stack([H.random_height_field(np.random.RandomState(s), (rows, cols), scale).reshape(rows, cols).astype(np.float32) for s in range(256)])
    t1 = time.perf_counter()
    env.set_heightfield_bank(host, scale)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    doc["generate_256_fields"] = {"device_ms": {"median": statistics.median(times), "min": min(times), "max": max(times)},
                                  "host_generate_s": t1 - t0, "host_upload_s": t2 - t1, "host_route_s": t2 - t0,
                                  "host_over_device": (t2 - t0) * 1e3 / statistics.median(times)}
    for e in arms.values():
        e.close()
    if args.deviation and os.path.exists(args.deviation):
        d = json.load(open(args.deviation))
        doc["generator_max_abs_deviation_m"] = {"bound": d["bound"], "worst": max(d["cases"].values()), "cases": d["cases"]}
    this, parent = _lines(args.headline_this), _lines(args.headline_parent)
    if this or parent:
        doc["bench_headline"] = {"this_commit": this, "parent_commit": parent}
        vals, mine = [r["value"] for r in parent if "value" in r], [r["value"] for r in this if "value" in r]
        if vals and mine:
            doc["bench_headline"]["parent_spread"] = (max(vals) - min(vals)) / statistics.median(vals)
            doc["bench_headline"]["this_over_parent"] = statistics.median(mine) / statistics.median(vals)
    print(json.dumps({k: v for k, v in doc.items() if k != "bench_headline"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["gate"]["pass"]:
        raise SystemExit(f"GATE: the bank of one is {excess:.2f} us per step slower than the shared grid; the shared arm's own spread is {spread:.2f} us")


if __name__ == "__main__":
    main()
