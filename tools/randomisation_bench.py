"""What does the domain randomisation cost?  Device-event timings on one MI355X, reported, not gated.

    python tools/randomisation_bench.py [--env-id Walker3DCustomEnv-v0] [--envs 4096] [--steps 200] [--blocks 8] [--out FILE.json]

Two handles step the same actions (uniform in [-1, 1]) in interleaved blocks of --steps steps: one with nothing attached, one with the
identity randomisation (strength [1, 1], delay 0, no pushes), whose perturb launch reads the action, clips, multiplies, writes the ring
and the effective action -- everything but the read of an older ring slot that a delay > 0 adds -- and leaves the dynamics alone: both
handles run the same physics, bit for bit (checked), and the difference is the perturb launch.  Then the sensor-noise launch and the
record launch, back to back on one stream (the figure includes the launch gap, as a trainer's step does).  Prints and writes one JSON
object: per-step medians and spreads (max - min over the blocks) in microseconds, and the step kernel's registers, LDS and scratch.
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
    ap.add_argument("--env-id", default="Walker3DCustomEnv-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from mocca_envs_amd.randomisation import Randomisation
    from mocca_envs_amd.vec_env import VecEnv
    if not torch.cuda.is_available():
        raise SystemExit("randomisation_bench needs a GPU: a timing taken elsewhere says nothing")
    n = args.envs
    plain, attached = VecEnv(args.env_id, n, device=0, seed=0), VecEnv(args.env_id, n, device=0, seed=0)
    attached.set_randomisation(Randomisation(obs_noise=0.02))
    act = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (args.blocks + 1, n, plain.act_dim)).astype(np.float32)).cuda()

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / reps      # microseconds per call

    for e in (plain, attached):
        e.reset()
        timed(lambda: e.step(act[args.blocks]), 50)     # warm-up: code objects, the pace calibration
    t_plain, t_att = [], []
    for k in range(args.blocks):                         # interleaved: other work shares the machine
        t_plain.append(timed(lambda: plain.step(act[k]), args.steps))
        t_att.append(timed(lambda: attached.step(act[k]), args.steps))
    same = bool((plain.get_state() == attached.get_state()).all())
    rows, rec = attached.obs.clone(), torch.zeros(n, 4, device="cuda")
    timed(lambda: attached.sensor_noise(rows), 50), timed(lambda: attached.randomisation_record(rec), 50)
    t_noise = [timed(lambda: attached.sensor_noise(rows), 1000) for _ in range(args.blocks)]
    t_rec = [timed(lambda: attached.randomisation_record(rec), 1000) for _ in range(args.blocks)]
    med = lambda v: float(np.median(v))
    spread = lambda v: float(np.max(v) - np.min(v))
    out = {"env_id": args.env_id, "envs": n, "steps_per_block": args.steps, "blocks": args.blocks,
           "step_us": {"median": med(t_plain), "spread": spread(t_plain)},
           "step_with_perturb_us": {"median": med(t_att), "spread": spread(t_att)},
           "perturb_us": med(t_att) - med(t_plain),
           "same_state_after_the_blocks": same,
           "sensor_noise_launch_us": {"median": med(t_noise), "spread": spread(t_noise), "dim": attached.obs_dim},
           "record_launch_us": {"median": med(t_rec), "spread": spread(t_rec)},
           "kernel_info": plain.kernel_info()}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    plain.close(), attached.close()


if __name__ == "__main__":
    main()
