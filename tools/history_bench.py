"""What does the observation-action history cost?  Device-event timings on one MI355X, reported, not gated.

    python tools/history_bench.py [--env-id Walker3DCustomEnv-v0] [--envs 4096] [--history 3[,S]] [--steps 200] [--blocks 8] [--out FILE.json]

Three handles step the same actions (uniform in [-1, 1]) in interleaved blocks of --steps steps, on one stream: one steps and nothing
else; one steps and then writes the row [obs | hist] with the history kernel (one launch, in place on the wide row, plus the copy of the
observation into the row's head that a trainer without another sensor pays: `TorchVecEnv`'s path); one steps and builds the SAME row in
torch eager -- `torch.cat` of the previous observation and the action into a frame, `torch.roll` of the frames, a `torch.where` on the
step's `done` for the envs whose episode ended, `torch.cat` into the row.  The history's cost is the difference to the plain step, per arm;
the history launch alone, back to back, is timed as well (the figure includes the launch gap, as a trainer's step does).  The three handles
run the same physics, and the two rows are compared by bits after the blocks.  Prints and writes one JSON object: per-step medians and
spreads (max - min over the blocks) in microseconds, and the step kernel's registers, LDS and scratch.
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
    ap.add_argument("--history", default="3", metavar="K[,S]")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from mocca_envs_amd.history import History
    from mocca_envs_amd.vec_env import VecEnv
    if not torch.cuda.is_available():
        raise SystemExit("history_bench needs a GPU: a timing taken elsewhere says nothing")
    n = args.envs
    hist = History(*(int(v) for v in args.history.split(",")))
    if hist.stride != 1:
        raise SystemExit("the torch arm rolls one frame per step: stride 1")
    plain, kernel, eager = (VecEnv(args.env_id, n, device=0, seed=0) for _ in range(3))
    kernel.set_history(hist)
    d, a, K = plain.obs_dim, plain.act_dim, hist.steps
    w = kernel.history_dim
    act = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (args.blocks + 1, n, a)).astype(np.float32)).cuda()
    row_k = torch.zeros(n, d + w, device="cuda")
    state = {"frames": torch.zeros(n, K, d + a, device="cuda"), "prev": torch.zeros(n, d, device="cuda"), "row": torch.zeros(n, d + w, device="cuda")}
    zero = torch.zeros((), device="cuda")

    def kernel_step(x):
        kernel.step(x)
        row_k[:, :d].copy_(kernel.obs)
        kernel.history(row_k, x, out=row_k[:, d:])

    def eager_step(x):
        eager.step(x)
        frames = torch.roll(state["frames"], 1, dims=1)
        frames[:, 0] = torch.cat([state["prev"], x], 1)
        frames = torch.where((eager.done != 0)[:, None, None], zero, frames)
        state["frames"], state["prev"] = frames, eager.obs.clone()
        state["row"] = torch.cat([eager.obs, frames.reshape(n, -1)], 1)

    def timed(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1000.0 / reps      # microseconds per call

    for e in (plain, kernel, eager):
        e.reset()
    row_k[:, :d].copy_(kernel.obs)
    kernel.history(row_k, None, out=row_k[:, d:])
    state["prev"].copy_(eager.obs)
    warm = act[args.blocks]
    timed(lambda: plain.step(warm), 50), timed(lambda: kernel_step(warm), 50), timed(lambda: eager_step(warm), 50)      # code objects, the pace calibration
    t_plain, t_kernel, t_eager = [], [], []
    for k in range(args.blocks):                         # interleaved: other work shares the machine
        x = act[k]
        t_plain.append(timed(lambda: plain.step(x), args.steps))
        t_kernel.append(timed(lambda: kernel_step(x), args.steps))
        t_eager.append(timed(lambda: eager_step(x), args.steps))
    torch.cuda.synchronize()
    same_state = bool((plain.get_state() == kernel.get_state()).all()) and bool((plain.get_state() == eager.get_state()).all())
    same_rows = bool((row_k.view(torch.int32) == state["row"].view(torch.int32)).all())
    timed(lambda: kernel.history(row_k, warm, out=row_k[:, d:]), 50)
    t_launch = [timed(lambda: kernel.history(row_k, warm, out=row_k[:, d:]), 1000) for _ in range(args.blocks)]
    med = lambda v: float(np.median(v))
    spread = lambda v: float(np.max(v) - np.min(v))
    out = {"env_id": args.env_id, "envs": n, "history": hist.as_dict(), "history_dim": w, "row": d + w, "steps_per_block": args.steps, "blocks": args.blocks,
           "step_us": {"median": med(t_plain), "spread": spread(t_plain)},
           "step_with_history_kernel_us": {"median": med(t_kernel), "spread": spread(t_kernel)},
           "step_with_torch_eager_rows_us": {"median": med(t_eager), "spread": spread(t_eager)},
           "history_kernel_arm_us": med(t_kernel) - med(t_plain),
           "torch_eager_arm_us": med(t_eager) - med(t_plain),
           "history_launch_us": {"median": med(t_launch), "spread": spread(t_launch), "bytes_moved_per_launch": 4 * n * (2 * w + d + a)},
           "same_state_after_the_blocks": same_state, "same_rows_after_the_blocks": same_rows,
           "kernel_info": plain.kernel_info()}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for e in (plain, kernel, eager):
        e.close()


if __name__ == "__main__":
    main()
