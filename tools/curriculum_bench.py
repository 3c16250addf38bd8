"""What does the per-env adaptive curriculum cost?  Device-event timings on one MI355X, reported, not gated.

    python tools/curriculum_bench.py [--env-id Walker3DStepperEnv-v0] [--envs 4096] [--adaptive 21,-1[,PATIENCE]] [--steps 200] [--blocks 8] [--out FILE.json]

Three handles step the same actions (uniform in [-1, 1]) in interleaved blocks of --steps steps, on one stream: one steps and nothing
else; one has the curriculum attached, so that every step is followed by the rule's launch (include/mocca.h mocca_set_curriculum); one steps
and runs the HOST recipe the launch replaces, per step: read the step's done bytes and info words on the host (a synchronise), decide the
same rule in torch, write the levels with set_param_v.  The curriculum's cost is the difference to the plain step, per arm; the rule's
launch alone (mocca_curriculum_apply on a step's done bytes), back to back, is timed as well (the figure includes the launch gap, as a
trainer's step does).  The default thresholds, 21 and -1, are met by no episode: every ended episode goes through the rule and is counted, no
level moves, and the three handles keep walking the same terrain -- with thresholds that move levels the plain handle stays at level 0
while the other two climb, and the arms then also hold the dearer steps of harder terrain.  The attached handle and the host-recipe
handle are compared by levels after the blocks.  Prints and writes one JSON object: per-step medians and spreads (max - min over the
blocks) in microseconds, and the step kernel's registers, LDS and scratch.
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
    ap.add_argument("--env-id", default="Walker3DStepperEnv-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--adaptive", default="21,-1", metavar="PROMOTE,DEMOTE[,PATIENCE]")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.curriculum import Curriculum
    from mocca_envs_amd.vec_env import VecEnv
    if not torch.cuda.is_available():
        raise SystemExit("curriculum_bench needs a GPU: a timing taken elsewhere says nothing")
    n = args.envs
    cur = Curriculum(*(int(v) for v in args.adaptive.split(",")))
    plain, attached, host = (VecEnv(args.env_id, n, device=0, seed=0) for _ in range(3))
    totals = attached.set_curriculum(cur)
    host.set_param_v(L.PARAM_CURRICULUM, [0.0], broadcast=True)
    act = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (args.blocks + 1, n, plain.act_dim)).astype(np.float32)).cuda()
    state = {"level": torch.zeros(n), "streak": torch.zeros(n, dtype=torch.int64), "hold": torch.zeros(n, dtype=torch.bool)}

    def host_step(x):
        """the recipe a trainer without the launch runs: records to the host, the rule in torch, the levels back (no recycle draw: none is configured)"""
        host.step(x)
        done, s = host.done.cpu() != 0, host.info.cpu().long()      # the device-to-host read in the middle of the rollout
        level, streak, hold = state["level"], state["streak"], state["hold"]
        judged = done & ~hold
        hold &= ~done
        ok, bad = judged & (s >= cur.promote_at), judged & (s <= cur.demote_at)
        streak[judged & ~ok & ~bad] = 0
        streak[ok] = streak[ok].clamp(min=0) + 1
        streak[bad] = streak[bad].clamp(max=0) - 1
        up, down = ok & (streak >= cur.patience), bad & (streak <= -cur.patience)
        streak[up | down] = 0
        new = torch.where(up, (level + 1).clamp(max=cur.max_level), torch.where(down, (level - 1).clamp(min=cur.min_level), level))
        hold |= new != level
        state["level"] = new
        host.set_param_v(L.PARAM_CURRICULUM, new)

    def timed(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1000.0 / reps      # microseconds per call

    for e in (plain, attached, host):
        e.reset()
    warm = act[args.blocks]
    # code objects and the pace calibration; the host arm's warm steps move its levels, so the attached handle takes the same steps
    timed(lambda: plain.step(warm), 50), timed(lambda: attached.step(warm), 50), timed(lambda: host_step(warm), 50)
    t_plain, t_attached, t_host = [], [], []
    for k in range(args.blocks):                         # interleaved: other work shares the machine
        x = act[k]
        t_plain.append(timed(lambda: plain.step(x), args.steps))
        t_attached.append(timed(lambda: attached.step(x), args.steps))
        t_host.append(timed(lambda: host_step(x), args.steps))
    torch.cuda.synchronize()
    levels = attached.curriculum_levels().cpu()
    same_levels = bool((levels == state["level"].to(torch.int32)).all())
    episodes = float(totals[:, 0].sum())
    done, info = attached.done.clone(), attached.info.clone()
    spare = VecEnv(args.env_id, n, device=0, seed=0)      # the launch alone, on a handle whose levels nothing else reads
    spare.set_curriculum(cur)
    timed(lambda: spare.curriculum_apply(done, info), 50)
    t_launch = [timed(lambda: spare.curriculum_apply(done, info), 1000) for _ in range(args.blocks)]
    med = lambda v: float(np.median(v))
    spread = lambda v: float(np.max(v) - np.min(v))
    out = {"env_id": args.env_id, "envs": n, "curriculum": cur.as_dict(), "steps_per_block": args.steps, "blocks": args.blocks,
           "step_us": {"median": med(t_plain), "spread": spread(t_plain)},
           "step_with_curriculum_launch_us": {"median": med(t_attached), "spread": spread(t_attached)},
           "step_with_host_recipe_us": {"median": med(t_host), "spread": spread(t_host)},
           "curriculum_launch_arm_us": med(t_attached) - med(t_plain),
           "host_recipe_arm_us": med(t_host) - med(t_plain),
           "curriculum_launch_us": {"median": med(t_launch), "spread": spread(t_launch), "done_envs_of_the_timed_launch": int((done != 0).sum())},
           "episodes_judged": episodes, "levels_after_the_blocks": np.bincount(levels.numpy(), minlength=10).tolist(),
           "same_levels_as_the_host_recipe": same_levels,
           "kernel_info": plain.kernel_info()}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for e in (plain, attached, host, spare):
        e.close()


if __name__ == "__main__":
    main()
