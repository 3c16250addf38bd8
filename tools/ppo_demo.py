#!/usr/bin/env python3
"""A whole PPO run on the drop-in surface, on one MI355X: does a user of the reference who switches to `trainer_api.make_vec_envs` get an env
that LEARNS, and what does the step kernel cost on the workload a trained policy produces (VERDICT r5 Weak 5)?

Plain PPO in the pytorch-a2c-ppo-acktr mould the reference's trainers (README.md:33-39) follow -- Gaussian MLP policy 2 x 256 tanh, separate value
net, GAE(0.95), clipped surrogate, Adam, running observation normalisation -- with everything on the device: the step kernel writes observation /
reward / masks / bad_masks straight into the rollout storage (`step(action, into=...)`), Monitor's statistics come from `envs.episode_totals`.
No curriculum unless asked for (--curriculum K, --adaptive-curriculum ..): this is a sanity run, not SymmetricRL; --symmetric gives it SymmetricRL's symmetric network, --mirror-loss its symmetry loss,
--mirror-dup its duplicated tuples.

  python tools/ppo_demo.py [--env-id Walker3DCustomEnv-v0] [--envs 4096] [--steps 32] [--iters 400] [--minutes 12] [--out gpurun_out/r06_ppo_demo]
                           [--device-policy [--device-returns [--device-grad [--device-update]]]] [--symmetric | --mirror-loss COEF | --mirror-dup]
                           [--base-controller FILE] [--height-scan NX,NY] [--depth-camera W,H]
                           [--distill-from TEACHER.npz --privileged-scan NX,NY] [--privileged-critic --privileged-scan NX,NY]
                           [--rand-strength LO,HI] [--rand-latency LO,HI] [--rand-push INTERVAL,MAX] [--obs-noise SCALE] [--rand-privileged]
                           [--history K[,S]] [--curriculum K | --adaptive-curriculum PROMOTE,DEMOTE[,PATIENCE] [--curriculum-recycle]]
--base-controller FILE (required for the planner ids, Walker3DPlannerEnv-v0 / MikePlannerEnv-v0): ALLSTEPS's second step.  FILE is a
`BaseController.save_npz` file or the <out>_policy.npz of an earlier run of this script on a Stepper id (told apart by the keys; the latter
brings its observation statistics along); it is frozen as the env's base controller and the policy trained here emits 15-number plans.
Every --device-* flag works: collection is then `act_plan_step`, policy -> base controller -> step, three launches per step.
--height-scan NX,NY: the observation row becomes [obs | scan], a `perception.scan_grid` of NX x NY terrain heights over 0 .. 2 m ahead and
-0.5 .. 0.5 m sideways, through `make_vec_envs(height_scan=...)`: a planner that cannot see the height field has nothing to plan on.
--depth-camera W,H: an egocentric depth image of W x H pixels is appended, [obs | depth] or [obs | scan | depth]: a `perception.DepthCamera` on
the base, 0.15 m ahead of and 0.10 m above its origin, pitched 35 degrees down, 90 degrees of vertical field, 0.05 .. 6 m, rigidly mounted and
blind to the robot's own links, through `make_vec_envs(depth_camera=...)`.  Rows wider than the device policy's 336 inputs are refused.
--device-policy: collection runs through `envs.act_step(obs[t], into=...)` -- the policy kernel (normalisation, both nets, the sample, its
log-probability, the value) and the step kernel, two launches per step and no torch op; `envs.update_policy(flat)` once per iteration hands the
kernel the optimiser's new weights and the running observation statistics.  The noise then comes from the kernel, not from torch.randn.
--device-returns (with --device-policy): what follows collection runs on the device too.  value[T] comes from the policy kernel
(`envs.venv.act(obs[T], deterministic=True)`), returns, advantages and their normalisation from `envs.finish_rollout` (two launches instead of
the Python loop over t), and the running observation statistics from `envs.update_obs_stats`, which sees EVERY observation of the rollout
(rows 1 .. T) and writes mean and 1 / sqrt(var + eps) straight into the tail of the flat parameter tensor; that tensor is allocated once and
only its head is refreshed from the optimiser's parameters.
--device-grad (with --device-returns): learning runs on the device as well.  The parameters live in ONE flat tensor in
`DevicePolicy.flat_params()`'s order (the nn.Linear weights are views into it); each minibatch is one `envs.ppo_grad` on the raw rollout
storage and the `perm` chunk -- evaluate_actions, the clipped surrogate, the value loss and backward() in four launches --, the global-norm
clip scales the gradient by its own `stats[5]`, torch.optim.Adam steps the flat parameter and `envs.update_policy(flat)` follows every step.
--device-update (with --device-grad): the whole learn block is ONE call, `envs.ppo_update` on the flat tensor -- per epoch a shuffle on the
device, per minibatch the gradient, the global-norm clip, Adam's step (`rollout.AdamState` holds the moments and the step count on the device)
and the repack --; no torch.randperm, no torch.optim.Adam, nothing read on the host.  --fixed-std keeps log_std out through `n_params`.
--symmetric: the policy is the mirror-symmetric network built from the env's get_mirror_indices() (`symmetry.SymmetricGaussian` over the same
`pi`, `vf` and `log_std`): it serves the torch update, torch collection and --verify-grad; with --device-policy the attached policy carries
`envs.symmetric_policy(...)`'s mirror tables, and with --device-grad each minibatch is one symmetric `ppo_grad` (mocca_ppo_grad_sym).
--mirror-loss COEF (not with --symmetric): SymmetricRL's mirror-symmetry loss, COEF * `symmetry.mirror_loss` = COEF * mean((pi(n(s)) -
M_a pi(n(M_o s)))^2) over the env's get_mirror_indices(), added to the plain policy's loss; the logged lines carry `mirror_loss`, the
iteration's mean of the term over its minibatches, and COEF 0 logs the asymmetry of an unconstrained run.  The torch update adds it through
autograd; with --device-grad / --device-update `envs.set_policy_mirror_loss` attaches the tables and the weight, each minibatch's gradient is
mocca_ppo_grad_mirror and the term is its stats[7].  Collection stays the plain policy's: one forward pass per step.
--mirror-dup (not with --symmetric or --mirror-loss): SymmetricRL's duplicated tuples, the plain policy trained on every minibatch row AND
its mirror image (M_o s, M_a a) with the row's own old_logp, advantage and return -- 2 B samples per minibatch.  The torch update builds them
with `symmetry.duplicate_minibatch`; with --device-grad / --device-update `envs.set_policy_mirror_dup` attaches the tables and each
minibatch's gradient is mocca_ppo_grad_dup on the B rows as they lie.  The logged lines carry `mirror_loss`, `symmetry.mirror_loss` of the
current actor on the rollout's first row of observations (computed at logged iterations only, never trained on), and `twin_dlogp`, the mean
since the last logged line of stats[7]: the twins' share of mean(old_logp - logp), how far off-policy the policy's asymmetry puts them.
--distill-from TEACHER.npz --privileged-scan NX,NY (with --device-update; used with --depth-camera W,H): teacher-student distillation
(DAgger) in place of PPO.  TEACHER.npz is the <out>_policy.npz of a run with --height-scan NX,NY: it is frozen in the handle's teacher slot
(`envs.attach_teacher`) and reads `envs.privileged`, the row [obs | scan] that `make_vec_envs(privileged_scan=...)` keeps beside the student's
own row, which stays [obs | depth].  The student collects with its own noise through `act_step`; after every step `envs.teacher_targets` stores
the teacher's mean and value of the state reached beside the row, one more launch; the iteration's learning is ONE `envs.distill_update` --
the regression of the student's mean onto the teacher's, with the teacher's value as the critic's target -- and the logged lines carry `L_d`,
the mean squared error of the actor's mean over the iteration's minibatches.  log_std takes no gradient from the regression: it starts at the
teacher's and stays there.
--privileged-critic --privileged-scan NX,NY (not with --distill-from or a symmetry method): PPO with an asymmetric actor-critic.  The actor
reads the observation row as ever ([obs | depth] with --depth-camera W,H); the critic reads `envs.privileged`, the row [obs | scan] that
`make_vec_envs(privileged_scan=...)` keeps beside it, under running statistics of its own.  The critic only exists while training, so nothing
privileged reaches the policy that is saved.  The rollout storage gains `critic_obs` [T + 1][N][obs + scan], one copy per step from
`envs.privileged` (counted in the reported rate).  Every arm builds the critic on those rows: the torch update and --verify-grad evaluate
`vf` on them, --device-policy attaches an asymmetric `DevicePolicy` (`attach_policy` binds `envs.privileged` for the critic's workgroups),
--device-returns keeps a second `ObsStats` that writes into the longer tail of the flat tensor, and --device-grad / --device-update pass
`critic_obs=` (mocca_ppo_grad_priv / mocca_ppo_update_priv).  <out>_policy.npz also holds `critic_obs_mean` / `critic_obs_var`.
--rand-strength LO,HI / --rand-latency LO,HI / --rand-push INTERVAL,MAX / --obs-noise SCALE: domain randomisation on the device through
`make_vec_envs(randomisation=Randomisation(...))` -- every episode draws its motor strength in [LO, HI] and its action latency of LO .. HI
steps, every INTERVAL steps the base is pushed by up to MAX m/s, and uniform noise of half-width SCALE is added to the policy's row (the
critic's privileged row stays clean).  Every arm works: the randomisation acts on what the step kernel reads and writes, whoever produced the
action.  --rand-privileged (with --privileged-critic): the privileged row becomes [obs | scan | record], the critic knows the plant.
<out>_policy.npz records the randomisation the policy was trained under (`randomisation`, a JSON string).
--history K[,S]: the observation-action history through `make_vec_envs(history=History(K, S))`, all observation columns plus the actions: the
policy's row ends in the K pairs [obs | action] it read and output S, 2 S, .. K S steps ago (newest first; include/mocca.h mocca_history), so
that the actor can tell the plant it has from what its commands did.  Every arm works (the row is just wider; --symmetric takes the env's
extended mirror tables); not with --mirror-loss / --mirror-dup, whose torch side mirrors with get_mirror_indices() alone.
<out>_policy.npz records the history (`history`, a JSON string): tools/randomisation_eval.py rebuilds the env with it.
--curriculum K (Stepper ids): every env on the terrain of level K (`set_env_params({"curriculum": K})`), fixed for the run.
--adaptive-curriculum PROMOTE,DEMOTE[,PATIENCE] (Stepper ids; not with --curriculum): ALLSTEPS's curriculum, per env and on the device, through
`make_vec_envs(curriculum=Curriculum(PROMOTE, DEMOTE, PATIENCE))` -- an episode that ends with steps_reached >= PROMOTE is a success, one with
<= DEMOTE a failure, PATIENCE (default 1) of either in a row move that env one level up or down; the rule is one small launch behind every
step (include/mocca.h mocca_set_curriculum), so the collection loop stays free of host reads.  --curriculum-recycle: an env promoted at level
9 restarts at a level drawn from 0 .. 9.  Each logged line gains `mean_level` and `level_episodes`, the episodes judged at each level since
the last line (`envs.curriculum_totals`, read and zeroed at log time).  <out>_policy.npz records the curriculum (`curriculum`, a JSON string).
--verify-grad also runs the autograd path on the first minibatch of each iteration and prints the largest difference, scaled per tensor
(--mirror-dup: on that minibatch's rows whose ratio and whose twin's ratio lie more than 1e-4 from the clip bounds, where the surrogate's
gradient jumps and two float32 evaluations may disagree on a sample's side; the twins' ratios are spread over the bounds); with
--device-update, whose minibatches are drawn on the device, it takes one `envs.ppo_grad` on a torch.randperm chunk ahead of the update.
writes <out>.jsonl (one line per logged iteration: env-steps so far, mean episode return / length of the episodes that ended since the last line,
wall-clock env-steps/s of the whole loop incl. learning) and <out>_policy.npz (weights + observation statistics: `bench.py`'s workload
bracket loads profiles/ppo_policy_walker3d.npz as its `ppo_policy` workload)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-id", default="Walker3DCustomEnv-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=32, help="rollout length T")
    ap.add_argument("--iters", type=int, default=100000)
    ap.add_argument("--minutes", type=float, default=12.0, help="stop after this much wall-clock")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-std", type=float, default=-1.0, help="initial log of the action noise's standard deviation")
    ap.add_argument("--fixed-std", action="store_true", help="keep the action noise fixed (the policy cannot collapse onto standing still)")
    ap.add_argument("--out", default="gpurun_out/r06_ppo_demo")
    ap.add_argument("--device-policy", action="store_true", help="collect with the policy on the device (act_step)")
    ap.add_argument("--device-returns", action="store_true", help="GAE, advantage normalisation and observation statistics on the device (finish_rollout, update_obs_stats)")
    ap.add_argument("--verify-returns", action="store_true", help="with --device-returns: also run the torch GAE loop on the same storage and insist on the same bits")
    ap.add_argument("--device-grad", action="store_true", help="with --device-returns: each minibatch's loss and gradient on the device (ppo_grad); the parameters live in one flat tensor")
    ap.add_argument("--device-update", action="store_true", help="with --device-grad: the whole update -- shuffle, gradient, clip, Adam, repack for every epoch and minibatch -- as one call (ppo_update)")
    ap.add_argument("--symmetric", action="store_true", help="SymmetricRL's symmetric network: mean, value and log_std symmetrised through the env's mirror tables")
    ap.add_argument("--mirror-loss", type=float, default=None, metavar="COEF", help="SymmetricRL's mirror-symmetry loss with this weight (0: only logged); not with --symmetric")
    ap.add_argument("--mirror-dup", action="store_true", help="SymmetricRL's duplicated tuples: train on every row and its mirror image; not with --symmetric or --mirror-loss")
    ap.add_argument("--base-controller", default=None, metavar="FILE", help="the planner ids' frozen base controller: a BaseController.save_npz file or this script's policy file of a Stepper run")
    ap.add_argument("--height-scan", default=None, metavar="NX,NY", help="append a scan_grid of NX x NY terrain heights (0 .. 2 m ahead, -0.5 .. 0.5 m sideways) to the observation row")
    ap.add_argument("--depth-camera", default=None, metavar="W,H", help="append a W x H depth image from a forward camera on the base, pitched 35 degrees down, to the observation row")
    ap.add_argument("--terrain-bank", type=int, default=0, metavar="K", help="planner ids: train on a bank of K random height fields generated on the device, another one in every episode (0: the shipped map)")
    ap.add_argument("--terrain-seed", type=int, default=0, metavar="S", help="seed of the terrain bank")
    ap.add_argument("--terrain-refresh", type=int, default=0, metavar="M", help="regenerate the bank every M iterations with seed S + iteration (0: never)")
    ap.add_argument("--terrain-gain", type=float, default=1.0, metavar="G", help="the generated fields are multiplied by G: the difficulty knob")
    ap.add_argument("--distill-from", default=None, metavar="TEACHER.npz", help="with --device-update: distil this frozen teacher (the policy file of a --height-scan run) into the student instead of PPO")
    ap.add_argument("--privileged-scan", default=None, metavar="NX,NY", help="with --distill-from: the teacher's scan_grid, kept beside the observation row (envs.privileged), never in it")
    ap.add_argument("--privileged-critic", action="store_true", help="with --privileged-scan: PPO whose critic reads envs.privileged ([obs | scan]) while the actor reads the observation row")
    ap.add_argument("--rand-strength", default=None, metavar="LO,HI", help="each episode draws its motor strength in [LO, HI], 0 < LO <= HI <= 1")
    ap.add_argument("--rand-latency", default=None, metavar="LO,HI", help="each episode draws its action latency of LO .. HI steps (at most 7)")
    ap.add_argument("--rand-push", default=None, metavar="INTERVAL,MAX", help="every INTERVAL steps the base's velocity jumps by up to MAX m/s along x and y")
    ap.add_argument("--obs-noise", type=float, default=None, metavar="SCALE", help="uniform noise of this half-width on every column of the policy's observation row")
    ap.add_argument("--rand-privileged", action="store_true", help="with --privileged-critic: the plant's record joins the critic's row, [obs | scan | record]")
    ap.add_argument("--history", default=None, metavar="K[,S]", help="append the last K (observation, action) pairs, S steps apart (default 1), to the policy's row")
    ap.add_argument("--curriculum", type=int, default=None, metavar="K", help="Stepper ids: every env on the terrain of level K, 0 .. 9")
    ap.add_argument("--adaptive-curriculum", default=None, metavar="PROMOTE,DEMOTE[,PATIENCE]", help="Stepper ids: every env's own episodes move its own level on the device")
    ap.add_argument("--curriculum-recycle", action="store_true", help="with --adaptive-curriculum: an env promoted at level 9 restarts at a level drawn from 0 .. 9")
    ap.add_argument("--verify-grad", action="store_true", help="with --device-grad: also run the autograd path on the first minibatch of each iteration and print the largest scaled difference")
    args = ap.parse_args(argv)
    if args.device_grad and not args.device_returns:
        ap.error("--device-grad requires --device-returns")
    if args.device_update and not args.device_grad:
        ap.error("--device-update requires --device-grad")
    if args.mirror_loss is not None and args.symmetric:
        ap.error("--mirror-loss is not for --symmetric: a symmetric network has no mirror loss")
    if args.mirror_loss is not None and not args.mirror_loss >= 0.0:
        ap.error("--mirror-loss takes a weight >= 0")
    if args.mirror_dup and (args.symmetric or args.mirror_loss is not None):
        ap.error("--mirror-dup is not for --symmetric or --mirror-loss: one symmetry method at a time")
    if args.verify_grad and not args.device_grad:
        ap.error("--verify-grad requires --device-grad")
    if args.device_returns and not args.device_policy:
        ap.error("--device-returns requires --device-policy")
    if args.verify_returns and not args.device_returns:
        ap.error("--verify-returns requires --device-returns")
    planner = "Planner" in args.env_id
    if planner != (args.base_controller is not None):
        ap.error("--base-controller is required for the planner ids, and only for them")
    if planner and (args.symmetric or args.mirror_loss is not None or args.mirror_dup):
        ap.error("the planner ids publish no mirror indices for plans: no --symmetric / --mirror-loss / --mirror-dup")
    if args.terrain_bank and not planner:
        ap.error("--terrain-bank is for the planner ids: the other tasks have no height field")
    if args.terrain_refresh and not args.terrain_bank:
        ap.error("--terrain-refresh requires --terrain-bank")
    if args.distill_from is not None and not args.device_update:
        ap.error("--distill-from requires --device-update")
    if args.distill_from is not None and (args.symmetric or args.mirror_loss is not None or args.mirror_dup or args.verify_grad):
        ap.error("--distill-from is not for --symmetric / --mirror-loss / --mirror-dup / --verify-grad: the regression gradient is the plain policy's")
    if args.privileged_scan is not None and ((args.distill_from is None and not args.privileged_critic) or args.height_scan is not None):
        ap.error("--privileged-scan goes with --distill-from or --privileged-critic and not with --height-scan")
    if args.privileged_critic and (args.privileged_scan is None or args.distill_from is not None or args.symmetric or args.mirror_loss is not None
                                   or args.mirror_dup):
        ap.error("--privileged-critic requires --privileged-scan and is not for --distill-from / --symmetric / --mirror-loss / --mirror-dup")
    if args.rand_privileged and not args.privileged_critic:
        ap.error("--rand-privileged requires --privileged-critic: the record is the tail of the critic's row")
    if (args.curriculum is not None or args.adaptive_curriculum is not None) and "Stepper" not in args.env_id:
        ap.error("--curriculum / --adaptive-curriculum are for the Stepper ids: the other tasks have no curriculum levels")
    if args.curriculum is not None and (args.adaptive_curriculum is not None or not 0 <= args.curriculum <= 9):
        ap.error("--curriculum takes a level 0 .. 9 and is not for --adaptive-curriculum, which moves the levels itself")
    if args.curriculum_recycle and args.adaptive_curriculum is None:
        ap.error("--curriculum-recycle requires --adaptive-curriculum")
    import torch
    import torch.nn as nn
    from mocca_envs_amd.trainer_api import make_vec_envs
    torch.manual_seed(args.seed)
    extra = {}
    cur = None
    if args.adaptive_curriculum is not None:
        from mocca_envs_amd.curriculum import Curriculum
        cur = Curriculum(*(int(v) for v in args.adaptive_curriculum.split(",")), recycle=args.curriculum_recycle)
        extra["curriculum"] = cur
    rand = None
    if any(v is not None for v in (args.rand_strength, args.rand_latency, args.rand_push, args.obs_noise)) or args.rand_privileged:
        from mocca_envs_amd.randomisation import Randomisation
        pair = lambda text, kind, default: default if text is None else tuple(k(v) for k, v in zip(kind, text.split(",")))
        rand = Randomisation(strength=pair(args.rand_strength, (float, float), (1.0, 1.0)), latency=pair(args.rand_latency, (int, int), (0, 0)),
                             push=pair(args.rand_push, (int, float), (0, 0.0)), obs_noise=args.obs_noise, privileged=args.rand_privileged)
        extra["randomisation"] = rand
    hist = None
    if args.history is not None:
        if args.mirror_loss is not None or args.mirror_dup:
            ap.error("--history is not for --mirror-loss / --mirror-dup: their torch side mirrors with get_mirror_indices() alone")
        from mocca_envs_amd.history import History
        hist = History(*(int(v) for v in args.history.split(",")))
        extra["history"] = hist
    if args.base_controller is not None:
        from mocca_envs_amd.controller import BaseController
        extra["base_controller"] = BaseController.load(args.base_controller)
    if args.height_scan is not None:
        from mocca_envs_amd.perception import scan_grid
        nx, ny = (int(v) for v in args.height_scan.split(","))
        extra["height_scan"] = dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), nx, ny))
    if args.privileged_scan is not None:
        from mocca_envs_amd.perception import scan_grid
        nx, ny = (int(v) for v in args.privileged_scan.split(","))
        extra["privileged_scan"] = dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), nx, ny))
    if args.depth_camera is not None:
        from mocca_envs_amd.perception import DepthCamera
        cw, ch = (int(v) for v in args.depth_camera.split(","))
        extra["depth_camera"] = DepthCamera(offset=(0.15, 0.0, 0.10), pitch=-35.0, fov_y=90.0, near=0.05, far=6.0, width=cw, height=ch)
    if args.terrain_bank:
        extra["terrain_bank"] = dict(n_fields=args.terrain_bank, seed=args.terrain_seed, gain=args.terrain_gain, redraw_at_reset=True)
    envs = make_vec_envs(args.env_id, seed=args.seed, num_processes=args.envs, record_events=False, **extra)
    if args.curriculum is not None:
        envs.set_env_params({"curriculum": args.curriculum})      # (before the first reset, which lays the terrain out)
    dev, N, T = envs.device, args.envs, args.steps
    od, ad = envs.observation_space.shape[0], envs.action_space.shape[0]
    if (args.depth_camera is not None or hist is not None) and od > 336:
        raise SystemExit(f"--depth-camera {args.depth_camera} / --history {args.history}: the observation row would have {od} entries, the policy kernel takes at most 336")

    def mlp(i, o, gain):
        net = nn.Sequential(nn.Linear(i, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, o)).to(dev)
        for m in net:
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight, 2 ** 0.5); nn.init.zeros_(m.bias)
        nn.init.orthogonal_(net[-1].weight, gain)
        return net

    PC = args.privileged_critic
    oc = envs.privileged.shape[1] if PC else od      # what the critic reads: [obs | scan], or the actor's row
    pi, vf = mlp(od, ad, 0.01), mlp(oc, 1, 1.0)
    log_std = nn.Parameter(torch.full((ad,), args.log_std, device=dev), requires_grad=not args.fixed_std)
    if args.distill_from is not None:      # the regression gives log_std no gradient: the student explores with the teacher's noise throughout
        import numpy as np
        with np.load(args.distill_from, allow_pickle=False) as z:
            log_std.data.copy_(torch.from_numpy(z["log_std"]).to(dev))
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + ([] if args.fixed_std else [log_std]), lr=args.lr, eps=1e-5)
    # rollout storage, a2c-ppo-acktr's layout; the step kernel writes rows t + 1 / t of obs, rewards, masks, bad_masks itself
    S = {"obs": torch.zeros(T + 1, N, od, device=dev), "reward": torch.zeros(T, N, 1, device=dev), "masks": torch.ones(T + 1, N, 1, device=dev),
         "bad_masks": torch.ones(T + 1, N, 1, device=dev), "act": torch.zeros(T, N, ad, device=dev), "logp": torch.zeros(T, N, 1, device=dev),
         "value": torch.zeros(T + 1, N, 1, device=dev)}
    row = lambda t: {"obs": S["obs"][t + 1], "reward": S["reward"][t], "masks": S["masks"][t + 1], "bad_masks": S["bad_masks"][t + 1]}
    mean, var, count = torch.zeros(od, device=dev), torch.ones(od, device=dev), 1e-4
    norm = lambda o: ((o - mean) / torch.sqrt(var + 1e-8)).clamp(-10.0, 10.0)
    cnorm = norm      # the critic's normalisation; --privileged-critic: of its own rows, under its own statistics
    if PC:
        S["critic_obs"] = torch.zeros(T + 1, N, oc, device=dev)
        cmean, cvar = torch.zeros(oc, device=dev), torch.ones(oc, device=dev)
        cnorm = lambda o: ((o - cmean) / torch.sqrt(cvar + 1e-8)).clamp(-10.0, 10.0)
    ckw = lambda: {"critic_obs": S["critic_obs"][:T]} if PC else {}      # what ppo_grad / ppo_update take beside the storage

    def logprob(mu, a):
        return (-0.5 * ((a - mu) / log_std.exp()) ** 2 - log_std - 0.9189385332046727).sum(-1, keepdim=True)

    if args.symmetric:
        from mocca_envs_amd.policy import DevicePolicy
        from mocca_envs_amd.symmetry import SymmetricGaussian
        tables = envs.symmetric_policy(DevicePolicy.from_torch(pi, vf, log_std)).symmetry
        sym = SymmetricGaussian(pi, vf, log_std, tables).to(dev)      # shares pi, vf and log_std
        inv_std_now = lambda: inv_std if args.device_returns else 1.0 / torch.sqrt(var + 1e-8)

    if args.mirror_loss is not None:
        from mocca_envs_amd.symmetry import MirrorTransform, mirror_loss
        mirror_tf = MirrorTransform(envs.get_mirror_indices(), od, ad, device=dev)
        lm_sum, lm_n = torch.zeros((), device=dev), 0      # the term over the minibatches since the last logged line

    if args.mirror_dup:
        from mocca_envs_amd.symmetry import MirrorTransform, duplicate_minibatch, mirror_loss
        mirror_tf = MirrorTransform(envs.get_mirror_indices(), od, ad, device=dev)
        td_sum, td_n = torch.zeros((), device=dev), 0      # stats[7] over the minibatches since the last logged line

    def aux_loss(mb):
        """what --mirror-loss adds to the minibatch's loss -> (COEF * L_m or 0, L_m or None); the mirror acts on the RAW rows"""
        if args.mirror_loss is None:
            return 0.0, None
        l_m = mirror_loss(lambda x: pi(norm(x)), raw_all[mb], mirror_tf)
        return args.mirror_loss * l_m, l_m

    def minibatch(mb):
        """(old_logp, adv, returns) of the minibatch, [b, 1] each; --mirror-dup: of its 2 b samples, the twins carrying their rows' own"""
        if args.mirror_dup:
            return duplicate_minibatch(raw_all[mb], a_all[mb], lp_all[mb], adv_all[mb], ret_all[mb], None, mirror_tf)[2:5]
        return lp_all[mb], adv_all[mb], ret_all[mb]

    def evaluate(mb):
        """(logp [b, 1], value [b, 1]) of the minibatch's stored actions under the current parameters; --mirror-dup: [2 b, 1], the rows then
        their mirror images, mirrored on the RAW rows"""
        if args.mirror_dup:
            o2, a2 = duplicate_minibatch(raw_all[mb], a_all[mb], lp_all[mb], adv_all[mb], ret_all[mb], None, mirror_tf)[:2]
            return logprob(pi(norm(o2)), a2), vf(norm(o2))
        if args.symmetric:      # the mirror acts on the RAW row
            lp, _, v = sym.evaluate_actions(raw_all[mb], a_all[mb], mean, inv_std_now(), 10.0)
            return lp.unsqueeze(-1), v.unsqueeze(-1)
        return logprob(pi(o_all[mb]), a_all[mb]), vf(c_all[mb])

    if args.device_policy:
        from mocca_envs_amd.policy import DevicePolicy
        dp = DevicePolicy.from_torch(pi, vf, log_std, obs_mean=mean, obs_var=var, eps=1e-8, clip=10.0,
                                     **(dict(critic_obs_mean=cmean, critic_obs_var=cvar) if PC else {}))
        envs.attach_policy(envs.symmetric_policy(dp) if args.symmetric else dp)
        if args.mirror_loss is not None and args.device_grad:      # for the gradient only: act_step keeps running the plain policy
            envs.set_policy_mirror_loss(envs.policy_mirror_tables(dp), args.mirror_loss)
        if args.mirror_dup and args.device_grad:      # likewise
            envs.set_policy_mirror_dup(envs.policy_mirror_tables(dp))
        row_act = lambda t: dict(row(t), action=S["act"][t], logp=S["logp"][t], value=S["value"][t])
        if args.distill_from is not None:      # the frozen teacher; its labels of the state in obs[t] lie in row t beside it
            envs.attach_teacher(DevicePolicy.from_npz(args.distill_from))
            S["t_mean"], S["t_value"] = torch.zeros(T + 1, N, ad, device=dev), torch.zeros(T + 1, N, 1, device=dev)
            ld_sum, ld_n = torch.zeros((), device=dev), 0      # L_d over the minibatches since the last logged line
        # DevicePolicy.flat_params()'s order, built on the device: layers of pi then vf (W, b), log_std, mean, 1 / sqrt(var + eps)
        flat_params = lambda: torch.cat([q.reshape(-1) for net in (pi, vf) for m in net if isinstance(m, nn.Linear) for q in (m.weight, m.bias)]
                                        + [log_std, mean, 1.0 / torch.sqrt(var + 1e-8)] + ([cmean, 1.0 / torch.sqrt(cvar + 1e-8)] if PC else []))

    if args.device_returns:
        from mocca_envs_amd.rollout import ObsStats
        stats = ObsStats(od, dev, eps=1e-8)
        head = [q for net in (pi, vf) for m in net if isinstance(m, nn.Linear) for q in (m.weight, m.bias)] + [log_std]
        n_head = sum(q.numel() for q in head)
        flat = torch.zeros(n_head + 2 * od + (2 * oc if PC else 0), device=dev)      # DevicePolicy.flat_params()'s order; allocated once
        mean, inv_std = flat[n_head:n_head + od], flat[n_head + od:n_head + 2 * od]      # the statistics tail: update_obs_stats writes it
        norm = lambda o: ((o - mean) * inv_std).clamp(-10.0, 10.0)       # the policy kernel's formula
        cnorm = norm
        if PC:      # the critic's statistics: a second ObsStats over the privileged rows, into the longer tail
            stats_c = ObsStats(oc, dev, eps=1e-8)
            cmean, cinv_std = flat[n_head + 2 * od:n_head + 2 * od + oc], flat[n_head + 2 * od + oc:]
            cnorm = lambda o: ((o - cmean) * cinv_std).clamp(-10.0, 10.0)
        adv_buf, ret_buf = torch.zeros(T, N, 1, device=dev), torch.zeros(T, N, 1, device=dev)

    if args.device_grad:
        # the parameters live in ONE flat tensor, flat[:n_head]; the modules' weights are views into it (for saving and --verify-grad)
        with torch.no_grad():
            torch.cat([q.reshape(-1) for q in head], out=flat[:n_head])
        pos = 0
        for q in head:
            q.data = flat[pos:pos + q.numel()].view_as(q)
            pos += q.numel()
        if args.device_update:
            from mocca_envs_amd.rollout import AdamState
            adam = AdamState(n_head, dev)      # the optimiser's state lives on the device
            u_stats = torch.zeros(args.epochs * args.minibatches, 8, device=dev)
        else:
            w_flat = flat[:n_head].requires_grad_()
            opt = torch.optim.Adam([w_flat], lr=args.lr, eps=1e-5)
        g_buf, s_buf = torch.zeros(n_head, device=dev), torch.zeros(8, device=dev)

    def off_the_clip_bounds(mb):
        """--mirror-dup: the rows of `mb` whose ratio and whose twin's ratio both lie more than 1e-4 from 1 - clip and 1 + clip.  The
        surrogate's gradient jumps there, and two float32 evaluations may put a sample on either side: --verify-grad compares the two
        gradients on the rows where the loss is differentiable, as the checkers of tests/ do by construction.  A plain minibatch's ratios
        are all 1 +- 1e-6 at the first minibatch; the twins' are spread over the bounds by the policy's asymmetry."""
        with torch.no_grad():
            r = (evaluate(mb)[0] - minibatch(mb)[0]).exp().reshape(2, -1)
            near = ((r - (1 - args.clip)).abs() < 1e-4) | ((r - (1 + args.clip)).abs() < 1e-4)
        return mb[~near.any(0)]

    def verify_grad(mb, it):
        """g_buf holds ppo_grad's gradient of minibatch `mb` at the current parameters: print its largest difference from autograd"""
        lp, v = evaluate(mb)
        lp_old, adv_mb, ret_mb = minibatch(mb)
        ratio = (lp - lp_old).exp()
        surr = torch.min(ratio * adv_mb, ratio.clamp(1 - args.clip, 1 + args.clip) * adv_mb).mean()
        v_loss = 0.5 * (v - ret_mb).pow(2).mean()
        auto = torch.autograd.grad(-surr + 0.5 * v_loss + aux_loss(mb)[0], head[:-1] if args.fixed_std else head)      # (vf on the critic's rows: evaluate)
        worst, pos = 0.0, 0
        for g in auto:
            worst = max(worst, ((g_buf[pos:pos + g.numel()] - g.reshape(-1)).abs().max() / g.abs().max().clamp_min(1e-30)).item())
            pos += g.numel()
        print(json.dumps({"verify_grad": worst, "iter": it + 1}), flush=True)

    S["obs"][0].copy_(envs.reset())
    if PC:
        S["critic_obs"][0].copy_(envs.privileged)
    if args.distill_from is not None:
        envs.teacher_targets(S["t_mean"][0], S["t_value"][0])
    envs.episode_totals.zero_()
    log = open(args.out + ".jsonl", "w")
    t_start, total_steps, last_tot = time.perf_counter(), 0, torch.zeros(4, device=dev)
    for it in range(args.iters):
        if args.terrain_refresh and it and it % args.terrain_refresh == 0:
            envs.refresh_terrain(args.terrain_seed + it)     # on the stream of the steps around it: no synchronise
        # ---- collect
        if args.device_returns:
            with torch.no_grad():
                # the statistics see every observation collected so far: the reset row first, then rows 1 .. T of the previous rollout
                envs.update_obs_stats(stats, S["obs"][1:] if it else S["obs"][:1], mean_out=mean, inv_std_out=inv_std)
                if PC:
                    envs.update_obs_stats(stats_c, S["critic_obs"][1:] if it else S["critic_obs"][:1], mean_out=cmean, inv_std_out=cinv_std)
                if not args.device_grad:
                    torch.cat([q.reshape(-1) for q in head], out=flat[:n_head])
                envs.update_policy(flat)
                for t in range(T):
                    envs.act_step(S["obs"][t], into=row_act(t))      # (--privileged-critic: the value is the critic's on envs.privileged)
                    if PC:      # the critic's row of the state just reached, beside the actor's
                        S["critic_obs"][t + 1].copy_(envs.privileged)
                    if args.distill_from is not None:      # the teacher labels the state the student has just reached
                        envs.teacher_targets(S["t_mean"][t + 1], S["t_value"][t + 1])
                envs.venv.act(S["obs"][T], deterministic=True, out={"value": S["value"][T]})
                if args.verify_returns:
                    raw = envs.finish_rollout(S["reward"], S["value"], S["masks"], S["bad_masks"], args.gamma, args.lam, args.reward_scale, normalise=False)
                    adv_t = torch.zeros(T, N, 1, device=dev)
                    gae = torch.zeros(N, 1, device=dev)
                    rew = S["reward"] * args.reward_scale
                    for t in reversed(range(T)):
                        delta = rew[t] + args.gamma * S["value"][t + 1] * S["masks"][t + 1] - S["value"][t]
                        gae = (delta + args.gamma * args.lam * S["masks"][t + 1] * gae) * S["bad_masks"][t + 1]
                        adv_t[t] = gae
                    same = lambda u, v: bool((u.view(torch.int32) == v.view(torch.int32)).all().item())
                    if not (same(raw["adv"], adv_t) and same(raw["returns"], adv_t + S["value"][:T])):
                        raise SystemExit("finish_rollout differs from the torch GAE loop")
                    print(json.dumps({"verify_returns": "ok", "iter": it + 1}), flush=True)
                fin = envs.finish_rollout(S["reward"], S["value"], S["masks"], S["bad_masks"], args.gamma, args.lam, args.reward_scale,
                                          returns=ret_buf, adv=adv_buf, normalise=True, adv_eps=1e-8)
                adv, ret = fin["adv"], fin["returns"]
        else:
            with torch.no_grad():
                flat = S["obs"][0]
                bm, bv, bn = flat.mean(0), flat.var(0, unbiased=False), flat.shape[0]     # running observation statistics (one row per iteration is enough)
                d = bm - mean
                tot = count + bn
                mean = mean + d * bn / tot
                var = (var * count + bv * bn + d * d * count * bn / tot) / tot
                if PC:      # the same merge over the critic's rows
                    c0 = S["critic_obs"][0]
                    dc = c0.mean(0) - cmean
                    cmean, cvar = cmean + dc * bn / tot, (cvar * count + c0.var(0, unbiased=False) * bn + dc * dc * count * bn / tot) / tot
                count = tot
                if args.device_policy:
                    envs.update_policy(flat_params())
                for t in range(T):
                    if args.device_policy:
                        envs.act_step(S["obs"][t], into=row_act(t))
                        if PC:
                            S["critic_obs"][t + 1].copy_(envs.privileged)
                        continue
                    if args.symmetric:
                        mu, ls, v = sym(S["obs"][t], mean, inv_std_now(), 10.0)
                        eps = torch.randn_like(mu)
                        S["act"][t].copy_(mu + ls.exp() * eps)
                        S["logp"][t].copy_((-0.5 * eps * eps - ls - 0.9189385332046727).sum(-1, keepdim=True)); S["value"][t].copy_(v.unsqueeze(-1))
                        envs.step(S["act"][t], into=row(t))
                        continue
                    o = norm(S["obs"][t])
                    mu = pi(o)
                    a = mu + log_std.exp() * torch.randn_like(mu)
                    S["act"][t].copy_(a); S["logp"][t].copy_(logprob(mu, a)); S["value"][t].copy_(vf(cnorm(S["critic_obs"][t])) if PC else vf(o))
                    envs.step(S["act"][t], into=row(t))
                    if PC:
                        S["critic_obs"][t + 1].copy_(envs.privileged)
                S["value"][T].copy_(sym(S["obs"][T], mean, inv_std_now(), 10.0)[2].unsqueeze(-1) if args.symmetric
                                    else vf(cnorm(S["critic_obs"][T])) if PC else vf(norm(S["obs"][T])))
                # GAE; an episode cut by the TimeLimit (bad_masks = 0) is not bootstrapped through: its advantage stops there (a2c-ppo-acktr's use_proper_time_limits)
                adv = torch.zeros(T, N, 1, device=dev)
                gae = torch.zeros(N, 1, device=dev)
                rew = S["reward"] * args.reward_scale
                for t in reversed(range(T)):
                    delta = rew[t] + args.gamma * S["value"][t + 1] * S["masks"][t + 1] - S["value"][t]
                    gae = (delta + args.gamma * args.lam * S["masks"][t + 1] * gae) * S["bad_masks"][t + 1]
                    adv[t] = gae
                ret = adv + S["value"][:T]
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        total_steps += N * T
        # ---- learn
        B = N * T
        o_all, a_all, lp_all = norm(S["obs"][:T]).reshape(B, od), S["act"].reshape(B, ad), S["logp"].reshape(B, 1)
        adv_all, ret_all, raw_all = adv.reshape(B, 1), ret.reshape(B, 1), S["obs"][:T].reshape(B, od)
        c_all = cnorm(S["critic_obs"][:T]).reshape(B, oc) if PC else o_all      # what vf reads in the torch arms
        if args.distill_from is not None:
            # DAgger's regression as one call: epochs x minibatches of [shuffle, distill_grad, clip, Adam, repack] on the rows the student visited
            envs.distill_update(S["obs"][:T], S["t_mean"][:T], flat, adam, minibatch_rows=B // args.minibatches, epochs=args.epochs,
                                value_target=S["t_value"][:T], distill_coef=1.0, value_coef=0.5, n_params=n_head - ad if args.fixed_std else n_head,
                                lr=args.lr, eps=1e-5, max_grad_norm=0.5, seed=args.seed, stats=u_stats)
            ld_sum += u_stats[:, 7].sum(); ld_n += u_stats.shape[0]
        elif args.device_update:
            if args.verify_grad:      # the update draws its minibatches on the device: one gradient call on a chunk of our own, ahead of it
                mb = torch.randperm(B, device=dev)[:B // args.minibatches]
                if args.mirror_dup:
                    mb = off_the_clip_bounds(mb)
                envs.ppo_grad(S["obs"][:T], S["act"], S["logp"], adv, ret, idx=mb, clip=args.clip, value_coef=0.5, grad=g_buf, stats=s_buf, **ckw())
                verify_grad(mb, it)
            # ppo.update() as one call: epochs x minibatches of [shuffle, ppo_grad, clip, Adam, repack]; u_stats keeps a row per minibatch
            envs.ppo_update(S["obs"][:T], S["act"], S["logp"], adv, ret, flat, adam, minibatch_rows=B // args.minibatches, epochs=args.epochs,
                            clip=args.clip, value_coef=0.5, n_params=n_head - ad if args.fixed_std else n_head, lr=args.lr, eps=1e-5,
                            max_grad_norm=0.5, seed=args.seed, stats=u_stats, **ckw())
            if args.mirror_loss is not None:
                lm_sum += u_stats[:, 7].sum(); lm_n += u_stats.shape[0]
            if args.mirror_dup:
                td_sum += u_stats[:, 7].sum(); td_n += u_stats.shape[0]
        for ep in range(0 if args.device_update else args.epochs):
            perm = torch.randperm(B, device=dev)
            for k, mb in enumerate(perm.chunk(args.minibatches)):
                if args.device_grad:
                    # evaluate_actions, the clipped surrogate, the value loss and backward() as one call on the raw storage (--symmetric: of
                    # the symmetric network -- the attached policy carries the mirror tables)
                    if args.verify_grad and ep == 0 and k == 0 and args.mirror_dup:      # a call of its own on the rows off the clip bounds
                        mb_v = off_the_clip_bounds(mb)
                        envs.ppo_grad(S["obs"][:T], S["act"], S["logp"], adv, ret, idx=mb_v, clip=args.clip, value_coef=0.5, grad=g_buf, stats=s_buf)
                        verify_grad(mb_v, it)
                    envs.ppo_grad(S["obs"][:T], S["act"], S["logp"], adv, ret, idx=mb, clip=args.clip, value_coef=0.5, grad=g_buf, stats=s_buf, **ckw())
                    if args.verify_grad and ep == 0 and k == 0 and not args.mirror_dup:
                        verify_grad(mb, it)
                    with torch.no_grad():
                        if args.mirror_loss is not None:
                            lm_sum += s_buf[7]; lm_n += 1
                        if args.mirror_dup:
                            td_sum += s_buf[7]; td_n += 1
                        sq = s_buf[5]
                        if args.fixed_std:      # log_std is not a parameter then: its entries leave the norm and the step
                            sq = (sq - g_buf[n_head - ad:].square().sum()).clamp(min=0.0)
                            g_buf[n_head - ad:].zero_()
                        g_buf.mul_((0.5 / (sq.sqrt() + 1e-6)).clamp(max=1.0))      # clip_grad_norm_(.., 0.5) from the sum of grad^2
                    w_flat.grad = g_buf
                    opt.step()
                    envs.update_policy(flat)
                    continue
                lp, v = evaluate(mb)
                lp_old, adv_mb, ret_mb = minibatch(mb)
                ratio = (lp - lp_old).exp()
                surr = torch.min(ratio * adv_mb, ratio.clamp(1 - args.clip, 1 + args.clip) * adv_mb).mean()
                v_loss = 0.5 * (v - ret_mb).pow(2).mean()
                if args.mirror_dup:      # what mocca_ppo_grad_dup reports in stats[7]: the twins' sum over the 2 b samples
                    td_sum += (lp_old - lp.detach())[mb.numel():].sum() / (2 * mb.numel()); td_n += 1
                aux, l_m = aux_loss(mb)
                if l_m is not None:
                    lm_sum += l_m.detach(); lm_n += 1
                opt.zero_grad(set_to_none=True)
                (-surr + 0.5 * v_loss + aux).backward()
                nn.utils.clip_grad_norm_(list(pi.parameters()) + list(vf.parameters()) + ([] if args.fixed_std else [log_std]), 0.5)
                opt.step()
        with torch.no_grad():      # rollouts.after_update()
            S["obs"][0].copy_(S["obs"][T]); S["masks"][0].copy_(S["masks"][T]); S["bad_masks"][0].copy_(S["bad_masks"][T])
            if PC:
                S["critic_obs"][0].copy_(S["critic_obs"][T])
            if args.distill_from is not None:
                S["t_mean"][0].copy_(S["t_mean"][T]); S["t_value"][0].copy_(S["t_value"][T])
        if it % 10 == 9 or it == 0:
            tot_now = envs.episode_totals.clone()
            dlt = (tot_now - last_tot).cpu().numpy()
            last_tot = tot_now
            wall = time.perf_counter() - t_start
            line = {"iter": it + 1, "env_steps": total_steps, "wall_s": round(wall, 1), "env_steps_per_s_incl_learning": round(total_steps / wall),
                    "episodes": int(dlt[2]), "mean_return": float(dlt[0] / max(dlt[2], 1)), "mean_length": float(dlt[1] / max(dlt[2], 1)),
                    "truncated_fraction": float(dlt[3] / max(dlt[2], 1)), "log_std": float(log_std.mean().item())}
            if args.mirror_loss is not None:      # the mean of L_m over the minibatches since the last logged line
                line["mirror_loss"] = float(lm_sum.item() / max(lm_n, 1))
                lm_sum.zero_(); lm_n = 0
            if args.mirror_dup:
                with torch.no_grad():      # the asymmetry of the current actor; monitored, never trained on
                    line["mirror_loss"] = float(mirror_loss(lambda x: pi(norm(x)), S["obs"][0], mirror_tf).item())
                line["twin_dlogp"] = float(td_sum.item() / max(td_n, 1))
                td_sum.zero_(); td_n = 0
            if args.distill_from is not None:      # the mean of L_d over the minibatches since the last logged line
                line["L_d"] = float(ld_sum.item() / max(ld_n, 1))
                ld_sum.zero_(); ld_n = 0
            if "Stepper" in args.env_id:      # next_step_index of the running episodes (the step's info word): how far along the 20 planks the batch is
                line["mean_next_step_index"] = float(envs.venv.info.float().mean().item())
            if cur is not None:      # read here, at log time: the collection loop stays free of synchronisation
                line["mean_level"] = float(envs.curriculum_levels.float().mean().item())
                line["level_episodes"] = [int(v) for v in envs.curriculum_totals[:, 0].cpu().numpy()]
                envs.curriculum_totals.zero_()
            elif args.curriculum is not None:
                line["mean_level"] = float(args.curriculum)
            log.write(json.dumps(line) + "\n"); log.flush()
            print(json.dumps(line), flush=True)
            if wall > 60.0 * args.minutes:
                break
    import numpy as np
    if args.device_returns:
        mean, var = stats.mean.float(), stats.var.float()
        if PC:
            cmean, cvar = stats_c.mean.float(), stats_c.var.float()
    extra_stats = dict(critic_obs_mean=cmean.cpu().numpy(), critic_obs_var=cvar.cpu().numpy()) if PC else {}
    np.savez(args.out + "_policy.npz", obs_mean=mean.cpu().numpy(), obs_var=var.cpu().numpy(), log_std=log_std.detach().cpu().numpy(),
             **{f"pi_{k.replace('.', '_')}": v.detach().cpu().numpy() for k, v in pi.state_dict().items()},
             **{f"vf_{k.replace('.', '_')}": v.detach().cpu().numpy() for k, v in vf.state_dict().items()},
             env_id=np.array(args.env_id), env_steps=np.array(total_steps), **extra_stats,
             **({} if rand is None else dict(randomisation=np.array(json.dumps(rand.as_dict())))),
             **({} if hist is None else dict(history=np.array(json.dumps(hist.as_dict())))),
             **({} if cur is None else dict(curriculum=np.array(json.dumps(cur.as_dict())))))
    envs.close()


if __name__ == "__main__":
    main()
