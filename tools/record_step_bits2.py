"""Record what the step kernel computes on the paths tools/record_step_bits.py leaves out, bit for bit: other trees (the leaf sets of
Walker2D and Crab2D), a Custom batch with every optional epilogue argument attached, a planner batch behind a base controller (the
kernel keeps `robot_state`), and the task-layer (INJECT) instance.  One SHA-256 per env.step, as there; tests/test_gpu_step_trims2.py
recomputes the hashes with the library under test and compares them with the files this tool wrote from the library of the commit
BEFORE a bit-exact kernel change:

    python tools/record_step_bits2.py               # every case -> tests/golden/step_bits2_<case>.json  (needs the GPU)
    python tools/record_step_bits2.py --oracle      # auto-resets and row classes of the f32 CPU oracle on the epilogue case's tape (no GPU)

MOCCA_LIB_PATH selects the library, as everywhere.

The epilogue case hashes, besides what every case hashes, the terminal-observation buffer, the two mask columns, the records of the
episodes that ended in the step (return, length, done bits: 16 bytes each, exact) and the totals of length, episodes and truncated
episodes.  The fourth total, the sum of the returns, is the one value of a step that is not a function of its inputs alone: the envs
that end in one launch add their returns with one float atomic each, in the order the waves get there, and float addition does not
commute in its last bit.  It is therefore held to the float64 sum of the recorded returns (which ARE hashed) within the rounding of its
own additions: k additions, each off by at most half an ulp of a partial sum, |error| <= k * 2^-24 * max |partial sum|."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rsb = _load("record_step_bits", "tools", "record_step_bits.py")   # its `classes` helper, seeds and hashing scheme; its CASES stay as they are
SEED, TAPE_SEED = rsb.SEED, rsb.TAPE_SEED
ENV_OFFSET = 4096
#        case          env id                   envs steps
CASES = {"walker2d": ("Walker2DCustomEnv-v0", 32, 24),
         "crab2d": ("Crab2DCustomEnv-v0", 32, 24),
         "epilogue": ("Walker3DCustomEnv-v0", 64, 40),       # terminal obs, episode statistics, info, per-env gain and eval mode, env_offset
         "planner_ctrl": ("Walker3DPlannerEnv-v0", 32, 12),  # plan_step behind a base controller: the step kernel keeps robot_state
         "task_step": ("Walker3DStepperEnv-v0", 32, 3)}      # the INJECT instance: no physics, contact flags from the caller


def golden_path(case, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), f"step_bits2_{case}.json")


def _digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).tobytes())
    return h.hexdigest()


def per_env_vectors(n):
    """(applied gain, eval mode) of the epilogue case, one value per env"""
    rng = np.random.default_rng(TAPE_SEED + 1)
    return rng.uniform(0.7, 1.3, n).astype(np.float32), (np.arange(n) % 3 == 0).astype(np.float32)


def return_sum_bound(returns):
    """returns: the recorded episode returns in any order -> (their float64 sum, the bound on the float32 total's distance from it)"""
    r = np.asarray(returns, np.float64)
    if r.size == 0:
        return 0.0, 0.0
    return float(r.sum()), float(r.size * 2.0 ** -24 * np.abs(r).sum())   # sum |r_i| bounds every partial sum in every order


def record(case):
    """Step the case on the GPU -> {"hashes": [one hex digest per step], ...}"""
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    env_id, n, steps = CASES[case]
    out = {"env_id": env_id, "envs": n, "steps": steps, "seed": SEED, "tape_seed": TAPE_SEED}
    rng = np.random.default_rng(TAPE_SEED)
    kw = {}
    if case == "epilogue":
        kw = dict(env_offset=ENV_OFFSET, terminal_obs=True)
    elif case == "planner_ctrl":
        kw = dict(base_controller=_load("controller_reference", "tests", "controller_reference.py").random_controller("small", seed=7))
    env = VecEnv(env_id, n, auto_reset=True, seed=SEED, **kw)
    ep = None
    if case == "epilogue":
        ep = env.episode_stats(True, slots=4)
        gain, evalm = per_env_vectors(n)
        env.set_param_v(L.PARAM_APPLIED_GAIN, gain)
        env.set_param_v(L.PARAM_EVAL_MODE, evalm)
    dbg = env.set_debug(True)
    env.reset()
    nd = 13 + 2 * int(env.model.n_joints)
    hashes, recs, resets, returns = [], [], 0, []
    for k in range(1, steps + 1):
        if case == "task_step":
            act = torch.from_numpy(rng.uniform(-1, 1, (n, env.act_dim)).astype(np.float32)).cuda()
            touch, target = rng.integers(0, 2, (n, 2)).astype(np.int32), rng.integers(0, 3, (n, 2)).astype(np.int32)
            obs, rew, done, info = env.task_step(act, touch, target)
        elif case == "planner_ctrl":
            obs, rew, done, info = env.plan_step(torch.from_numpy(rng.normal(0, 1, (n, env.plan_dim)).astype(np.float32)).cuda())
        else:
            obs, rew, done, info = env.step(torch.from_numpy(rng.uniform(-1, 1, (n, env.act_dim)).astype(np.float32)).cuda())
        torch.cuda.synchronize()
        parts = [obs, rew, done, info, env.get_state()[:, :nd], env.get_task()]
        d = done.cpu().numpy()
        resets += int((d != 0).sum())
        if case == "task_step":
            parts.append(env.get_terrain())
        elif case == "planner_ctrl":
            parts.extend(env.base_outputs())     # the controller ran on the robot_state the step before kept
        elif case == "epilogue":
            serial = ep["first_serial"] + k - 1
            ended = ep["records"][serial % ep["slots"]].numpy()[d != 0]      # pinned host memory; the launch has completed
            assert (ended[:, 0] == serial).all(), "an episode record of another launch"
            returns.extend(ended[:, 1].copy().view(np.float32).tolist())
            totals = ep["totals"].cpu().numpy()
            want, bound = return_sum_bound(returns)
            assert abs(float(totals[0]) - want) <= bound, ("sum of the episode returns", float(totals[0]), want, bound)
            parts.extend([env.terminal_obs, ep["masks"], ep["bad_masks"], ended, totals[1:]])
        hashes.append(_digest(*parts))
        recs.append(dbg.cpu().numpy().copy())
    out.update(lds_bytes=int(env.kernel_info()["lds_bytes"]), auto_resets=resets,
               classes=rsb.classes(np.concatenate(recs), int(env.model.max_contacts)), records=int(np.concatenate(recs).shape[0]), hashes=hashes)
    env.close()
    return out


def oracle_epilogue():
    """The epilogue case's tape through the f32 CPU oracle: how many envs end (and reset), and the row classes of the last substeps."""
    from mocca_envs_amd.vec_env import TASKS, _DEFAULT_PARAMS, compile_model_for
    from oracle import oracle as orc
    orc.build()
    env_id, n, steps = CASES["epilogue"]
    model = compile_model_for(env_id)
    model.max_contacts = min(int(model.max_contacts), int(model.max_rows) // 3)
    o = orc.Oracle(model.to_bytes(), TASKS[env_id], n, "f32")
    o.set_param(orc.PARAM_AUTO_RESET, 1)
    for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
        o.set_param(pid, val)
    o.reset(seed=SEED)
    rng = np.random.default_rng(TAPE_SEED)
    recs, resets = [], 0
    for _ in range(steps):
        _, _, d, _ = o.step(rng.uniform(-1, 1, (n, o.act_dim)).astype(np.float32))
        resets += int((np.asarray(d) != 0).sum())
        recs.append(o.get_debug())
    return {"auto_resets": resets, "classes": rsb.classes(np.concatenate(recs), int(model.max_contacts))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out-dir", default=None, help="where the JSON files go (default: tests/golden)")
    ap.add_argument("--oracle", action="store_true", help="the CPU oracle on the epilogue case's tape (default gain, no eval mode); writes nothing")
    args = ap.parse_args()
    if args.oracle:
        print("epilogue", oracle_epilogue())
        sys.exit(0)
    for case in args.cases:
        out = record(case)
        os.makedirs(args.out_dir or os.path.dirname(golden_path(case)), exist_ok=True)
        with open(golden_path(case, args.out_dir), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(case, out["lds_bytes"], out["auto_resets"], out["classes"], out["hashes"][-1][:16])
