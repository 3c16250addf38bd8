"""Record what the step kernel computes where the body velocities of the kinematics walk decide it, bit for bit: one SHA-256 per
env.step, as tools/record_step_bits3.py does (whose machinery this tool uses), over small batches chosen for the walk's second phase going
level by level over DPP (mocca_device.h walk_phase2, WALK_LEVELS).  tests/test_gpu_walk_levels.py recomputes the hashes with the library
under test and compares them with the files this tool wrote from the library of the commit BEFORE the change:

    python tools/record_step_bits4.py               # every case -> tests/golden/step_bits4_<case>.json  (needs the GPU)

MOCCA_LIB_PATH selects the library, as everywhere.

  walker3d        Walker3DCustomEnv-v0, 32 envs x 24 steps with auto-reset: bodies 1, 2, 3 sit in two DPP rows (both legs hang on the trunk)
  stepper         Walker3DStepperEnv-v0, 32 x 16: the same tree in the other task instance
  walker2d, crab2d, laikago   32 x 16: the other trees that take the level-by-level phase (three, two and four leaf chains)
  cassie          CassieEnv-v0, 32 x 6: loop closures, the tree keeps lane = body and the sum along the path
  fast_joints     Walker3DCustomEnv-v0, 16 x 4 from set_state: every joint speed drawn from +-50 rad/s on a base that spins at up to
                  10 rad/s -- the velocity chain dominates the velocity-product accelerations and the bias forces
  adversarial     Walker3DCustomEnv-v0, 16 x 4 from the states of the fuzz tests (record_step_bits3.adversarial_batch), four of them with
                  non-finite joint or base velocities: what a lane holds before its parent's value is final must not reach the result"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_step_bits3", os.path.join(ROOT, "tools", "record_step_bits3.py"))
rsb3 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb3)   # (puts the repository and tests/ on sys.path)

SEED, TAPE_SEED, STATE_SEED = rsb3.SEED, rsb3.TAPE_SEED, rsb3.STATE_SEED
#        case           env id                   envs steps
CASES = {"walker3d": ("Walker3DCustomEnv-v0", 32, 24),
         "stepper": ("Walker3DStepperEnv-v0", 32, 16),
         "walker2d": ("Walker2DCustomEnv-v0", 32, 16),
         "crab2d": ("Crab2DCustomEnv-v0", 32, 16),
         "laikago": ("LaikagoCustomEnv-v0", 32, 16),
         "cassie": ("CassieEnv-v0", 32, 6),
         "fast_joints": ("Walker3DCustomEnv-v0", 16, 4),
         "adversarial": ("Walker3DCustomEnv-v0", 16, 4)}
FAST_QD, FAST_SPIN = 50.0, 10.0   # rad/s


def golden_path(case, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), f"step_bits4_{case}.json")


adversarial_batch = rsb3.adversarial_batch


def fast_batch(st, nj):
    """the states after a reset (fp32 [n][state_dim]) with every joint speed drawn from +-FAST_QD and the base's angular velocity from +-FAST_SPIN"""
    rng = np.random.default_rng(STATE_SEED)
    st = np.array(st, np.float32)
    st[:, 13 + nj:13 + 2 * nj] = rng.uniform(-FAST_QD, FAST_QD, (st.shape[0], nj)).astype(np.float32)
    st[:, 10:13] = rng.uniform(-FAST_SPIN, FAST_SPIN, (st.shape[0], 3)).astype(np.float32)
    return st


def record(case):
    """Step the case on the GPU -> {"hashes": [one hex digest per step], ...}"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    env_id, n, steps = CASES[case]
    env = VecEnv(env_id, n, auto_reset=True, seed=SEED)
    env.reset()
    nj = int(env.model.n_joints)
    if case == "adversarial":
        env.set_state(adversarial_batch(env_id, n))
    if case == "fast_joints":
        env.set_state(fast_batch(env.get_state().cpu().numpy(), nj))
    nd = 13 + 2 * nj
    rng = np.random.default_rng(TAPE_SEED)
    hashes, resets = [], 0
    for _ in range(steps):
        act = torch.from_numpy(rng.uniform(-1, 1, (n, env.act_dim)).astype(np.float32)).cuda()
        obs, rew, done, info = env.step(act)
        state = env.get_state()[:, :nd]
        h = hashlib.sha256()
        for x in (obs, rew, done, info, state, env.get_task()):
            h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
        hashes.append(h.hexdigest())
        resets += int((done.cpu().numpy() != 0).sum())
    out = {"env_id": env_id, "envs": n, "steps": steps, "seed": SEED, "tape_seed": TAPE_SEED, "state_seed": STATE_SEED,
           "lds_bytes": int(env.kernel_info()["lds_bytes"]), "auto_resets": resets, "hashes": hashes}
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out-dir", default=None, help="where the JSON files go (default: tests/golden)")
    args = ap.parse_args()
    for case in args.cases:
        out = record(case)
        os.makedirs(args.out_dir or os.path.dirname(golden_path(case)), exist_ok=True)
        with open(golden_path(case, args.out_dir), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(case, out["lds_bytes"], out["auto_resets"], out["hashes"][-1][:16])
