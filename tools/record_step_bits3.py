"""Record what the step kernel computes where the ABA outward pass decides it, bit for bit: one SHA-256 per env.step, as
tools/record_step_bits.py and tools/record_step_bits2.py do, over small batches chosen for the level-by-level outward pass
(mocca_device.h, aba_passes, OUTWARD_DPP).  tests/test_gpu_aba_outward.py recomputes the hashes with the library under test and compares
them with the files this tool wrote from the library of the commit BEFORE the change:

    python tools/record_step_bits3.py               # every case -> tests/golden/step_bits3_<case>.json  (needs the GPU)

MOCCA_LIB_PATH selects the library, as everywhere.

  walker3d        Walker3DCustomEnv-v0, 32 envs x 24 steps with auto-reset: bodies 1, 2, 3 sit in two DPP rows (both legs hang on the trunk)
  walker2d, crab2d, laikago   32 x 16: the other trees that take the level-by-level pass (three, two and four leaf chains)
  cassie          CassieEnv-v0, 32 x 6: loop closures, the tree keeps the root->body walk
  adversarial     Walker3DCustomEnv-v0, 16 x 4 from the states of the fuzz tests (tests/fuzz_blobs.py adversarial_states: upside-down bases,
                  joints past their stops, speeds beyond the clamp, deep penetration, bases 500 m out), four of them with non-finite
                  velocities (an infinite joint speed, a NaN angular velocity, ...): what a lane holds before its parent's value is final
                  must not reach the result whatever it is"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):   # tests/: fuzz_blobs and the dense reference it places the robots with
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, TAPE_SEED, STATE_SEED = 21, 3, 8
#        case           env id                  envs steps
CASES = {"walker3d": ("Walker3DCustomEnv-v0", 32, 24),
         "walker2d": ("Walker2DCustomEnv-v0", 32, 16),
         "crab2d": ("Crab2DCustomEnv-v0", 32, 16),
         "laikago": ("LaikagoCustomEnv-v0", 32, 16),
         "cassie": ("CassieEnv-v0", 32, 6),
         "adversarial": ("Walker3DCustomEnv-v0", 16, 4)}


def golden_path(case, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), f"step_bits3_{case}.json")


def adversarial_batch(env_id, n):
    """n adversarial states of the shipped robot (fp32), four of them with non-finite velocities"""
    import fuzz_blobs as F
    from mocca_envs_amd.vec_env import compile_model_for
    m = compile_model_for(env_id)
    st, _ = F.adversarial_states(m, np.random.default_rng(STATE_SEED), n)
    st[:, 3:7] /= np.linalg.norm(st[:, 3:7], axis=1)[:, None]
    st = st.astype(np.float32)
    nj = int(m.n_joints)
    st[3, 13 + nj + 5] = np.inf          # a joint speed of the first leg (body 6)
    st[7, 10:13] = np.nan                # the base's angular velocity
    st[11, 13 + nj + 0] = -np.inf        # the joint speed of body 1: the trunk both DPP rows compute
    st[13, 7] = np.inf                   # the base's linear velocity
    return st


def record(case):
    """Step the case on the GPU -> {"hashes": [one hex digest per step], ...}"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    env_id, n, steps = CASES[case]
    env = VecEnv(env_id, n, auto_reset=True, seed=SEED)
    env.reset()
    if case == "adversarial":
        env.set_state(adversarial_batch(env_id, n))
    nd = 13 + 2 * int(env.model.n_joints)
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
