"""Record what the step kernel computes where the order of its LDS reads could decide it, bit for bit: one SHA-256 per env.step over the
dynamic state, the task record, observations, rewards, done flags, info and the debug words, as tools/record_step_bits4.py does (whose
adversarial batch this tool uses), over the smallest batches that reach every path of the constraint rows' sweeps and of the ABA inward
levels (mocca_device.h solve_constraints / aba_passes, MOCCA_NO_TRIM_10 .. 12).  tests/test_gpu_sweep_prefetch.py recomputes the hashes
with the library under test and compares them with the files this tool wrote from the library of the commit BEFORE the change:

    python tools/record_step_bits5.py               # every case, recorded twice -> tests/golden/step_bits5_<case>.json  (needs the GPU)
    python tools/record_step_bits5.py --oracle      # the coverage figures of the f32 CPU oracle on the same tapes (no GPU)

MOCCA_LIB_PATH selects the library, as everywhere.

  custom          Walker3DCustomEnv-v0, 32 envs x 24 steps, seed 0, auto-reset: the headline instance; waves with and without a second path
  stepper         Walker3DStepperEnv-v0, 32 x 16: the other 128-VGPR instance
  planner         Walker3DPlannerEnv-v0, 32 x 12: whichever order the resource rule leaves it, it must equal the parent
  custom_compact  Walker3DCustomEnv-v0 with max_rows = 32, 32 x 16: the compact layout (mocca_r32.hip)
  custom_r64      Walker3DCustomEnv-v0 with max_rows = 64, 32 x 16: the 64-row instance (mocca_r64.hip)
  walker2d, crab2d, laikago   32 x 16: other NB / MAXD / leaf sets -- the bounds of the fetch ahead at the last body and the last position
  cassie          CassieEnv-v0, 32 x 6: loop closures, both paths in every substep
  adversarial     Walker3DCustomEnv-v0, 16 x 4 from the fuzz tests' adversarial states, four with non-finite velocities: nothing may
                  depend on a value being finite

Coverage (COVERAGE, checked before a file is written and stored in it): env-steps whose last substep held a self contact
(MOCCA_DBG_SELF > 0) and env-steps whose last substep held no row."""
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

SEED, TAPE_SEED, STATE_SEED = 0, 0, rsb3.STATE_SEED
#        case              env id                    envs steps caps (VecEnv's max_rows)
CASES = {"custom": ("Walker3DCustomEnv-v0", 32, 24, {}),
         "stepper": ("Walker3DStepperEnv-v0", 32, 16, {}),
         "planner": ("Walker3DPlannerEnv-v0", 32, 12, {}),
         "custom_compact": ("Walker3DCustomEnv-v0", 32, 16, {"max_rows": 32}),
         "custom_r64": ("Walker3DCustomEnv-v0", 32, 16, {"max_rows": 64}),
         "walker2d": ("Walker2DCustomEnv-v0", 32, 16, {}),
         "crab2d": ("Crab2DCustomEnv-v0", 32, 16, {}),
         "laikago": ("LaikagoCustomEnv-v0", 32, 16, {}),
         "cassie": ("CassieEnv-v0", 32, 6, {}),
         "adversarial": ("Walker3DCustomEnv-v0", 16, 4, {})}
# case -> least number of env-steps with a self contact, and whether env-steps without a row must occur (5 % of the env-steps; the f32 CPU
# oracle on these tapes: custom 88 of 768 and 45 without a row, stepper 49 of 512 and 31)
COVERAGE = {"custom": (38, True), "stepper": (25, True)}
DBG_ROWS, DBG_SELF = 0, 7   # MOCCA_DBG_ROWS, MOCCA_DBG_SELF (include/mocca.h)

adversarial_batch = rsb3.adversarial_batch


def golden_path(case, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), f"step_bits5_{case}.json")


def coverage(recs):
    """recs [k][>= 8] int32 debug records, one per env-step -> {"self_contact": ..., "no_rows": ...}"""
    recs = np.asarray(recs)
    return {"self_contact": int((recs[:, DBG_SELF] > 0).sum()), "no_rows": int((recs[:, DBG_ROWS] == 0).sum())}


def covered(case, cov):
    need_self, need_zero = COVERAGE.get(case, (0, False))
    return cov["self_contact"] >= need_self and (cov["no_rows"] > 0 or not need_zero)


def record(case):
    """Step the case on the GPU -> {"hashes": [one hex digest per step], "coverage": {...}, ...}"""
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    env_id, n, steps, caps = CASES[case]
    env = VecEnv(env_id, n, auto_reset=True, seed=SEED, **caps)
    dbg = env.set_debug(True)
    env.reset()
    if case == "adversarial":
        env.set_state(adversarial_batch(env_id, n))
    nd = 13 + 2 * int(env.model.n_joints)
    rng = np.random.default_rng(TAPE_SEED)
    hashes, recs, resets = [], [], 0
    for _ in range(steps):
        act = torch.from_numpy(rng.uniform(-1, 1, (n, env.act_dim)).astype(np.float32)).cuda()
        obs, rew, done, info = env.step(act)
        state = env.get_state()[:, :nd]
        d = dbg.cpu().numpy().copy()
        h = hashlib.sha256()
        for x in (state, env.get_task(), obs, rew, done, info):
            h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
        h.update(np.ascontiguousarray(d).tobytes())
        hashes.append(h.hexdigest())
        recs.append(d)
        resets += int((done.cpu().numpy() != 0).sum())
    out = {"env_id": env_id, "envs": n, "steps": steps, "caps": caps, "seed": SEED, "tape_seed": TAPE_SEED, "state_seed": STATE_SEED,
           "lds_bytes": int(env.kernel_info()["lds_bytes"]), "auto_resets": resets, "coverage": coverage(np.concatenate(recs)),
           "hashes": hashes}
    env.close()
    return out


def oracle_coverage(case):
    """The same tape through the f32 CPU oracle: the coverage figures the batches were chosen by, before any GPU time."""
    from mocca_envs_amd.vec_env import TASKS, _DEFAULT_PARAMS, compile_model_for
    from oracle import oracle as orc
    orc.build()
    env_id, n, steps, caps = CASES[case]
    model = compile_model_for(env_id)
    if "max_rows" in caps:      # as VecEnv sets them
        model.max_rows = caps["max_rows"]
        model.max_contacts = min(20, caps["max_rows"] // 3) if caps["max_rows"] > 48 else min(int(model.max_contacts), caps["max_rows"] // 3)
    o = orc.Oracle(model.to_bytes(), TASKS[env_id], n, "f32")
    o.set_param(orc.PARAM_AUTO_RESET, 1)
    for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
        o.set_param(pid, val)
    o.reset(seed=SEED)
    rng = np.random.default_rng(TAPE_SEED)
    recs = []
    for _ in range(steps):
        o.step(rng.uniform(-1, 1, (n, o.act_dim)).astype(np.float32))
        recs.append(o.get_debug())
    return coverage(np.concatenate(recs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out-dir", default=None, help="where the JSON files go (default: tests/golden)")
    ap.add_argument("--oracle", action="store_true", help="coverage figures of the CPU oracle on the cases' tapes; writes nothing")
    args = ap.parse_args()
    for case in args.cases:
        if args.oracle:
            print(case, oracle_coverage(case))
            continue
        out, again = record(case), record(case)
        if out != again:
            sys.exit(f"{case}: two recordings differ -- nothing written")
        if not covered(case, out["coverage"]):
            sys.exit(f"{case}: coverage {out['coverage']} misses {COVERAGE[case]} -- nothing written")
        os.makedirs(args.out_dir or os.path.dirname(golden_path(case)), exist_ok=True)
        with open(golden_path(case, args.out_dir), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(case, out["lds_bytes"], out["auto_resets"], out["coverage"], out["hashes"][-1][:16])
