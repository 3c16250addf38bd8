"""Record what the step kernel computes, bit for bit: one SHA-256 per env.step over observations, rewards, done flags, info, the dynamic
state and the task record of a small batch stepped under a seeded U(-1, 1) action tape, plus which row classes the sample's last substeps
held (from the debug record).  tests/test_gpu_step_trims.py recomputes the hashes with the library under test and compares them with the
files this tool wrote from the library of the commit BEFORE a bit-exact kernel change:

    python tools/record_step_bits.py                # every case -> tests/golden/step_bits_<case>.json  (needs the GPU)
    python tools/record_step_bits.py --oracle       # the row classes the f32 CPU oracle holds on the Custom case's tape (no GPU)

MOCCA_LIB_PATH selects the library, as everywhere."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED, TAPE_SEED = 21, 3
#        case               env id                    envs steps curriculum caps (VecEnv's max_rows / max_contacts)
CASES = {"custom": ("Walker3DCustomEnv-v0", 128, 48, None, {}),
         "stepper_c9": ("Walker3DStepperEnv-v0", 128, 48, 9, {}),
         "planner": ("Walker3DPlannerEnv-v0", 128, 48, None, {}),
         "laikago": ("LaikagoCustomEnv-v0", 128, 48, None, {}),
         "cassie": ("CassieEnv-v0", 32, 6, None, {}),
         "custom_compact": ("Walker3DCustomEnv-v0", 128, 48, None, {"max_rows": 32}),
         # the 48-row instance with a contact cap the walker reaches: under the default cap of 12 no env of the Custom case ever has more
         # terrain contacts than the solver holds (f32 oracle, this tape: at most 9 in 1000 steps), so the path that keeps the deepest runs here
         "custom_cap4": ("Walker3DCustomEnv-v0", 128, 48, None, {"max_contacts": 4})}
# row classes of a last substep (debug words: 0 rows, 1 limit rows, 2 contacts kept, 3..4 terrain slots within the margin, 7 self pairs)
CLASSES = ("no_rows", "limits_only", "self_contact", "rows_ge_8", "terrain_over_cap")


def golden_path(case, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), f"step_bits_{case}.json")


def classes(rec, max_contacts):
    """rec [k][>= 8] int32 debug records -> {class: number of records that hold it}"""
    rec = np.asarray(rec).astype(np.int64)
    nr, nl, selfp = rec[:, 0], rec[:, 1], rec[:, 7]
    slots = (rec[:, 3] & 0xFFFFFFFF) | ((rec[:, 4] & 0xFFFFFFFF) << 32)
    n_terrain = np.array([bin(int(s)).count("1") for s in slots])
    held = {"no_rows": nr == 0, "limits_only": (nr > 0) & (nr == nl), "self_contact": selfp > 0, "rows_ge_8": nr >= 8,
            "terrain_over_cap": n_terrain > max_contacts}
    return {k: int(v.sum()) for k, v in held.items()}


def record(case):
    """Step the case on the GPU -> {"hashes": [one hex digest per step], "classes": {...}, ...}"""
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    env_id, n, steps, curriculum, caps = CASES[case]
    env = VecEnv(env_id, n, auto_reset=True, seed=SEED, **caps)
    if curriculum is not None:
        env.set_param(L.PARAM_CURRICULUM, curriculum)
    dbg = env.set_debug(True)
    env.reset()
    nd = 13 + 2 * int(env.model.n_joints)   # the dynamic state proper (the slots' impulses behind it are not stored by these blobs)
    rng = np.random.default_rng(TAPE_SEED)
    hashes, recs = [], []
    for _ in range(steps):
        act = torch.from_numpy(rng.uniform(-1, 1, (n, env.act_dim)).astype(np.float32)).cuda()
        obs, rew, done, info = env.step(act)
        h = hashlib.sha256()
        for x in (obs, rew, done, info, env.get_state()[:, :nd], env.get_task()):
            h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
        hashes.append(h.hexdigest())
        recs.append(dbg.cpu().numpy().copy())
    out = {"env_id": env_id, "envs": n, "steps": steps, "curriculum": curriculum, "caps": caps, "seed": SEED, "tape_seed": TAPE_SEED,
           "lds_bytes": int(env.kernel_info()["lds_bytes"]), "classes": classes(np.concatenate(recs), int(env.model.max_contacts)), "hashes": hashes}
    env.close()
    return out


def oracle_classes(case="custom"):
    """The same tape through the f32 CPU oracle: the row classes its last substeps hold (what the sample is chosen by, before any GPU time)."""
    from mocca_envs_amd.vec_env import TASKS, _DEFAULT_PARAMS, compile_model_for
    from oracle import oracle as orc
    orc.build()
    env_id, n, steps, curriculum, caps = CASES[case]
    model = compile_model_for(env_id)
    if "max_rows" in caps:      # as VecEnv sets them
        model.max_rows = caps["max_rows"]
    model.max_contacts = caps.get("max_contacts", min(int(model.max_contacts), int(model.max_rows) // 3))
    o = orc.Oracle(model.to_bytes(), TASKS[env_id], n, "f32")
    o.set_param(orc.PARAM_AUTO_RESET, 1)
    for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
        o.set_param(pid, val)
    if curriculum is not None:
        o.set_param(orc.PARAM_CURRICULUM, curriculum)
    o.reset(seed=SEED)
    rng = np.random.default_rng(TAPE_SEED)
    recs = []
    for _ in range(steps):
        o.step(rng.uniform(-1, 1, (n, o.act_dim)).astype(np.float32))
        recs.append(o.get_debug())
    return classes(np.concatenate(recs), int(model.max_contacts))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out-dir", default=None, help="where the JSON files go (default: tests/golden)")
    ap.add_argument("--oracle", action="store_true", help="row classes of the CPU oracle on the cases' tapes; writes nothing")
    args = ap.parse_args()
    for case in args.cases:
        if args.oracle:
            print(case, oracle_classes(case))
            continue
        out = record(case)
        os.makedirs(args.out_dir or os.path.dirname(golden_path(case)), exist_ok=True)
        with open(golden_path(case, args.out_dir), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(case, out["lds_bytes"], out["classes"], out["hashes"][-1][:16])
