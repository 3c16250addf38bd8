"""The kinematics walk's second phase forming the body velocities level by level over DPP (mocca_device.h walk_phase2, WALK_LEVELS: the
outward pass's lane layout, v_b = v_parent(b) + S_b qd_b from what the left neighbour holds, MAXD - 1 shifts) changes no result bit: every
step of eight small batches must hash to what the library of the commit BEFORE the change produced (tests/golden/step_bits4_<case>.json,
written by tools/record_step_bits4.py from that library on an MI355X; recorded twice there, identical).  One SHA-256 per step over
observations, rewards, done flags, info, the dynamic state and the task record; no tolerance.

  walker3d      Walker3DCustomEnv-v0, 32 envs x 24 steps with auto-reset (at least one reset in the recording): bodies 1, 2, 3 are computed
                in two rows and stored from one -- a wrong table or a lane reading a masked neighbour shows here
  stepper       Walker3DStepperEnv-v0, 32 x 16: the same tree, the other task instance
  walker2d, crab2d, laikago    32 x 16: the other trees that take the new phase
  cassie        CassieEnv-v0, 32 x 6: loop closures, the tree keeps lane = body and the sum along the path
  fast_joints   Walker3DCustomEnv-v0, 16 x 4 from set_state: joint speeds of +-50 rad/s on a base spinning at up to 10 rad/s -- the velocity
                chain dominates the velocity-product accelerations and the bias forces
  adversarial   Walker3DCustomEnv-v0, 16 x 4 from the fuzz tests' adversarial states, four of them with non-finite joint or base velocities:
                the argument for exactness (a body's value is a function of its parent's alone, so what a lane held before is never seen)
                assumes nothing about finite values, and this batch holds it to that

Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("record_step_bits4", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_step_bits4.py"))
rsb4 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb4)

pytestmark = pytest.mark.gpu


def test_the_cases_are_the_issues():
    assert rsb4.CASES == {"walker3d": ("Walker3DCustomEnv-v0", 32, 24), "stepper": ("Walker3DStepperEnv-v0", 32, 16),
                          "walker2d": ("Walker2DCustomEnv-v0", 32, 16), "crab2d": ("Crab2DCustomEnv-v0", 32, 16),
                          "laikago": ("LaikagoCustomEnv-v0", 32, 16), "cassie": ("CassieEnv-v0", 32, 6),
                          "fast_joints": ("Walker3DCustomEnv-v0", 16, 4), "adversarial": ("Walker3DCustomEnv-v0", 16, 4)}
    assert rsb4.FAST_QD == 50.0


@pytest.mark.parametrize("case", list(rsb4.CASES))
def test_steps_hash_to_the_parents(case):
    with open(rsb4.golden_path(case)) as f:
        want = json.load(f)
    env_id, n, steps = rsb4.CASES[case]
    assert (want["env_id"], want["envs"], want["steps"], want["seed"], want["tape_seed"], want["state_seed"]) == \
        (env_id, n, steps, rsb4.SEED, rsb4.TAPE_SEED, rsb4.STATE_SEED), "the recording is of another sample: run tools/record_step_bits4.py on the parent's library"
    assert len(want["hashes"]) == steps
    if case == "walker3d":
        assert want["auto_resets"] >= 1, "the recording holds no auto-reset"
    if case == "adversarial":
        st = rsb4.adversarial_batch(env_id, n)
        bad = ~np.isfinite(st).all(axis=1)
        assert bad.sum() >= 4 and np.isnan(st).any() and np.isinf(st).any()
        # ... in the velocities: the base's (7 .. 12) or the joints' (the columns behind the joint angles)
        from mocca_envs_amd.vec_env import compile_model_for
        nj = int(compile_model_for(env_id).n_joints)
        vel = np.concatenate([st[:, 7:13], st[:, 13 + nj:13 + 2 * nj]], axis=1)
        assert (~np.isfinite(vel).all(axis=1)).sum() >= 4
    got = rsb4.record(case)
    print(case, got["auto_resets"], got["lds_bytes"])
    assert got["lds_bytes"] == want["lds_bytes"]
    first = next((t for t in range(steps) if got["hashes"][t] != want["hashes"][t]), None)
    assert first is None, (case, "first step whose outputs differ from the parent's", first)
    assert got["auto_resets"] == want["auto_resets"]
