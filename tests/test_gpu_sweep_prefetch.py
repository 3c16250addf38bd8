"""Reading the LDS operands of the constraint rows' sweeps and of the ABA inward levels a step ahead (mocca_device.h AHEAD_OUTWARD,
AHEAD_INWARD, AHEAD_LEVELS: the same operations in the same order, only the place of the reads changes) alters no result bit: every step of
ten small batches must hash to what the library of the commit BEFORE the change produced (tests/golden/step_bits5_<case>.json, written by
tools/record_step_bits5.py from that library on an MI355X; recorded twice there, identical).  One SHA-256 per step over the dynamic state,
the task record, observations, rewards, done flags, info and the debug words; no tolerance.

  custom          Walker3DCustomEnv-v0, 32 envs x 24 steps, seed 0, auto-reset: the headline instance; waves with one path and with two
  stepper         Walker3DStepperEnv-v0, 32 x 16: the other 128-VGPR instance
  planner         Walker3DPlannerEnv-v0, 32 x 12: whichever order the resource rule leaves it, it must equal the parent
  custom_compact  max_rows = 32, 32 x 16: the compact layout's instance
  custom_r64      max_rows = 64, 32 x 16: the 64-row instance
  walker2d, crab2d, laikago    32 x 16: other NB / MAXD / leaf sets -- the fetch ahead at the last body and the last path position
  cassie          CassieEnv-v0, 32 x 6: loop closures, both paths in every substep
  adversarial     Walker3DCustomEnv-v0, 16 x 4 from the fuzz tests' adversarial states, four with non-finite velocities

Coverage, asserted by the recorder and again here on the stored figures: a self contact in the last substep of at least 38 of the Custom
batch's 768 env-steps and 25 of the Stepper batch's 512 (5 %; the f32 CPU oracle gives 88 and 49), and env-steps without a row in both
(the oracle: 45 and 31).

Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("record_step_bits5", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_step_bits5.py"))
rsb5 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb5)

pytestmark = pytest.mark.gpu


def test_the_cases_are_the_issues():
    assert rsb5.CASES == {"custom": ("Walker3DCustomEnv-v0", 32, 24, {}), "stepper": ("Walker3DStepperEnv-v0", 32, 16, {}),
                          "planner": ("Walker3DPlannerEnv-v0", 32, 12, {}), "custom_compact": ("Walker3DCustomEnv-v0", 32, 16, {"max_rows": 32}),
                          "custom_r64": ("Walker3DCustomEnv-v0", 32, 16, {"max_rows": 64}), "walker2d": ("Walker2DCustomEnv-v0", 32, 16, {}),
                          "crab2d": ("Crab2DCustomEnv-v0", 32, 16, {}), "laikago": ("LaikagoCustomEnv-v0", 32, 16, {}),
                          "cassie": ("CassieEnv-v0", 32, 6, {}), "adversarial": ("Walker3DCustomEnv-v0", 16, 4, {})}
    assert rsb5.SEED == 0 and rsb5.COVERAGE == {"custom": (38, True), "stepper": (25, True)}


@pytest.mark.parametrize("case", list(rsb5.CASES))
def test_steps_hash_to_the_parents(case):
    with open(rsb5.golden_path(case)) as f:
        want = json.load(f)
    env_id, n, steps, caps = rsb5.CASES[case]
    assert (want["env_id"], want["envs"], want["steps"], want["caps"], want["seed"], want["tape_seed"], want["state_seed"]) == \
        (env_id, n, steps, caps, rsb5.SEED, rsb5.TAPE_SEED, rsb5.STATE_SEED), "the recording is of another sample: run tools/record_step_bits5.py on the parent's library"
    assert len(want["hashes"]) == steps
    assert rsb5.covered(case, want["coverage"]), ("the recording misses its coverage condition", want["coverage"])
    if case == "custom":
        assert want["auto_resets"] >= 1, "the recording holds no auto-reset"
    if case == "adversarial":
        st = rsb5.adversarial_batch(env_id, n)
        assert (~np.isfinite(st).all(axis=1)).sum() >= 4 and np.isnan(st).any() and np.isinf(st).any()
    got = rsb5.record(case)
    print(case, got["auto_resets"], got["lds_bytes"], got["coverage"])
    assert got["lds_bytes"] == want["lds_bytes"]   # the instance the case is meant for: 48-row, compact or 64-row
    first = next((t for t in range(steps) if got["hashes"][t] != want["hashes"][t]), None)
    assert first is None, (case, "first step whose outputs differ from the parent's", first)
    assert got["auto_resets"] == want["auto_resets"] and got["coverage"] == want["coverage"]
