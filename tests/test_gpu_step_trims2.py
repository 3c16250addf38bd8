"""The second batch of instruction trims of the step kernel (mocca_device.h / mocca_kernels.h: childless bodies leave the constraint
rows' outward sweep, no zeroed second-path registers, walks that precede an observation form no joint axes, the epilogue reads its kernel
arguments where it uses them) changes no result bit on the paths tests/test_gpu_step_trims.py does not reach: every step of five small
batches must hash to what the library of the commit BEFORE the trims produced (tests/golden/step_bits2_<case>.json, written by
tools/record_step_bits2.py from that library on an MI355X; recorded twice there, identical).  One SHA-256 per step, no tolerance.

  walker2d, crab2d   32 envs x 24 steps: other leaf sets of the outward sweep; the sample must hold substeps WITH rows
  epilogue           Walker3DCustomEnv-v0, 64 x 40, every optional epilogue argument attached: terminal observations, episode statistics
                     (return, masks, bad masks, totals, records), info, per-env gain and eval-mode vectors, env_offset 4096.  The hash also
                     covers the terminal-observation buffer, both mask columns, the episode records and the integer totals; the sum of the
                     returns is held to the recorded returns within the rounding of its own atomic additions (see the tool: the one value
                     that depends on the order the waves finish in).  The recording must hold auto-resets: the f32 CPU oracle ends 99
                     episodes on this tape (tools/record_step_bits2.py --oracle, default gain), the parent's library 97.
  planner_ctrl       Walker3DPlannerEnv-v0, 32 x 12 plan_step behind a base controller: the kernel keeps robot_state, and the hash covers
                     the controller's outputs, which are a function of it
  task_step          Walker3DStepperEnv-v0, 32 envs, three mocca_task_step calls: the INJECT instances compile from the same header

Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import pytest

_spec = importlib.util.spec_from_file_location("record_step_bits2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_step_bits2.py"))
rsb2 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb2)

pytestmark = pytest.mark.gpu


def _golden(case):
    with open(rsb2.golden_path(case)) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(rsb2.CASES))
def test_steps_hash_to_the_parents(case):
    want = _golden(case)
    env_id, n, steps = rsb2.CASES[case]
    assert (want["env_id"], want["envs"], want["steps"], want["seed"], want["tape_seed"]) == (env_id, n, steps, rsb2.SEED, rsb2.TAPE_SEED), \
        "the recording is of another sample: run tools/record_step_bits2.py on the parent's library"
    assert len(want["hashes"]) == steps
    if case in ("walker2d", "crab2d"):
        assert want["records"] - want["classes"]["no_rows"] > 0, (case, "no substep with rows in the sample", want["classes"])
        assert want["classes"]["limits_only"] > 0 and want["classes"]["rows_ge_8"] > 0, (case, want["classes"])
    if case == "epilogue":
        assert want["auto_resets"] >= 1, "the recording holds no auto-reset"
    got = rsb2.record(case)
    print(case, got["auto_resets"], got["classes"])
    assert got["lds_bytes"] == want["lds_bytes"]
    first = next((t for t in range(steps) if got["hashes"][t] != want["hashes"][t]), None)
    assert first is None, (case, "first step whose outputs differ from the parent's", first)
    assert (got["classes"], got["auto_resets"]) == (want["classes"], want["auto_resets"]), (case, got["classes"], want["classes"])
