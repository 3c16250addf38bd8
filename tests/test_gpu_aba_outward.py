"""The ABA outward pass that goes level by level over DPP (mocca_device.h aba_passes, OUTWARD_ROUNDS: every root->leaf chain on consecutive
lanes of a DPP row, a body's step applied to what its left neighbour holds, MAXD rounds) changes no result bit: every step of six small
batches must hash to what the library of the commit BEFORE the change produced (tests/golden/step_bits3_<case>.json, written by
tools/record_step_bits3.py from that library on an MI355X; recorded twice there, identical).  One SHA-256 per step over observations,
rewards, done flags, info, the dynamic state and the task record; no tolerance.

  walker3d      Walker3DCustomEnv-v0, 32 envs x 24 steps with auto-reset (the recording holds 21): bodies 1, 2, 3 are computed in two rows
                and stored from one -- a wrong table shows here
  walker2d, crab2d, laikago    32 x 16: the other trees that take the new pass (three, two and four chains of three bodies at most)
  cassie        CassieEnv-v0, 32 x 6: loop closures, the tree keeps the root->body walk
  adversarial   Walker3DCustomEnv-v0, 16 x 4 from the fuzz tests' adversarial states, four of them with non-finite velocities: the argument
                for exactness (a body's value is a function of its parent's alone, so what a lane held before is never seen) assumes
                nothing about finite values, and this batch holds it to that

Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("record_step_bits3", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_step_bits3.py"))
rsb3 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb3)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(rsb3.CASES))
def test_steps_hash_to_the_parents(case):
    with open(rsb3.golden_path(case)) as f:
        want = json.load(f)
    env_id, n, steps = rsb3.CASES[case]
    assert (want["env_id"], want["envs"], want["steps"], want["seed"], want["tape_seed"], want["state_seed"]) == \
        (env_id, n, steps, rsb3.SEED, rsb3.TAPE_SEED, rsb3.STATE_SEED), "the recording is of another sample: run tools/record_step_bits3.py on the parent's library"
    assert len(want["hashes"]) == steps
    if case == "walker3d":
        assert want["auto_resets"] >= 1, "the recording holds no auto-reset"
    if case == "adversarial":
        st = rsb3.adversarial_batch(env_id, n)
        assert (~np.isfinite(st).all(axis=1)).sum() == 4 and np.isnan(st).any() and np.isinf(st).any()
    got = rsb3.record(case)
    print(case, got["auto_resets"], got["lds_bytes"])
    assert got["lds_bytes"] == want["lds_bytes"]
    first = next((t for t in range(steps) if got["hashes"][t] != want["hashes"][t]), None)
    assert first is None, (case, "first step whose outputs differ from the parent's", first)
    assert got["auto_resets"] == want["auto_resets"]
