"""The step kernel's instruction trims (mocca_device.h: midpoint records of the self-collision broad phase, limit rows that carry their gap,
the base's 6x6 Cholesky factor formed once across lanes) change no result bit: every env.step of seven small batches must hash to what the library of the commit BEFORE the trims produced
(tests/golden/step_bits_<case>.json, written by tools/record_step_bits.py from that library on an MI355X).  One SHA-256 per step over
observations, rewards, done flags, info, the dynamic state and the task record; no tolerance.  The 48-row instance runs the Custom,
Stepper (curriculum 9), Planner and Laikago batches (128 envs x 48 steps) and Cassie (32 x 6), the compact instance the Custom batch again
(max_rows = 32).

The Custom sample must hold every row class the trims touch, asserted from the flags the recording stored (last substeps of the steps,
debug record): no rows at all, limit rows only, a self contact, eight rows or more, more terrain contacts than max_contacts.  The f32 CPU
oracle (tools/record_step_bits.py --oracle, same blob, seed and tape; no GPU) holds on the 128 x 48 Custom batch
    no rows 296   limit rows only 2731   self contact 879   >= 8 rows 1704   terrain contacts over the cap 0
and the parent's library 299 / 2726 / 874 / 1700 / 0.  The last class cannot come from that batch at all: under U(-1, 1) torques the walker
never rests on more than 9 of its 34 terrain slots (oracle: 128 envs x 1000 steps, with and without auto-reset, maximum 9 resp. 8) against
a cap of 12, whatever the seed or the step count.  The class is therefore held by a second Custom batch on the same 48-row instance whose
blob caps the contacts at 4 (`custom_cap4`: oracle 11 last substeps over the cap, parent's library 12), and asserted there; the first four
are asserted on the default batch.  Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import pytest

_spec = importlib.util.spec_from_file_location("record_step_bits", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_step_bits.py"))
rsb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsb)

pytestmark = pytest.mark.gpu

# classes a case's stored flags must show
MUST_HOLD = {"custom": ("no_rows", "limits_only", "self_contact", "rows_ge_8"),
             "custom_cap4": ("no_rows", "limits_only", "self_contact", "rows_ge_8", "terrain_over_cap"),
             "custom_compact": ("no_rows", "limits_only", "self_contact", "rows_ge_8"),
             "stepper_c9": ("self_contact", "rows_ge_8"), "planner": ("self_contact", "rows_ge_8"), "laikago": ("limits_only",), "cassie": ("rows_ge_8",)}


def _golden(case):
    with open(rsb.golden_path(case)) as f:
        return json.load(f)


def test_the_custom_sample_holds_every_row_class():
    held = {k: 0 for k in rsb.CLASSES}
    for case in ("custom", "custom_cap4"):          # Walker3DCustomEnv-v0 on the 48-row instance, default caps and max_contacts = 4
        g = _golden(case)
        assert g["env_id"] == "Walker3DCustomEnv-v0" and g["lds_bytes"] > 8192, (case, g["env_id"], g["lds_bytes"])
        for k in rsb.CLASSES:
            held[k] += g["classes"][k]
    for k in rsb.CLASSES:
        assert held[k] > 0, (k, held)


@pytest.mark.parametrize("case", list(rsb.CASES))
def test_steps_hash_to_the_parents(case):
    want = _golden(case)
    env_id, n, steps, curriculum, caps = rsb.CASES[case]
    assert (want["env_id"], want["envs"], want["steps"], want["curriculum"], want["caps"], want["seed"], want["tape_seed"]) == \
        (env_id, n, steps, curriculum, caps, rsb.SEED, rsb.TAPE_SEED), "the recording is of another sample: run tools/record_step_bits.py on the parent's library"
    assert len(want["hashes"]) == steps
    for k in MUST_HOLD[case]:
        assert want["classes"][k] > 0, (case, k, want["classes"])
    assert (want["lds_bytes"] <= 8192) == ("max_rows" in caps), (case, want["lds_bytes"])   # the compact instance where it is meant
    got = rsb.record(case)
    print(case, got["classes"])
    assert got["lds_bytes"] == want["lds_bytes"]
    first = next((t for t in range(steps) if got["hashes"][t] != want["hashes"][t]), None)
    assert first is None, (case, "first step whose outputs differ from the parent's", first)
    assert got["classes"] == want["classes"], (case, got["classes"], want["classes"])
