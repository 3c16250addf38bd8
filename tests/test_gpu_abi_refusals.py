"""The C ABI's refusals: every recorded one keeps its code and its message (tests/golden/abi_refusals.json, recorded by
tools/record_abi_refusals.py against the library before the host layer was cut into units), the refusals that used to leave a stale message
now name their entry and their argument, and a refused call leaves the handle as it was."""
import ctypes as C
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = "B"
# the refusals that set no message before: (entry, arguments as the recorder writes them)
SILENT = [
    ("mocca_reset", [None, 0, None, None]), ("mocca_step", [None] * 6), ("mocca_plan_step", [None] * 6), ("mocca_task_step", [None] * 9),
    ("mocca_observe", [None, None]), ("mocca_get_state", [None, None]), ("mocca_set_state", [None, None]), ("mocca_get_task", [None, None]),
    ("mocca_set_task", [None, None]), ("mocca_get_terrain", [None, None]), ("mocca_set_terrain", [None, None]),
    ("mocca_set_param_v", [2, None, 0, None]), ("mocca_get_link_frames", [None, None]), ("mocca_set_draw_tape", [B, 0]),
]


def _recorder():
    spec = importlib.util.spec_from_file_location("record_abi_refusals", os.path.join(ROOT, "tools", "record_abi_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    return _recorder()


def test_recorded_refusals_keep_code_and_message(rec):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_refusals.json")))
    assert golden["n_envs"] == rec.N and sum(c["rc"] < 0 for c in golden["cases"]) > 200
    for why in golden["unreached"]:
        assert any(k in why for k in ("HIP error", "host allocation", "2^31", "at 2 envs")), why
    hs = rec.Handles()
    try:
        wrong = []
        for c in golden["cases"]:
            rc, msg = hs.call(c["handle"], c["entry"], c["args"])
            if c["message"] is None:   # refused without a message when the file was recorded: today it names its entry
                if rc != c["rc"] or not (msg or "").startswith(c["entry"] + ": "):
                    wrong.append((c["handle"], c["entry"], c["args"], (c["rc"], c["entry"] + ": ..."), (rc, msg)))
            elif (rc, msg) != (c["rc"], c["message"]):
                wrong.append((c["handle"], c["entry"], c["args"], (c["rc"], c["message"]), (rc, msg)))
        assert not wrong, wrong[:5]
    finally:
        hs.close()


def _rollout(hs, name, torch, with_attachments):
    """reset and 3 steps on fixed actions (and, with the attachments, the deterministic policy's output and the history block of each step)
    -> every output and the final state, task and terrain records, as one list of tensors"""
    lib, h = hs.lib, hs.h[name]
    od, ad = hs.dims(name)
    f32 = dict(dtype=torch.float32, device="cuda")
    obs, rew, done = torch.zeros(rec_n(hs), od, **f32), torch.zeros(rec_n(hs), **f32), torch.zeros(rec_n(hs), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    out = []
    assert lib.mocca_reset(h, None, 7, p(obs), None) == 0
    out.append(obs.clone())
    for k in range(3):
        act = torch.full((rec_n(hs), ad), 0.1 * (k - 1), **f32)
        if with_attachments:
            a, v, blk = torch.zeros(rec_n(hs), ad, **f32), torch.zeros(rec_n(hs), **f32), torch.zeros(rec_n(hs), lib.mocca_history_dim(h), **f32)
            assert lib.mocca_act(h, p(obs), od, None, 1, p(a), None, p(v), None, None) == 0
            assert lib.mocca_history(h, p(obs), od, p(act), ad, p(blk), blk.shape[1], None) == 0
            out += [a, v, blk]
        assert lib.mocca_step(h, p(act), p(obs), p(rew), p(done), None, None) == 0
        out += [obs.clone(), rew.clone(), done.clone()]
    state = torch.zeros(rec_n(hs), lib.mocca_state_dim(h), **f32)
    task = torch.zeros(rec_n(hs), 40, dtype=torch.int32, device="cuda")
    terrain = torch.zeros(rec_n(hs), 128, **f32)
    assert lib.mocca_get_state(h, p(state), None) == 0 and lib.mocca_get_task(h, p(task), None) == 0 and lib.mocca_get_terrain(h, p(terrain), None) == 0
    torch.cuda.synchronize()
    return out + [state, task, terrain]


def rec_n(hs):
    return hs.lib.mocca_n_envs(hs.h["walker"])


def _same_bits(a, b, torch):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_silent_refusals_now_speak_and_leave_the_handle_alone(rec):
    import torch
    hs, twin = rec.Handles(), rec.Handles()
    try:
        assert hs.call("walker", "mocca_set_param", [99, 0.0]) == (-1, rec.SENTINEL)   # (call() provokes it again ahead of every case)
        for entry, args in SILENT:
            rc, msg = hs.call("walker", entry, args)
            assert rc == -1 and msg is not None and msg.startswith(entry + ": "), (entry, rc, msg)   # None: the earlier message stood
        assert hs.call("walker", "mocca_step", [None] * 6)[1] == "mocca_step: act_dev, obs_dev, rew_dev and done_dev must not be NULL"
        assert hs.call("walker", "mocca_set_draw_tape", [B, 0])[1] == "mocca_set_draw_tape: n_per_env must be positive with a tape"
        _same_bits(_rollout(hs, "walker", torch, False), _rollout(twin, "walker", torch, False), torch)
    finally:
        hs.close()
        twin.close()


def test_a_refused_setter_leaves_the_attachment_in_place(rec):
    import torch
    hs, twin = rec.Handles(), rec.Handles()
    try:
        od, ad = hs.dims("walker")
        table, n_layers, base = rec.nets(od, ad)
        for x in (hs, twin):
            assert x.call("walker", "mocca_set_history", [{"i32": [0, 1]}, 2, ad, 2, 1])[0] == 0
            assert x.call("walker", "mocca_set_policy", [table, n_layers, od, ad, 5.0])[0] == 0
            assert x.call("walker", "mocca_update_policy", [{"dev_f32n": [base, 0.01]}, base, None])[0] == 0
        rc, msg = hs.call("walker", "mocca_set_history", [{"i32": [0, 0]}, 2, ad, 2, 1])
        assert rc == -1 and msg == "mocca_set_history: column 0 is repeated"
        rc, msg = hs.call("walker", "mocca_set_policy", [table, n_layers, od, 0, 5.0])
        assert rc == -1 and msg == "mocca_set_policy: act_dim must be 1 .. 32"
        _same_bits(_rollout(hs, "walker", torch, True), _rollout(twin, "walker", torch, True), torch)
    finally:
        hs.close()
        twin.close()
