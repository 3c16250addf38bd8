"""The layer loop the three MFMA MLP kernels share (csrc/mocca_mlp.h: mfma_layer) changes no result bit: act() plain and mirror-symmetric
(policy_kernel), plan_step()'s base outputs (controller_kernel) and ppo_grad() in its four modes (ppo_rows_kernel and the launches behind it)
must hash to what the library of the commit BEFORE the kernels shared the loop produced (tests/golden/mlp_bits.json, written by
tools/record_mlp_bits.py from that library on an MI355X).  One SHA-256 per case over the raw output bytes; no tolerance.  The cases and why
they are the smallest that exercise every path of the loop: tools/record_mlp_bits.py.  Needs a real MI355X: -m gpu."""
import importlib.util
import json
import os

import pytest

_spec = importlib.util.spec_from_file_location("record_mlp_bits", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_mlp_bits.py"))
rmb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rmb)

pytestmark = pytest.mark.gpu
N_CASES = {"act": 4 * 2 * 3 * 2, "plan_step": 3 * 3 * 2, "ppo_grad": 4 * 4 * 3 * 2}      # nets x forms x batches x modes: no case may go missing


@pytest.mark.parametrize("group", list(rmb.GROUPS))
def test_outputs_hash_to_the_parents(group):
    with open(rmb.GOLDEN) as f:
        want = {k: v for k, v in json.load(f).items() if k.startswith(group + "/")}
    got = rmb.GROUPS[group]()
    assert len(want) == N_CASES[group] and sorted(got) == sorted(want), "the recording is of other cases: run tools/record_mlp_bits.py on the parent's library"
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, (f"{len(differ)} of {len(want)} cases differ from the parent's bits", differ[:8])


def test_detaching_another_kind_leaves_the_attached_mirror_alone():
    """The handle holds ONE mirror attachment (symmetric network, mirror loss or duplicated rows).  With kind Y attached, detaching each
    other kind X through the Python surface returns without error and ppo_grad() gives the bytes it gave before: a detach of what is not
    attached is a no-op, not a detach of what is.  Detaching Y itself then gives the plain policy's bytes.  "small", 17 rows."""
    import numpy as np
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    net, kinds = rmb.NETS[0], ("sym", "mirror", "dup")
    p, dp = rmb._policy(net)
    tables = rmb._tables(net)
    d = {k: torch.from_numpy(v).cuda() for k, v in rmb.storage(p, net).items()}
    idx = torch.from_numpy(np.random.default_rng([17, 17]).permutation(rmb.PPO_STORAGE)[:17].astype(np.int64)).cuda()
    env = VecEnv("Walker3DCustomEnv-v0", 4, seed=3)

    def grad():
        o = env.ppo_grad(d["obs"], d["action"], d["old_logp"], d["adv"], d["returns"], idx=idx, old_value=d["old_value"], value_clip=True, **rmb.KW)
        return rmb._digest(o["grad"], o["stats"])

    try:
        env.set_policy(dp)
        plain = grad()
        seen = {plain}
        for attached in kinds:
            rmb.attach(env, attached, tables)
            before = grad()
            for other in kinds:
                if other != attached:
                    rmb.attach(env, other, None)
                    assert grad() == before, (attached, other)
            held = {"sym": getattr(env.policy, "symmetry", None), "mirror": env.mirror_loss, "dup": env.mirror_dup}
            assert [k for k in kinds if held[k] is not None] == [attached], (attached, held)
            seen.add(before)
            rmb.attach(env, attached, None)
            assert grad() == plain, attached
        assert len(seen) == 4, "the four modes are four different functions"
    finally:
        env.close()
