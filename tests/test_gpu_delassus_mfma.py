"""The Delassus matrix built on the matrix pipe (delassus_mfma, mocca_device.h) against the VALU build it replaces (MOCCA_PARAM_KERNEL_VARIANT
bit 2 forces the latter for every row count): v_mfma_f32_16x16x4_f32 evaluates the same k-ordered fma chain, and the tile store sends every
product where delassus_store leaves it, so two handles of the same env id, seed and action tape must agree BIT FOR BIT after every step --
observations, rewards, done flags, info, state, task records and the debug record (active sets, clamp masks, step signature).  No tolerance.

The batches are chosen so that the sample meets every path through the build; the test asserts that it did, from the row count of each
step's last substep (debug word 0): 1 row, 2 rows (even: both orientations of the one pair are kept), odd counts within one tile, exactly 16,
17..31 (four tiles), exactly 32, 33 or more (the VALU build on both sides) and substeps with a two-body row (a self contact).  For these seeds
the f32 CPU oracle (oracle/oracle.py, same blobs, same tapes, 256 envs x 200 steps) holds, per class of last substeps:
    Custom, U(-1, 1):      1: 3620   2: 5391   odd <= 15: 21132   16: 313    17..31: 572     two-body: 8260
    Custom, zero actions:                      odd <= 15: 13337   16: 4716   17..31: 17787
    Stepper, curriculum 9: 1: 1301   2: 2065   odd <= 15: 17633   16: 1858   17..31: 11907   32: 101   >= 33: 304   two-body: 14638
    Custom, max_rows = 32 (compact instance: one tile up to 16 rows, the VALU build above):  16: 313   17: 216
Fewer than 8 rows (MOCCA_DELASSUS_MFMA_MIN) take the VALU build on both sides; the classes 1, 2 and the small odd counts stay asserted, and the
sample must also hold the threshold's two sides (7 and 8 rows) and, within one tile, even counts 8..14 (both orientations at distance nr / 2;
oracle: 7603 / 8867 / 10104 in the three 48-row batches) and odd counts 9..15 (5839 / 11754 / 9754).
Needs a real MI355X: -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, SEED, TAPE_SEED = 256, 200, 21, 3

#          id                       env id                   zero    curriculum  max_rows  classes the sample must hold
BATCHES = [("custom_uniform", "Walker3DCustomEnv-v0", False, None, None, ("1", "2", "odd<=15", "7", "8", "even8..14", "odd9..15", "16", "17..31", "two_body")),
           ("custom_zero", "Walker3DCustomEnv-v0", True, None, None, ("odd<=15", "even8..14", "odd9..15", "16", "17..31")),
           ("stepper_c9", "Walker3DStepperEnv-v0", False, 9, None, ("1", "2", "odd<=15", "7", "8", "even8..14", "odd9..15", "16", "17..31", "32", ">=33", "two_body")),
           ("custom_compact", "Walker3DCustomEnv-v0", False, None, 32, ("7", "8", "even8..14", "odd9..15", "16", "17"))]


def _classes(rec, max_rows, max_contacts):
    r, nc, selfp = rec[:, 0], rec[:, 2], rec[:, 7]
    return {"7": r == 7, "8": r == 8, "even8..14": (r % 2 == 0) & (r >= 8) & (r <= 14), "odd9..15": (r % 2 == 1) & (r >= 9) & (r <= 15), "1": r == 1, "2": r == 2, "odd<=15": (r % 2 == 1) & (r > 1) & (r <= 15), "16": r == 16, "17": r == 17, "17..31": (r >= 17) & (r <= 31),
            "32": r == 32, ">=33": r >= 33,
            # a self contact within the margin and nothing dropped by the caps: its three rows act on two bodies
            "two_body": (selfp > 0) & (r > 0) & (r < max_rows) & (nc < max_contacts)}


@pytest.mark.parametrize("name,env_id,zero,curriculum,max_rows,must_hold", BATCHES, ids=[b[0] for b in BATCHES])
def test_matrix_pipe_and_valu_builds_agree_bit_for_bit(name, env_id, zero, curriculum, max_rows, must_hold):
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    kw = {} if max_rows is None else {"max_rows": max_rows}
    a_env = VecEnv(env_id, N, auto_reset=True, seed=SEED, **kw)
    b_env = VecEnv(env_id, N, auto_reset=True, seed=SEED, **kw)
    b_env.set_param(L.PARAM_KERNEL_VARIANT, 4)                 # bit 2: the VALU build for every row count; the instance stays the automatic one
    ka, kb = a_env.kernel_info(), b_env.kernel_info()
    assert ka["lds_bytes"] == kb["lds_bytes"] and (ka["lds_bytes"] <= 8192) == (max_rows is not None), (ka, kb)
    if curriculum is not None:
        a_env.set_param(L.PARAM_CURRICULUM, curriculum); b_env.set_param(L.PARAM_CURRICULUM, curriculum)
    dbg_a, dbg_b = a_env.set_debug(True), b_env.set_debug(True)
    assert torch.equal(a_env.reset(), b_env.reset())
    nd = 13 + 2 * a_env.model.n_joints       # (the slots' impulses behind the dynamic state are neither loaded nor stored by these blobs)
    rng = np.random.default_rng(TAPE_SEED)
    rec = []
    for t in range(STEPS):
        act_np = np.zeros((N, a_env.act_dim), np.float32) if zero else rng.uniform(-1, 1, (N, a_env.act_dim)).astype(np.float32)
        act = torch.from_numpy(act_np).cuda()
        for k, (x, y) in enumerate(zip(a_env.step(act), b_env.step(act))):
            assert torch.equal(x, y), (name, t, ("obs", "reward", "done", "info")[k])
        assert torch.equal(dbg_a, dbg_b), (name, t)              # rows, active sets, clamp masks and signature, step signature (words 16, 17)
        assert torch.equal(a_env.get_state()[:, :nd], b_env.get_state()[:, :nd]), (name, t)
        assert torch.equal(a_env.get_task(), b_env.get_task()), (name, t)
        rec.append(dbg_a.clone())
    if "Stepper" in env_id:
        assert torch.equal(a_env.get_terrain(), b_env.get_terrain())
    rec = torch.cat(rec).cpu().numpy()
    held = {k: int(v.sum()) for k, v in _classes(rec, int(a_env.model.max_rows), int(a_env.model.max_contacts)).items()}
    print(name, held)
    for k in must_hold:
        assert held[k] > 0, (name, k, held)
    a_env.close(); b_env.close()


def test_variant_bits():
    """Bits 0..1 keep naming the instance, bit 2 is independent of them; 3 and values beyond 7 name nothing."""
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv
    env = VecEnv("Walker3DCustomEnv-v0", 4, max_rows=32)
    compact = env.kernel_info()["lds_bytes"]
    for v, same in ((4, True), (1, False), (5, False), (6, False), (0, True)):
        env.set_param(L.PARAM_KERNEL_VARIANT, v)
        assert (env.kernel_info()["lds_bytes"] == compact) == same, v
    for v in (3, 7, 8, -1, 0.5):
        with pytest.raises(L.MoccaError):
            env.set_param(L.PARAM_KERNEL_VARIANT, v)
    env.close()
