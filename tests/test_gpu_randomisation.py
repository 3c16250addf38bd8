"""Domain randomisation on the GPU (include/mocca.h mocca_set_randomisation .. mocca_randomisation_record): the perturb kernel in front of
the step, the sensor noise and the record, all BY BITS against the numpy restatement (tests/randomisation_reference.py, which
tests/test_randomisation.py holds to the header) and against twin handles that are driven with the restated values.  N = 67 (no multiple
of any tile) and N = 5, 16 steps at most, seed 0: among 67 envs every delay 0 .. 3 and every phase 0 .. 3 occurs (asserted on the CPU)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import randomisation_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mocca_envs_amd import lib as L  # noqa: E402
from mocca_envs_amd import model as M  # noqa: E402
from mocca_envs_amd.randomisation import Randomisation  # noqa: E402
from mocca_envs_amd.vec_env import VecEnv  # noqa: E402

SEED = 0
CUSTOM, STEPPER = "Walker3DCustomEnv-v0", "Walker3DStepperEnv-v0"
FULL = Randomisation(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5))
FULL_CFG = R.Config(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _same(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _env(n, env_id=CUSTOM, **kw):
    return VecEnv(env_id, n, device=0, seed=SEED, **kw)


def _counters(env):
    """(T, E) of every env as the task record holds them now: what the next launch keys its draws by"""
    tk = _np(env.get_task())
    return tk[:, M.TW.T].astype(np.int64), tk[:, M.TW.EPISODE].view(np.uint32).astype(np.int64)


def _actions(n, act_dim, steps, scale, seed=1):
    a = np.random.default_rng(seed).uniform(-scale, scale, (steps, n, act_dim)).astype(np.float32)
    return a, torch.from_numpy(a).cuda()


def _near_timeout(env, every=3, left=2):
    """envs 0, every, 2 every, ..: `left` steps before the TimeLimit, so that the step kernel's auto-reset runs inside the test"""
    tk = env.get_task().clone()
    tk[::every, M.TW.T] = int(env.model.max_episode_steps) - left
    env.set_task(tk)


def _outputs_agree(a, b, what):
    torch.cuda.synchronize()
    for name, x, y in (("obs", a.obs, b.obs), ("rew", a.rew, b.rew), ("done", a.done, b.done), ("info", a.info, b.info),
                       ("state", a.get_state(), b.get_state()), ("task", a.get_task(), b.get_task())):
        assert _same(x, y), (what, name)


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 5])
def test_identity_randomisation_changes_nothing(n):
    """strength [1, 1], delay [0, 0], no push, no noise, auto-reset: every output equals a twin's with nothing attached over 12 steps (the
    actions lie in [-1, 1], where the clip is the identity: the step's energy penalty reads the buffer it is given); effective_action is
    the clipped action, shown on a thirteenth step with actions beyond the clip"""
    A, B = _env(n), _env(n)
    A.set_randomisation(Randomisation())
    A.reset(), B.reset()
    _near_timeout(A), _near_timeout(B)
    act_np, act = _actions(n, A.act_dim, 13, 1.0)
    resets = 0
    for t in range(12):
        A.step(act[t]), B.step(act[t])
        _outputs_agree(A, B, t)
        assert _same(A.effective_action(), act_np[t])
        resets += int((_np(A.done) != 0).sum())
    assert resets >= (n + 2) // 3                         # the auto-reset ran inside the comparison
    wide = (1.5 * act[12]).contiguous()
    clipped = R.clip(_np(wide))
    A.step(wide), B.step(torch.from_numpy(clipped).cuda())
    assert _same(A.effective_action(), clipped) and np.abs(_np(wide)).max() > 1.0
    _outputs_agree(A, B, "clipped")
    A.set_randomisation(None)                              # detached: the handle is the twin again
    A.step(wide), B.step(wide)
    _outputs_agree(A, B, "detached")
    with pytest.raises(L.MoccaError, match="mocca_get_effective_action needs a randomisation"):
        A.effective_action()
    A.close(), B.close()


# ---- 2. strength and latency -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 5])
def test_strength_and_latency_equal_the_restatement_and_a_twin(n):
    """range 0.5 .. 1, delays 0 .. 3, actions 1.5 x uniform (the clip acts), mocca_reset of a third of the envs after step 6 and the
    step kernel's auto-reset: effective_action equals the restatement, and a twin that is FED the restated actions agrees on everything"""
    A, B = _env(n), _env(n)
    A.set_randomisation(Randomisation(strength=(0.5, 1.0), latency=(0, 3)))
    cfg = R.Config(strength=(0.5, 1.0), latency=(0, 3))
    plant = R.Plant(SEED, np.arange(n), cfg, A.act_dim)
    A.reset(), B.reset()
    _near_timeout(A, every=4, left=3), _near_timeout(B, every=4, left=3)
    act_np, act = _actions(n, A.act_dim, 14, 1.5)
    delays, zeros = set(), 0
    for t in range(14):
        T, E = _counters(A)
        eff, _, _ = plant.step(act_np[t], T, E)
        delays |= set(R.episode_params(SEED, np.arange(n), E, cfg)[1].tolist())
        zeros += int((T < R.episode_params(SEED, np.arange(n), E, cfg)[1]).sum())
        A.step(act[t]), B.step(torch.from_numpy(eff).cuda())
        assert _same(A.effective_action(), eff), t
        _outputs_agree(A, B, t)
        if t == 6:
            mask = torch.zeros(n, dtype=torch.uint8)
            mask[1::3] = 1
            A.reset(mask), B.reset(mask)
    assert zeros > 0 and (delays == {0, 1, 2, 3} if n == 67 else len(delays) > 1)
    A.close(), B.close()


# ---- 3. pushes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,n", [(CUSTOM, 67), (CUSTOM, 5), ("Walker2DCustomEnv-v0", 5)])
def test_pushes_equal_a_twin_pushed_through_set_state(env_id, n):
    """interval 4, max 0.5: the twin gets the restated dv added to words 7 and 8 of its state through get_state / set_state before each
    step; states agree after each of 12 steps.  The planar walker takes dvx alone: its restated dvy is 0 and word 8 is the twin's"""
    planar = env_id != CUSTOM
    A, B = _env(n, env_id), _env(n, env_id)
    A.set_randomisation(Randomisation(push=(4, 0.5)))
    cfg = R.Config(push=(4, 0.5), planar=planar)
    A.reset(), B.reset()
    act_np, act = _actions(n, A.act_dim, 12, 1.0)
    fired, vy_pushed = 0, 0
    for t in range(12):
        T, E = _counters(A)
        phase = R.episode_params(SEED, np.arange(n), E, cfg)[2]
        fires, dv = R.push(SEED, np.arange(n), T, E, cfg, phase)
        st = _np(B.get_state()).copy()
        st[fires, 7] = st[fires, 7] + dv[fires, 0]
        if not planar:
            st[fires, 8] = st[fires, 8] + dv[fires, 1]
        B.set_state(st)
        fired += int(fires.sum())
        vy_pushed += int((dv[:, 1] != 0).sum())
        assert (np.abs(dv) <= 0.5).all() and not fires[T == 0].any()
        A.step(act[t]), B.step(act[t])
        _outputs_agree(A, B, t)
    assert fired >= n and (vy_pushed == 0 if planar else vy_pushed >= n)
    A.close(), B.close()


# ---- 4. sensor noise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,dim", [(CUSTOM, 52), (STEPPER, 65)])
@pytest.mark.parametrize("n", [67, 5])
def test_sensor_noise_equals_the_restatement(env_id, dim, n):
    """widths 52 and 65 (one more than a wave: 17 blocks, the last one ragged), row strides wider than dim, in place and out of place,
    sentinel columns intact, and the same rows from two calls without a step"""
    A = _env(n, env_id)
    assert A.obs_dim == dim
    A.reset()
    A.step(torch.zeros(n, A.act_dim, device="cuda")), A.step(torch.zeros(n, A.act_dim, device="cuda"))
    T, E = _counters(A)
    assert (T > 0).any()
    rng = np.random.default_rng(dim)
    scale = (2.0 ** -rng.integers(1, 9, dim)).astype(np.float32)
    scale[3] = 0.0                                         # a column without noise
    A.set_sensor_noise(scale)
    rows_np = np.full((n, dim + 5), 77.0, np.float32)
    rows_np[:, :dim] = rng.integers(-64, 65, (n, dim)) / 16.0
    want = R.noise(SEED, np.arange(n), T, E, rows_np, scale)
    assert _same(want[:, 3], rows_np[:, 3]) and (want[:, :3] != rows_np[:, :3]).mean() > 0.9
    rows = torch.from_numpy(rows_np).cuda()
    out = torch.full((n, dim + 9), -5.0, device="cuda")
    got = A.sensor_noise(rows, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _same(out[:, :dim], want) and bool((out[:, dim:] == -5.0).all()) and _same(rows, rows_np)       # out of place: the input is intact
    again = torch.full((n, dim + 9), -5.0, device="cuda")
    A.sensor_noise(rows, out=again)
    assert _same(again, out)
    A.sensor_noise(rows)                                   # in place
    assert _same(rows[:, :dim], want) and bool((rows[:, dim:] == 77.0).all())
    A.close()


# ---- 5. the record -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 5])
def test_record_equals_the_restatement_also_after_an_auto_reset(n):
    A = _env(n)
    A.set_randomisation(FULL)
    A.reset()
    _near_timeout(A)
    _, act = _actions(n, A.act_dim, 8, 1.0)
    wide = torch.full((n, 9), 3.0, device="cuda")
    seen_reset = False
    for t in range(8):
        T, E = _counters(A)
        want = R.record(SEED, np.arange(n), T, E, FULL_CFG)
        assert _same(A.randomisation_record(), want), t
        A.randomisation_record(out=wide[:, 2:])            # a strided tail: the columns around it stay
        assert _same(wide[:, 2:6], want) and bool((wide[:, :2] == 3.0).all()) and bool((wide[:, 6:] == 3.0).all())
        if t > 0 and (T == 0).any():
            seen_reset = True                              # these rows describe the NEW episode: its own strength, delay and phase
            assert (E[T == 0] >= 1).all()
        assert ((want[:, 2] >= 0) & (want[:, 2] <= 4)).all() and ((want[:, 0] >= 0.5) & (want[:, 0] <= 1.0)).all()
        A.step(act[t])
    assert seen_reset
    A.close()


# ---- 6. sharding -------------------------------------------------------------------------------------------------------------------------
def test_two_shards_reproduce_the_rows_they_own():
    """N = 8 against two handles of 4 with env_offset 0 and 4: effective actions, observations, states, records and noise, the same rows"""
    whole, parts = _env(8), [_env(4, env_offset=0), _env(4, env_offset=4)]
    rand = Randomisation(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5), obs_noise=2 ** -5)
    for e in [whole] + parts:
        e.set_randomisation(rand)
        e.reset()
    _, act = _actions(8, whole.act_dim, 10, 1.5)
    for t in range(10):
        whole.step(act[t])
        for e, sl in zip(parts, (slice(0, 4), slice(4, 8))):
            e.step(act[t, sl].contiguous())
            torch.cuda.synchronize()
            for name, x, y in (("eff", whole.effective_action(), e.effective_action()), ("obs", whole.obs, e.obs), ("state", whole.get_state(), e.get_state()),
                               ("record", whole.randomisation_record(), e.randomisation_record()),
                               ("noise", whole.sensor_noise(whole.obs, out=torch.zeros_like(whole.obs)), e.sensor_noise(e.obs, out=torch.zeros_like(e.obs)))):
                assert _same(x[sl], y), (t, name)
    assert not _same(whole.randomisation_record()[:4], whole.randomisation_record()[4:])
    for e in [whole] + parts:
        e.close()


# ---- 7. graph capture --------------------------------------------------------------------------------------------------------------------
def test_act_step_with_everything_attached_replays_like_eager():
    """one act_step (policy, perturb, step), the record and the sensor noise captured in ONE graph on a single stream: six replays equal six
    eager steps of a twin, by bits"""
    import policy_reference as PR
    from mocca_envs_amd.policy import DevicePolicy
    n = 67
    p = PR.random_policy("ppo", 52, 21, norm=True, seed=4)
    dp = DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)
    rand = Randomisation(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5), obs_noise=2 ** -6)
    E_, G_ = _env(n), _env(n)
    bufs = {}
    for name, e in (("E", E_), ("G", G_)):
        e.set_randomisation(rand)
        e.set_policy(dp)
        e.reset()
        bufs[name] = dict(row=torch.zeros(n, 52, device="cuda"), rec=torch.zeros(n, 4, device="cuda"), act=torch.zeros(n, 21, device="cuda"))
        bufs[name]["row"].copy_(e.obs)

    def one(e, b):
        e.act_step(b["row"], action_out=b["act"])
        e.randomisation_record(out=b["rec"])
        e.sensor_noise(e.obs, out=b["row"])                # the policy's next input: the noisy observation

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one(G_, bufs["G"]), one(G_, bufs["G"])             # warm-up ahead of the capture, as torch requires
    torch.cuda.current_stream().wait_stream(side)
    one(E_, bufs["E"]), one(E_, bufs["E"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one(G_, bufs["G"])
    for t in range(6):
        graph.replay()
        one(E_, bufs["E"])
        torch.cuda.synchronize()
        for k in ("row", "rec", "act"):
            assert _same(bufs["E"][k], bufs["G"][k]), (t, k)
        assert _same(E_.effective_action(), G_.effective_action()), t
        _outputs_agree(E_, G_, t)
    assert not _same(bufs["G"]["row"], G_.obs)              # the noise is there
    E_.close(), G_.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_handle_and_outputs_unchanged():
    n = 5
    A, B = _env(n), _env(n)
    for e in (A, B):
        e.set_randomisation(Randomisation(strength=(0.5, 1.0), latency=(0, 2), push=(4, 0.5), obs_noise=2 ** -4))
        e.reset()
    lib, h = A.lib, A.h
    cfg = lambda **kw: L.RandomisationConfig(**{**dict(strength_lo=0.5, strength_hi=1.0, delay_min=0, delay_max=2, push_interval=4, push_max=0.5), **kw})
    nan, inf = float("nan"), float("inf")
    bad = [dict(strength_lo=0.0), dict(strength_lo=-0.5), dict(strength_hi=1.5), dict(strength_lo=1.0, strength_hi=0.5), dict(strength_lo=nan),
           dict(strength_hi=nan), dict(delay_min=-1), dict(delay_min=2, delay_max=1), dict(delay_max=8), dict(push_max=-0.5), dict(push_max=nan),
           dict(push_max=inf), dict(push_interval=-1), dict(push_interval=65537)]
    for kw in bad:
        c = cfg(**kw)
        assert lib.mocca_set_randomisation(h, C.byref(c)) == -1, kw
        assert (lib.mocca_last_error(h) or b"").decode().startswith("mocca_set_randomisation:"), kw
    ok = np.full(A.obs_dim, 0.25, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for scales, dim, word in ((ok, A.obs_dim - 1, "obs_dim"), (np.full(A.obs_dim + 1, 0.25, np.float32), A.obs_dim + 1, "obs_dim"),
                              (np.where(np.arange(A.obs_dim) == 7, -0.25, ok).astype(np.float32), A.obs_dim, "scale 7"),
                              (np.where(np.arange(A.obs_dim) == 9, nan, ok).astype(np.float32), A.obs_dim, "scale 9"),
                              (np.where(np.arange(A.obs_dim) == 2, inf, ok).astype(np.float32), A.obs_dim, "scale 2")):
        assert lib.mocca_set_sensor_noise(h, ptr(scales), dim) == -1 and word in lib.mocca_last_error(h).decode(), word
    # strides narrower than the row, NULL pointers: nothing is written
    rows, out, rec = (torch.full((n, w), 9.0, device="cuda") for w in (A.obs_dim, A.obs_dim, 4))
    vp = lambda t: C.c_void_p(t.data_ptr())
    s = A._stream()
    for args in ((vp(rows), A.obs_dim - 1, vp(out), A.obs_dim), (vp(rows), A.obs_dim, vp(out), A.obs_dim - 1), (None, A.obs_dim, vp(out), A.obs_dim),
                 (vp(rows), A.obs_dim, None, A.obs_dim)):
        assert lib.mocca_sensor_noise(h, *args, s) == -1 and lib.mocca_last_error(h).decode().startswith("mocca_sensor_noise")
    assert lib.mocca_randomisation_record(h, vp(rec), 3, s) == -1 and "row_stride" in lib.mocca_last_error(h).decode()
    assert lib.mocca_randomisation_record(h, None, 4, s) == -1 and lib.mocca_get_effective_action(h, None, s) == -1
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((rec == 9.0).all())
    # the handle is as it was: it goes on exactly like its twin, which saw none of this
    _, act = _actions(n, A.act_dim, 4, 1.5)
    for t in range(4):
        A.step(act[t]), B.step(act[t])
        _outputs_agree(A, B, t)
        assert _same(A.effective_action(), B.effective_action()) and _same(A.randomisation_record(), B.randomisation_record())
        assert _same(A.sensor_noise(A.obs, out=torch.zeros_like(A.obs)), B.sensor_noise(B.obs, out=torch.zeros_like(B.obs)))
    # the calls without their setter
    fresh = _env(n)
    fresh.reset()
    for call, word in ((lambda: fresh.sensor_noise(fresh.obs.clone()), "mocca_set_sensor_noise"), (fresh.randomisation_record, "mocca_set_randomisation"),
                       (fresh.effective_action, "mocca_set_randomisation")):
        with pytest.raises(L.MoccaError, match=word):
            call()
    with pytest.raises(ValueError):
        fresh.set_randomisation(Randomisation(obs_noise=[0.1] * 3))
    with pytest.raises(L.MoccaError, match="needs a randomisation"):   # ... which refused before the handle changed
        fresh.effective_action()
    # Cassie's action is a PD target: no strength; latency and pushes are fine
    cas = _env(n, "CassieEnv-v0")
    with pytest.raises(L.MoccaError, match="MOCCA_TASK_CASSIE"):
        cas.set_randomisation(Randomisation(strength=(0.5, 1.0)))
    cas.set_randomisation(Randomisation(latency=(0, 2), push=(4, 0.25)))
    cas.reset()
    cas.step(torch.zeros(n, cas.act_dim, device="cuda"))
    assert _same(cas.randomisation_record()[:, 0], np.ones(n, np.float32))
    for e in (A, B, fresh, cas):
        e.close()


# ---- 9. the trainer surface --------------------------------------------------------------------------------------------------------------
def test_trainer_rows_noise_and_privileged_record():
    """make_vec_envs(privileged_scan=, randomisation=Randomisation(obs_noise=2^-6, privileged=True)): the head of envs.privileged is the
    observation of a twin without noise, the policy's row differs from it by exactly the restated noise, the tail is the record;
    attach_policy refuses a critic of the old width"""
    import ppo_priv_reference as P
    from mocca_envs_amd.perception import scan_grid
    from mocca_envs_amd.trainer_api import make_vec_envs
    n = 67
    scan = dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), 3, 2), z_above=1.0, max_drop=2.0)
    plant = dict(strength=(0.5, 1.0), latency=(0, 3), push=(4, 0.5))
    A = make_vec_envs(CUSTOM, SEED, n, None, privileged_scan=scan, randomisation=Randomisation(obs_noise=2 ** -6, privileged=True, **plant))
    twin = make_vec_envs(CUSTOM, SEED, n, None, privileged_scan=scan, randomisation=Randomisation(**plant))
    d = A.venv.obs_dim
    assert A.privileged.shape == (n, d + 6 + 4) and twin.privileged.shape == (n, d + 6) and A.randomisation.shape == (n, 4)
    assert A.randomisation.data_ptr() == A.privileged[:, d + 6:].data_ptr()
    with pytest.raises(ValueError, match="privileged_scan"):
        make_vec_envs(CUSTOM, SEED, n, None, randomisation=Randomisation(privileged=True))
    with pytest.raises(NotImplementedError, match="one handle"):
        make_vec_envs(CUSTOM, SEED, n, None, randomisation=Randomisation(), sub_batches=2)
    with pytest.raises(ValueError, match="critic reads"):
        A.attach_policy(P.device_policy(P.make_policy("ppo", in_dim=d, critic_in_dim=d + 6, norm=True, seed=3)))      # the old width
    A.attach_policy(P.device_policy(P.make_policy("ppo", in_dim=d, critic_in_dim=d + 10, norm=True, seed=3)))
    scale = np.full(d, 2 ** -6, np.float32)
    storage = torch.zeros(3, n, d, device="cuda")           # into= rows of a trainer's storage
    _, act = _actions(n, A.venv.act_dim, 6, 1.5)

    def check(row, clean, t):
        torch.cuda.synchronize()
        T, E = _counters(A.venv)
        assert _same(A.privileged[:, :d], clean) and _same(A.privileged[:, :d + 6], twin.privileged), t
        assert _same(row, R.noise(SEED, np.arange(n), T, E, _np(clean), scale)) and not _same(row, clean), t
        want = R.record(SEED, np.arange(n), T, E, FULL_CFG)
        assert _same(A.privileged[:, d + 6:], want) and _same(A.randomisation, want) and _same(twin.randomisation, want), t

    check(A.reset(), twin.reset(), "reset")
    for t in range(6):
        into = {"obs": storage[t % 3]} if t % 2 else None
        row = A.step(act[t], into=into)[0]
        clean = twin.step(act[t])[0]
        assert into is None or row.data_ptr() == storage[t % 3].data_ptr()
        check(row, clean, t)
    assert _same(A.effective_action(), twin.effective_action())
    A.close(), twin.close()


# ---- 10. the tools -----------------------------------------------------------------------------------------------------------------------
def test_ppo_demo_trains_under_a_randomisation_and_the_eval_tool_plays_its_policy(tmp_path, capsys):
    """tools/ppo_demo.py with the --rand-* flags, imported and driven, 64 envs x 8 steps, two iterations on the device arm: the policy file
    records the randomisation; tools/randomisation_eval.py plays it under the plain and under a randomised plant, 8 short episodes"""
    import importlib.util
    import json
    root = os.path.dirname(HERE)

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    out = str(tmp_path / "run")
    flags = ["--rand-strength", "0.5,1", "--rand-latency", "0,2", "--rand-push", "4,0.5", "--obs-noise", "0.02"]
    tool("ppo_demo").main(["--envs", "64", "--steps", "8", "--iters", "2", "--device-policy", "--device-returns", "--device-grad", "--device-update",
                           "--out", out] + flags)
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert lines and all(np.isfinite(x["mean_return"]) for x in lines)
    with np.load(out + "_policy.npz", allow_pickle=False) as z:
        assert Randomisation.from_dict(json.loads(str(z["randomisation"]))) == Randomisation(strength=(0.5, 1), latency=(0, 2), push=(4, 0.5), obs_noise=0.02)
    ev = tool("randomisation_eval")
    ev.main(["--policy", f"p={out}_policy.npz", "--envs", "8", "--max-steps", "20", "--out", out + "_eval.jsonl"])
    ev.main(["--policy", f"p={out}_policy.npz", "--envs", "8", "--max-steps", "20", "--out", out + "_eval.jsonl"] + flags)
    rows = [json.loads(x) for x in open(out + "_eval.jsonl")]
    assert [r["condition"] for r in rows] == ["plain", "randomised"] and rows[0]["evaluated_under"] is None
    assert rows[1]["evaluated_under"] == rows[1]["trained_under"] and all(np.isfinite(r["mean_return"]) and 0 < r["mean_length"] <= 20 for r in rows)
    with pytest.raises(SystemExit):
        tool("ppo_demo").main(["--rand-privileged", "--out", out])
