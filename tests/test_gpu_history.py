"""The observation-action history on the GPU (include/mocca.h mocca_set_history / mocca_history): the kernel BY BITS against the numpy
restatement (tests/history_reference.py, which tests/test_history.py holds to the header), against twin handles, through the trainer's rows,
act_step, a captured rollout, the mirror tables and the tools.  N = 67 (env blocks straddle workgroups) and N = 5 (most of one workgroup
idle), 16 steps at most, the four configurations of the CPU test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import history_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mocca_envs_amd import lib as L  # noqa: E402
from mocca_envs_amd import model as M  # noqa: E402
from mocca_envs_amd.history import History  # noqa: E402
from mocca_envs_amd.vec_env import VecEnv  # noqa: E402

SEED = 0
CUSTOM = "Walker3DCustomEnv-v0"
OBS, ACT = 52, 21
CONFIGS = {                                           # name -> (K, s, columns, A): tests/test_history.py's
    "k3_all": (3, 1, list(range(OBS)), ACT),
    "k2_s3_some": (2, 3, [0, 5, 6, 17, 30, 44, 51], ACT),
    "k4_s2_actions_only": (4, 2, [], ACT),
    "k16_one_column": (16, 1, [0], 0),
}


def _history(name):
    K, s, cols, A = CONFIGS[name]
    return History(K, stride=s, columns=None if len(cols) == OBS else cols, actions=bool(A))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _same(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _env(n, env_id=CUSTOM, **kw):
    return VecEnv(env_id, n, device=0, seed=SEED, **kw)


def _counters(env):
    """(T, E) of every env as the task record holds them now: what the next history launch keys its frames by"""
    tk = _np(env.get_task())
    return tk[:, M.TW.T].astype(np.int64), tk[:, M.TW.EPISODE].view(np.uint32).astype(np.int64)


def _actions(n, act_dim, steps, seed=1):
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (steps, n, act_dim)).astype(np.float32)
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


def _full(block, pairs):
    """does some env's block hold something in every one of its `pairs` pairs?"""
    b = _np(block)
    return bool((b.reshape(b.shape[0], pairs, -1) != 0).any(-1).all(-1).any())


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------------
CASES = [(n, name, "strided") for n in (67, 5) for name in CONFIGS] + [(67, "k3_all", "in_place"), (5, "k2_s3_some", "in_place"),
                                                                         (67, "k3_all", "no_act"), (5, "k4_s2_actions_only", "no_act")]


@pytest.mark.parametrize("n,name,mode", CASES)
def test_history_equals_the_restatement(n, name, mode):
    """16 steps of VecEnv.step + history: the auto-reset inside the comparison (the TimeLimit two steps away for a third of the envs, which
    is a T jump through set_task as well), a masked reset of another third after step 6, one skipped call (step 9).  `strided`: the block goes
    to columns 3 .. of rows wider than it, between sentinels; `in_place`: it is the tail of the very row whose head is read; `no_act`: no
    call brings an action"""
    K, s, cols, A = CONFIGS[name]
    dim = K * (len(cols) + A)
    env = _env(n)
    env.set_history(_history(name))
    assert env.history_dim == dim
    ref = R.History(n, K, s, cols, A)
    act_np, act = _actions(n, ACT, 16)
    out = torch.full((n, dim + 7), -5.0, device="cuda")
    wide = torch.full((n, OBS + dim + 2), -7.0, device="cuda")
    resets, seen = 0, 0

    def call(a_np, a):
        nonlocal seen
        if mode == "no_act":
            a_np = a = None
        T, E = _counters(env)
        obs = _np(env.obs).copy()
        want = ref(obs, a_np, T, E)
        if mode == "in_place":
            wide[:, :OBS].copy_(env.obs)
            got = env.history(wide, a, out=wide[:, OBS:])
            assert got.data_ptr() == wide[:, OBS:].data_ptr() and got.shape == (n, dim)
            assert _same(wide[:, :OBS], obs) and bool((wide[:, OBS + dim:] == -7.0).all())        # the head and what lies beyond the block
        else:
            got = env.history(env.obs, a, out=out[:, 3:])
            assert bool((out[:, :3] == -5.0).all()) and bool((out[:, 3 + dim:] == -5.0).all()) and _same(env.obs, obs)
        assert _same(got, want), (T.tolist(), E.tolist())
        seen += int((want != 0).any(1).sum())

    env.reset()
    call(None, None)
    _near_timeout(env)
    for t in range(16):
        env.step(act[t])
        resets += int((_np(env.done) != 0).sum())
        if t != 9:
            call(act_np[t], act[t])
        if t == 6:
            mask = torch.zeros(n, dtype=torch.uint8)
            mask[1::3] = 1
            env.reset(mask)
            call(None, None)          # the other envs' second call on their step: the newest action shows as +0.0
    assert resets >= (n + 2) // 3 and (seen > 8 * n or (mode == "no_act" and not cols))      # (actions only and no action: zeros throughout)
    env.close()


# ---- 2. two calls without a step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 5])
def test_a_second_call_without_a_step_changes_nothing(n):
    A, B = _env(n), _env(n)
    for e in (A, B):
        e.set_history(_history("k3_all"))
        e.reset()
        e.history(e.obs)
    _, act = _actions(n, ACT, 8)
    for t in range(8):
        A.step(act[t]), B.step(act[t])
        first = A.history(A.obs, act[t]).clone()
        if t in (2, 5):
            assert _same(A.history(A.obs, act[t]), first), t
        assert _same(first, B.history(B.obs, act[t])), t      # B calls once per step: the extra calls left the later blocks as they are
    assert _full(first, 3)
    A.close(), B.close()


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 5])
def test_a_twin_without_a_history_agrees_on_everything(n):
    A, B = _env(n), _env(n)
    A.set_history(_history("k2_s3_some"))
    A.reset(), B.reset()
    A.history(A.obs)
    _near_timeout(A), _near_timeout(B)
    _, act = _actions(n, ACT, 9)
    for t in range(6):
        A.step(act[t]), B.step(act[t])
        A.history(A.obs, act[t])
        _outputs_agree(A, B, t)
    A.set_history(None)                                        # detached: the handle is the twin again
    assert A.history_dim == 0 and A.lib.mocca_history_dim(A.h) == -1
    with pytest.raises(L.MoccaError, match="history needs a History"):
        A.history(A.obs)
    for t in range(6, 9):
        A.step(act[t]), B.step(act[t])
        _outputs_agree(A, B, t)
    A.close(), B.close()


# ---- 4. the trainer's rows -----------------------------------------------------------------------------------------------------------------
def test_trainer_rows_hold_what_the_policy_saw():
    """make_vec_envs(height_scan=, depth_camera=, randomisation=Randomisation(obs_noise=0.02), history=History(2)): rows are
    [noisy obs | scan | depth | hist]; the head, scan and depth are a twin's without a history; hist is the restatement fed with the NOISY
    heads and the actions passed, its observation parts the heads of the rows returned one and two steps earlier; step(into=) fills the
    caller's rows.  With privileged_scan= instead: envs.privileged is the twin's."""
    import randomisation_reference as RR
    from mocca_envs_amd.perception import DepthCamera, scan_grid
    from mocca_envs_amd.randomisation import Randomisation
    from mocca_envs_amd.trainer_api import make_vec_envs
    n = 67
    scan = dict(points=scan_grid((0.0, 2.0), (-0.5, 0.5), 3, 2), z_above=1.0, max_drop=2.0)
    cam = DepthCamera(offset=(0.15, 0.0, 0.10), pitch=-35.0, fov_y=90.0, near=0.05, far=6.0, width=4, height=3)
    rand = Randomisation(strength=(0.5, 1.0), latency=(0, 2), push=(4, 0.5), obs_noise=0.02)
    kw = dict(height_scan=scan, depth_camera=cam, randomisation=rand)
    A, twin = make_vec_envs(CUSTOM, SEED, n, None, history=History(2), **kw), make_vec_envs(CUSTOM, SEED, n, None, **kw)
    d, w = A.venv.obs_dim, 2 * (OBS + ACT)
    sensors = d + 6 + 12
    assert A.observation_space.shape == (sensors + w,) and twin.observation_space.shape == (sensors,) and A.venv.history_dim == w
    ref = R.History(n, 2, 1, list(range(OBS)), ACT)
    scale = np.full(d, np.float32(0.02), np.float32)
    storage = torch.zeros(3, n, sensors + w, device="cuda")
    act_np, act = _actions(n, ACT, 8)
    heads, checked, began, lived = [], 0, 0, np.zeros(n, np.int64)     # lived: the frames of its episode an env has behind it, one after the other

    def check(row, clean_row, a_np, t):
        nonlocal checked, began
        torch.cuda.synchronize()
        T, E = _counters(A.venv)
        began += int((T == 0).sum())
        lived[T == 0] = 0                                     # a new episode (the auto-reset inside the step)
        assert _same(row[:, :sensors], clean_row), t                                                   # [noisy obs | scan | depth]: the twin's row
        assert _same(row[:, :d], RR.noise(SEED, np.arange(n), T, E, _np(A.venv.obs), scale)) and not _same(row[:, :d], A.venv.obs), t
        head = _np(row[:, :d]).copy()
        assert _same(row[:, sensors:], ref(head, a_np, T, E)), t
        hist = _np(row[:, sensors:]).reshape(n, 2, OBS + ACT)
        for j in (1, 2):                       # the envs that have lived j steps of their episode: the row returned j steps ago, the action passed on it
            live = lived >= j
            if live.any():
                assert _same(hist[live, j - 1, :OBS], heads[-j][live]) and _same(hist[live, j - 1, OBS:], act_np[t - j + 1][live]), (t, j)
                checked += int(live.sum())
            assert not hist[~live, j - 1].any()
        heads.append(head)
        lived[:] += 1

    check(A.reset(), twin.reset(), None, "reset")
    _near_timeout(A.venv, every=4, left=3), _near_timeout(twin.venv, every=4, left=3)
    lived[::4] = 0                                            # their frame of step 0 is not the frame of the step before T = limit - 3
    for t in range(8):
        into = {"obs": storage[t % 3]} if t % 2 else None
        row = A.step(act[t], into=into)[0]
        assert (row.data_ptr() == storage[t % 3].data_ptr()) if into else (row.data_ptr() == A._wide.data_ptr())
        check(row, twin.step(act[t])[0], act_np[t], t)
    assert checked > 8 * n and began >= n + (n + 3) // 4      # the reset, and the auto-reset of a quarter of the envs inside the comparison
    A.close(), twin.close()
    # the scan kept beside the row: the privileged row is not the history's business
    kw = dict(privileged_scan=scan, randomisation=rand)
    A, twin = make_vec_envs(CUSTOM, SEED, n, None, history=History(2), **kw), make_vec_envs(CUSTOM, SEED, n, None, **kw)
    ref = R.History(n, 2, 1, list(range(OBS)), ACT)
    for t in range(3):
        row, clean = (A.reset(), twin.reset()) if t == 0 else (A.step(act[t])[0], twin.step(act[t])[0])
        torch.cuda.synchronize()
        T, E = _counters(A.venv)
        assert _same(A.privileged, twin.privileged) and _same(row[:, :d], clean) and row.shape == (n, d + w), t
        assert _same(row[:, d:], ref(_np(row[:, :d]).copy(), None if t == 0 else act_np[t], T, E)), t
    A.close(), twin.close()


# ---- 5. act_step and the graph -------------------------------------------------------------------------------------------------------------
def test_act_step_files_the_policys_action_and_a_captured_rollout_replays_like_eager():
    import policy_reference as PR
    from mocca_envs_amd.policy import DevicePolicy
    from mocca_envs_amd.trainer_api import make_vec_envs
    n, w = 67, 2 * (OBS + ACT)
    p = PR.random_policy("ppo", OBS + w, ACT, norm=True, seed=4)
    dp = DevicePolicy(p.actor, p.critic, p.log_std, obs_mean=p.obs_mean, inv_std=p.inv_std, clip=p.clip)
    E_, G_ = (make_vec_envs(CUSTOM, SEED, n, None, history=History(2)) for _ in range(2))
    with pytest.raises(ValueError, match="the policy maps"):
        E_.attach_policy(DevicePolicy(*[getattr(PR.random_policy("ppo", OBS, ACT, norm=False, seed=4), k) for k in ("actor", "critic", "log_std")]))
    for e in (E_, G_):
        e.attach_policy(dp)
        e.reset()
    ref = R.History(n, 2, 1, list(range(OBS)), ACT)
    ref(_np(E_.venv.obs).copy(), None, *_counters(E_.venv))
    _near_timeout(E_.venv), _near_timeout(G_.venv)
    stor = torch.zeros(4, n, OBS + w, device="cuda")
    graph = G_.capture_rollout(num_steps=4, warmup=2, sink=lambda t, o, r, m, b, a: stor[t].copy_(o))
    own = {"action": torch.zeros(n, ACT, device="cuda")}
    for k in range(10):                        # two warm-up steps, then two replays of four
        if k >= 2 and (k - 2) % 4 == 0:
            graph.replay()
        into = own if k % 2 else None          # the action goes to the caller's row or to this object's own buffer: the history follows it
        row = E_.act_step(into=into)[0]
        torch.cuda.synchronize()
        a = E_.last_act["action"]
        assert a.data_ptr() == (own["action"] if into else E_._pol_bufs["action"]).data_ptr()
        T, Ep = _counters(E_.venv)
        assert _same(row[:, OBS:], ref(_np(row[:, :OBS]).copy(), _np(a).copy(), T, Ep)), k
        valid = _np(row[:, OBS:2 * OBS] != 0).any(1)        # envs whose newest pair is there: its action is what the policy just output
        assert valid.sum() > n // 2 and _same(row[:, 2 * OBS:2 * OBS + ACT][valid], a[valid]), k
        if k >= 2:
            assert _same(stor[(k - 2) % 4], row), k
    _outputs_agree(E_.venv, G_.venv, "after the replays")
    E_.close(), G_.close()


# ---- 6. the mirror -------------------------------------------------------------------------------------------------------------------------
def test_symmetric_policy_acts_on_history_rows_and_is_equivariant():
    """the env's extended tables (policy_mirror_tables with a history attached): act(M_o row) == M_a act(row), numerically (==), the bound
    of tests/test_gpu_policy_symmetry.py, on rows the history kernel wrote"""
    import policy_reference as PR
    import policy_symmetry_reference as S
    n, K = 17, 3
    env = _env(n)
    env.set_history(History(K))
    w = env.history_dim
    assert OBS + w == 271
    p = PR.random_policy("ppo", OBS + w, ACT, norm=True, seed=13)
    with pytest.raises(ValueError, match="it must be the full row"):
        env.policy_mirror_tables(S.device_policy(PR.random_policy("ppo", OBS, ACT, norm=True, seed=13)))
    dp = env.symmetric_policy(S.device_policy(p))
    t = dp.symmetry
    assert len(t[0]) == OBS + w
    env.set_policy(dp)
    rows = torch.zeros(n, OBS + w, device="cuda")
    env.reset()
    _, act = _actions(n, ACT, 4)
    for k in range(4):
        env.step(act[k])
        rows[:, :OBS].copy_(env.obs)
        env.history(rows, act[k], out=rows[:, OBS:])
    x = _np(rows).copy()
    assert _full(x[:, OBS:], K)
    xm = S.mirror(x, t[0], t[1])
    out = lambda r: {k: _np(v) for k, v in env.act(torch.from_numpy(r).cuda(), deterministic=True, out={"mean": torch.empty(n, ACT, device="cuda")}).items()}
    a, b = out(x), out(xm)
    assert np.all(b["mean"] == S.mirror(a["mean"], t[2], t[3])) and np.all(b["value"] == a["value"])
    assert np.abs(S.mirror(a["mean"], t[2], t[3]) - a["mean"]).max() > 1e-3
    env.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_handle_and_outputs_unchanged():
    n = 5
    A, B = _env(n), _env(n)
    for e in (A, B):
        e.set_history(_history("k2_s3_some"))
        e.reset()
        e.history(e.obs)
    lib, h, dim = A.lib, A.h, A.history_dim
    cols = lambda *c: (C.c_int32 * max(len(c), 1))(*c)
    bad = [((cols(0, 52), 2, ACT, 2, 1), "column 52 is outside"), ((cols(-1), 1, ACT, 2, 1), "column -1 is outside"), ((cols(3, 7, 3), 3, ACT, 2, 1), "column 3 is repeated"),
           ((cols(0), 1, ACT, 17, 1), "steps must be"), ((cols(0), 1, ACT, -1, 1), "steps must be"), ((cols(0), 1, ACT, 2, 0), "stride must be"),
           ((cols(0), 1, ACT, 2, 9), "stride must be"), ((cols(0), 1, 33, 2, 1), "act_dim must be"), ((cols(0), 1, -1, 2, 1), "act_dim must be"),
           ((cols(*range(52)), 52, ACT, 16, 1), "at most 1024"), ((cols(), 0, 0, 2, 1), "at least one"), ((cols(0), 53, ACT, 2, 1), "n_cols must be"),
           ((None, 2, ACT, 2, 1), "n_cols must be")]
    for args, word in bad:
        assert lib.mocca_set_history(h, *args) == -1, word
        msg = (lib.mocca_last_error(h) or b"").decode()
        assert msg.startswith("mocca_set_history:") and word in msg, (word, msg)
    assert lib.mocca_history_dim(h) == dim
    rows, act, out = (torch.full((n, x), 9.0, device="cuda") for x in (OBS, ACT, dim))
    vp = lambda t: C.c_void_p(t.data_ptr())
    s = A._stream()
    for args, word in (((None, OBS, vp(act), ACT, vp(out), dim), "NULL"), ((vp(rows), OBS, vp(act), ACT, None, dim), "NULL"),
                       ((vp(rows), OBS - 1, vp(act), ACT, vp(out), dim), "row_stride"), ((vp(rows), OBS, vp(act), ACT, vp(out), dim - 1), "out_stride"),
                       ((vp(rows), OBS, vp(act), ACT - 1, vp(out), dim), "act_stride")):
        assert lib.mocca_history(h, *args, s) == -1 and word in lib.mocca_last_error(h).decode(), word
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and lib.mocca_history_dim(h) == dim                # nothing was launched
    assert lib.mocca_history(h, vp(rows), OBS, None, 0, vp(out), dim, s) == 0          # act_stride is not read without an action ...
    torch.cuda.synchronize()
    assert _same(out, B.history(rows)) and not bool((out == 9.0).any())                # ... and a following valid call is right
    for name, t in (("rows", rows[:, :OBS - 1]), ("rows", rows.double()), ("out", out[:, :dim - 1]), ("act", act[:, :ACT - 1]), ("rows", rows[:3])):
        with pytest.raises(ValueError, match=name):
            A.history(**{"rows": rows, "act": act, "out": out, name: t})
    with pytest.raises(ValueError, match="column 52"):
        A.set_history(History(2, columns=[52]))
    # the handle is as it was: it goes on exactly like its twin, which saw none of the refused calls
    _, actions = _actions(n, ACT, 7)
    for t in range(7):
        A.step(actions[t]), B.step(actions[t])
        assert _same(A.history(A.obs, actions[t]), B.history(B.obs, actions[t])), t
        _outputs_agree(A, B, t)
    assert _full(A.history(A.obs, actions[6]), 2)
    fresh = _env(n)
    assert lib.mocca_history_dim(fresh.h) == -1 and "mocca_set_history" in lib.mocca_last_error(fresh.h).decode()
    assert lib.mocca_history(fresh.h, vp(rows), OBS, None, 0, vp(out), dim, s) == -1 and "mocca_set_history" in lib.mocca_last_error(fresh.h).decode()
    with pytest.raises(L.MoccaError, match="set_history"):
        fresh.history(rows)
    # the trainer surface refuses before a device is touched
    from mocca_envs_amd.trainer_api import make_vec_envs
    with pytest.raises(NotImplementedError, match="history with terminal_observation=True"):
        make_vec_envs(CUSTOM, SEED, n, None, history=History(2), terminal_observation=True)
    with pytest.raises(NotImplementedError, match="history needs one handle"):
        make_vec_envs(CUSTOM, SEED, n, None, history=History(2), sub_batches=2)
    for e in (A, B, fresh):
        e.close()


# ---- 8. the tools --------------------------------------------------------------------------------------------------------------------------
def test_ppo_demo_trains_with_a_history_and_the_eval_tool_plays_its_policy(tmp_path, capsys):
    """tools/ppo_demo.py --history 2 under a randomisation, imported and driven, 64 envs x 8 steps, two iterations on the device arm: the
    policy file records the history and its first layer is as wide as the row; tools/randomisation_eval.py rebuilds the env with it"""
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
                           "--history", "2", "--out", out] + flags)
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert lines and all(np.isfinite(x["mean_return"]) for x in lines)
    with np.load(out + "_policy.npz", allow_pickle=False) as z:
        assert History.from_dict(json.loads(str(z["history"]))) == History(2)
        assert z["pi_0_weight"].shape[1] == OBS + 2 * (OBS + ACT) == z["obs_mean"].shape[0]
    ev = tool("randomisation_eval")
    ev.main(["--policy", f"p={out}_policy.npz", "--envs", "8", "--max-steps", "20", "--out", out + "_eval.jsonl"])
    ev.main(["--policy", f"p={out}_policy.npz", "--envs", "8", "--max-steps", "20", "--out", out + "_eval.jsonl"] + flags)
    rows = [json.loads(x) for x in open(out + "_eval.jsonl")]
    assert [r["condition"] for r in rows] == ["plain", "randomised"] and all(r["history"] == History(2).as_dict() for r in rows)
    assert all(np.isfinite(r["mean_return"]) and 0 < r["mean_length"] <= 20 for r in rows)
    with pytest.raises(SystemExit):
        tool("ppo_demo").main(["--history", "2", "--mirror-dup", "--out", out])
