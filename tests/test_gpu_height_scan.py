"""The terrain height scan on the GPU (include/mocca.h mocca_height_scan, csrc/mocca_scan.hip): values and hit / miss against the float64
numpy reference (tests/height_scan_reference.py) away from plank silhouettes, heading invariance, auto-reset, the fused row, hipGraph
capture with step / plan_step, the error cases, the trainer surface.  Figures: profiles/height_scan_parity.json.

The bound of every value comparison is the project's render / link-frame bound: on kept points
    |kernel - float64|  <=  4 x max|float32 numpy reference - float64|  +  one float32 ulp of the largest |float64 value|.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import height_scan_reference as HS  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mocca_envs_amd import lib as L  # noqa: E402
from mocca_envs_amd.perception import scan_grid  # noqa: E402
from mocca_envs_amd.vec_env import VecEnv, task_from_float64  # noqa: E402

FIGURES = os.environ.get("MOCCA_SCAN_FIGURES")      # a path: the measured errors are appended there as JSON lines


def _record(**kw):
    print(json.dumps(kw))
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _compare(env, task_id, pts, hf, what, **tags):
    """scan of every env of `env` against the references on its get_state / get_terrain snapshots -> asserts class and bound on kept points"""
    st, ter = env.get_state().cpu().numpy(), env.get_terrain().cpu().numpy()
    env.get_task()
    got = env.height_scan().cpu().numpy()
    assert got.shape == (env.n_envs, len(pts)) and got.dtype == np.float32
    e32 = ek = big = 0.0
    kept = lost = wrong = 0
    for e in range(env.n_envs):
        if not np.isfinite(st[e, :7]).all():          # (a diverged env has no pose to scan from)
            continue
        kw = HS.scene_kwargs(env.model, task_id, ter[e], hf)
        r64, c64 = HS.scan(st[e], task_id, pts, dtype=np.float64, **kw)
        r32, _ = HS.scan(st[e], task_id, pts, dtype=np.float32, **kw)
        keep = ~HS.excluded(st[e], task_id, pts, **kw)
        kept, lost = kept + int(keep.sum()), lost + int((~keep).sum())
        wrong += int(((got[e] == np.float32(-HS.MAX_DROP)) != (c64 == HS.CLS_NONE))[keep].sum())
        if keep.any():
            e32 = max(e32, float(np.abs(r32.astype(np.float64) - r64)[keep].max()))
            ek = max(ek, float(np.abs(got[e].astype(np.float64) - r64)[keep].max()))
            big = max(big, float(np.abs(r64[keep]).max()))
    ulp = float(np.spacing(np.float32(big)))
    _record(test=what, compared=kept, excluded=lost, class_mismatches=wrong, numpy_f32_err=e32, kernel_err=ek, ulp_floor=ulp, **tags)
    assert kept > 0
    assert wrong == 0, (what, tags, wrong)
    assert ek <= 4 * e32 + ulp, (what, tags, ek, e32, ulp)
    return got


def _gpu_scene(name, auto_reset=True):
    model, task_id, kw, st, tk, ter, hf = HS.scene_records(name)
    env = VecEnv(HS.SCENES[name][0], HS.RR.SCENE_ENVS, device=0, auto_reset=auto_reset, seed=HS.RR.SCENE_SEED, **kw)
    env.reset()
    env.set_state(st)
    env.set_task(task_from_float64(tk))
    t128 = np.zeros((HS.RR.SCENE_ENVS, 128), np.float32)
    t128[:, :ter.shape[1]] = ter
    env.set_terrain(t128)
    return env, task_id, hf


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HS.SCENES))
def test_scan_matches_the_reference(name):
    """Every scene of render_reference.SCENES, at the scene state and after 1, 10 and 100 random steps (auto-reset on, so the robots stay
    on their terrain).  Kept points: the float64 class does not change 1 mm away (height_scan_reference.excluded)."""
    env, task_id, hf = _gpu_scene(name)
    pts = HS.comparison_grid(name)
    env.set_height_scan(pts, HS.Z_ABOVE, HS.MAX_DROP)
    assert env.scan_dim == len(pts) == 77
    g = torch.Generator().manual_seed(11)
    done_steps = 0
    for upto in (0, 1, 10, 100):
        while done_steps < upto:
            env.step((torch.rand(env.n_envs, env.act_dim, generator=g) * 2 - 1).to(env.device))
            done_steps += 1
        _compare(env, task_id, pts, hf, "parity", scene=name, steps=upto)
    env.close()


# ---- heading -------------------------------------------------------------------------------------------------------------------------
def _quat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]   # xyzw


def _bound(st_row, task_id, pts, hf):
    r64, _ = HS.scan(st_row, task_id, pts, hf=hf)
    r32, _ = HS.scan(st_row, task_id, pts, hf=hf, dtype=np.float32)
    return r64, 4 * float(np.abs(r32 - r64).max()) + float(np.spacing(np.float32(np.abs(r64).max())))


def test_heading_frame_on_the_height_field():
    """Two envs at one position with different yaw, scanned with correspondingly rotated patterns, see the same world points: equal values
    (within the bound of each against the float64 reference).  Rolling and pitching the base changes nothing: only base_z enters."""
    env = VecEnv("Walker3DPlannerEnv-v0", 3, device=0, auto_reset=False, seed=1)
    env.reset()
    hf = env.height_field
    st = env.get_state().cpu().numpy()
    pos, ya, yb = np.array([1.7, -2.3, 1.1], np.float32), 0.6, -1.9
    st[:, 0:3] = pos
    st[0, 3:7], st[1, 3:7], st[2, 3:7] = _quat(0, 0, ya), _quat(0, 0, yb), _quat(0.3, -0.25, ya)
    env.set_state(st)
    st = env.get_state().cpu().numpy()
    pa = HS.comparison_grid()
    c, s = np.cos(ya - yb), np.sin(ya - yb)
    pb = (pa.astype(np.float64) @ np.array([[c, s], [-s, c]])).astype(np.float32)     # R_z(ya - yb) pa: R_z(yb) pb = R_z(ya) pa
    env.set_height_scan(pa)
    va = env.height_scan().cpu().numpy().astype(np.float64)
    env.set_height_scan(pb)
    vb = env.height_scan().cpu().numpy().astype(np.float64)
    ra, ba = _bound(st[0], HS.TASK_PLANNER, pa, hf)
    rb, bb = _bound(st[1], HS.TASK_PLANNER, pb, hf)
    rt, bt = _bound(st[2], HS.TASK_PLANNER, pa, hf)
    _record(test="heading", yaw_pair_diff=float(np.abs(va[0] - vb[1]).max()), tilt_diff=float(np.abs(va[0] - va[2]).max()), bound_a=ba, bound_b=bb, bound_tilted=bt,
            reference_pair_diff=float(np.abs(ra - rb).max()), reference_tilt_diff=float(np.abs(ra - rt).max()))
    assert np.ptp(ra) > 0.05                                        # (the patch of terrain is not flat: the comparison says something)
    assert np.abs(va[0] - ra).max() <= ba and np.abs(vb[1] - rb).max() <= bb and np.abs(va[2] - rt).max() <= bt
    assert np.abs(va[0] - vb[1]).max() <= ba + bb + np.abs(ra - rb).max()
    assert np.abs(va[0] - va[2]).max() <= ba + bt + np.abs(ra - rt).max()
    assert np.abs(ra - rb).max() < 1e-5 and np.abs(ra - rt).max() < 1e-5      # the references agree that nothing should change
    env.close()


# ---- auto-reset, records -------------------------------------------------------------------------------------------------------------
def test_scan_after_an_auto_reset_step_is_of_the_new_episode():
    n = 64
    env = VecEnv("Walker3DStepperEnv-v0", n, device=0, auto_reset=True, seed=3)
    env.reset()
    pts = HS.comparison_grid()
    env.set_height_scan(pts)
    g = torch.Generator().manual_seed(2)
    for _ in range(400):
        _, _, done, _ = env.step((torch.rand(n, env.act_dim, generator=g) * 2 - 1).to(env.device))
        if bool(done.any()):
            break
    fin = done.cpu().numpy() != 0
    assert fin.any(), "no episode ended in 400 random steps"
    got = _compare(env, HS.TASK_STEPPER, pts, None, "auto_reset", finished=int(fin.sum()))
    st, ter = env.get_state().cpu().numpy(), env.get_terrain().cpu().numpy()
    for e in np.nonzero(fin)[0][:8]:              # ... and for the envs that finished it is the scan of the state after the reset
        kw = HS.scene_kwargs(env.model, HS.TASK_STEPPER, ter[e], None)
        r64, _ = HS.scan(st[e], HS.TASK_STEPPER, pts, **kw)
        keep = ~HS.excluded(st[e], HS.TASK_STEPPER, pts, **kw)
        assert np.abs(got[e] - r64)[keep].max() < 1e-4
    env.close()


@pytest.mark.parametrize("env_id", ["Walker3DStepperEnv-v0", "MikePlannerEnv-v0", "CassieEnv-v0"])
def test_scan_writes_none_of_the_records(env_id):
    env = VecEnv(env_id, 64, device=0, auto_reset=True, seed=9)
    env.reset()
    env.set_height_scan(HS.comparison_grid())
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        env.step((torch.rand(64, env.act_dim, generator=g) * 2 - 1).to(env.device))
    before = [x.cpu().numpy().tobytes() for x in (env.get_state(), env.get_task(), env.get_terrain(), env.obs)]
    env.height_scan()
    env.height_scan(obs=env.obs)
    after = [x.cpu().numpy().tobytes() for x in (env.get_state(), env.get_task(), env.get_terrain(), env.obs)]
    assert before == after
    env.close()


# ---- the fused row -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,n_pts", [("Walker3DStepperEnv-v0", 77), ("Walker3DPlannerEnv-v0", 256), ("Walker3DCustomEnv-v0", 1)])
def test_fused_row_is_observation_then_scan(env_id, n_pts):
    n = 200
    env = VecEnv(env_id, n, device=0, auto_reset=True, seed=5)
    env.reset()
    rng = np.random.default_rng(0)
    env.set_height_scan(rng.uniform(-1.5, 1.5, (n_pts, 2)).astype(np.float32), 0.8, 1.5)
    obs = env.step(torch.zeros(n, env.act_dim, device=env.device))[0]
    alone = env.height_scan()
    assert alone.shape == (n, n_pts)
    pad, sentinel = 5, 12345.0
    store = torch.full((n, env.obs_dim + n_pts + pad), sentinel, device=env.device)
    wide = env.height_scan(out=store, obs=obs)
    torch.cuda.synchronize()
    assert wide.shape == (n, env.obs_dim + n_pts) and wide.data_ptr() == store.data_ptr()
    assert torch.equal(store[:, :env.obs_dim], obs)                                 # bit-equal to the step's observation
    assert torch.equal(store[:, env.obs_dim:env.obs_dim + n_pts], alone)            # bit-equal to the standalone scan
    assert bool((store[:, env.obs_dim + n_pts:] == sentinel).all())                 # the stride padding survives
    narrow = torch.full((n, n_pts + pad), sentinel, device=env.device)
    env.height_scan(out=narrow)
    assert torch.equal(narrow[:, :n_pts], alone) and bool((narrow[:, n_pts:] == sentinel).all())
    assert float(alone.min()) >= -1.5 and float(alone.max()) <= 0.8                 # the clamp
    env.close()


# ---- hipGraph ------------------------------------------------------------------------------------------------------------------------
def _graph_vs_eager(make, stepper, width, steps=20):
    A, B = make(), make()
    A.reset(); B.reset()
    pts = HS.comparison_grid()
    A.set_height_scan(pts); B.set_height_scan(pts)
    n = A.n_envs
    g = torch.Generator(device="cuda").manual_seed(4)
    acts = torch.rand(steps + 2, n, width, device="cuda", generator=g) * 2 - 1
    rows = torch.zeros(steps, n, A.obs_dim + len(pts), device="cuda")
    tmp = torch.zeros(n, A.obs_dim + len(pts), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(2):
            for e in (A, B):
                e.height_scan(out=tmp, obs=stepper(e)(acts[steps + t])[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for t in range(steps):
            A.height_scan(out=rows[t], obs=stepper(A)(acts[t])[0])
    graph.replay()
    torch.cuda.synchronize()
    for t in range(steps):
        eager = B.height_scan(obs=stepper(B)(acts[t])[0])
        assert torch.equal(eager, rows[t]), t
    assert torch.equal(A.get_state(), B.get_state()) and torch.equal(A.get_task(), B.get_task()) and torch.equal(A.get_terrain(), B.get_terrain())
    A.close(); B.close()


def test_step_and_scan_replay_from_one_graph():
    _graph_vs_eager(lambda: VecEnv("Walker3DStepperEnv-v0", 512, device=0, auto_reset=True, seed=6), lambda e: e.step, 21)


def test_plan_step_and_scan_replay_from_one_graph():
    import controller_reference as R
    ctrl = R.random_controller("small", seed=3)
    _graph_vs_eager(lambda: VecEnv("MikePlannerEnv-v0", 512, device=0, auto_reset=True, seed=6, base_controller=ctrl), lambda e: e.plan_step, 15)


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_messages():
    env = VecEnv("Walker3DStepperEnv-v0", 8, device=0, auto_reset=False)
    env.reset()
    lib, h = env.lib, env.h
    out = torch.zeros(8, 400, device=env.device)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    stream = env._stream()

    def refused(rc):
        assert rc == -1 and lib.mocca_last_error(h).decode().strip() != ""      # MOCCA_E_ARG, with a message

    assert lib.mocca_scan_dim(h) == 0
    refused(lib.mocca_height_scan(h, C.c_void_p(out.data_ptr()), 400, None, stream))          # before mocca_set_height_scan
    with pytest.raises(L.MoccaError):
        env.height_scan()
    good = np.zeros((4, 2), np.float32)
    refused(lib.mocca_set_height_scan(h, ptr(good), 0, 1.0, 2.0))                              # n_points outside 1 .. 256
    refused(lib.mocca_set_height_scan(h, ptr(np.zeros((257, 2), np.float32)), 257, 1.0, 2.0))
    for bad in (np.nan, np.inf):
        pts = good.copy(); pts[2, 1] = bad
        refused(lib.mocca_set_height_scan(h, ptr(pts), 4, 1.0, 2.0))                           # non-finite points
    refused(lib.mocca_set_height_scan(h, ptr(good), 4, -0.1, 2.0))                             # z_above < 0
    refused(lib.mocca_set_height_scan(h, ptr(good), 4, 1.0, 0.0))                              # max_drop <= 0
    refused(lib.mocca_set_height_scan(h, ptr(good), 4, 1.0, -1.0))
    assert lib.mocca_scan_dim(h) == 0                                                          # a refused call attaches nothing
    assert lib.mocca_set_height_scan(h, ptr(good), 4, 0.0, 2.0) == 0 and lib.mocca_scan_dim(h) == 4
    refused(lib.mocca_height_scan(h, C.c_void_p(out.data_ptr()), 3, None, stream))             # row_stride too small
    refused(lib.mocca_height_scan(h, C.c_void_p(out.data_ptr()), env.obs_dim + 3, C.c_void_p(env.obs.data_ptr()), stream))
    refused(lib.mocca_height_scan(h, None, 400, None, stream))
    assert lib.mocca_height_scan(h, C.c_void_p(out.data_ptr()), 4, None, stream) == 0
    with pytest.raises(ValueError):
        env.height_scan(out=torch.zeros(8, 3, device=env.device))
    with pytest.raises(ValueError):
        env.set_height_scan(np.zeros((4, 3), np.float32))
    env.set_height_scan(None)                                                                  # detaches
    assert env.scan_dim == 0
    env.close()
    # a planner handle before mocca_set_heightfield
    from mocca_envs_amd import model as M
    blob = M.compile_walker3d(M.TASK_WALKER3D_PLANNER).to_bytes()
    buf, hp = C.create_string_buffer(blob, len(blob)), C.c_void_p()
    assert lib.mocca_create(buf, len(blob), M.TASK_WALKER3D_PLANNER, 8, 0, C.byref(hp)) == 0
    assert lib.mocca_set_height_scan(hp, ptr(good), 4, 1.0, 2.0) == 0
    rc = lib.mocca_height_scan(hp, C.c_void_p(out.data_ptr()), 4, None, stream)
    assert rc == -1 and b"heightfield" in lib.mocca_last_error(hp)
    torch.cuda.synchronize()
    lib.mocca_destroy(hp)


# ---- the trainer surface -------------------------------------------------------------------------------------------------------------
def test_trainer_surface_returns_and_fills_wide_rows():
    from mocca_envs_amd.trainer_api import TorchVecEnv, make_vec_envs
    n, T = 256, 6
    pts = scan_grid((-0.45, 1.05), (-0.45, 0.45), 11, 7)
    hs = dict(points=pts, z_above=1.0, max_drop=2.0)
    envs = make_vec_envs("Walker3DStepperEnv-v0", 7, n, None, height_scan=hs)
    twin = VecEnv("Walker3DStepperEnv-v0", n, device=0, auto_reset=True, seed=7)
    twin.set_height_scan(**hs)
    d, P = twin.obs_dim, 77
    assert envs.observation_space.shape == (d + P,) and envs.venv.scan_dim == P
    o, to = envs.reset(), twin.reset()
    assert o.shape == (n, d + P) and torch.equal(o[:, :d], to) and torch.equal(o[:, d:], twin.height_scan())
    g = torch.Generator(device="cuda").manual_seed(8)
    acts = torch.rand(3 * T, n, 21, device="cuda", generator=g) * 2 - 1
    for t in range(T):                                              # step(): VecEnv and TorchVecEnv agree
        o, r, done, infos = envs.step(acts[t])
        to, tr = twin.step(acts[t])[:2]
        assert o.shape == (n, d + P) and r.shape == (n, 1)
        assert torch.equal(o[:, :d], to) and torch.equal(o[:, d:], twin.height_scan()) and torch.equal(r[:, 0], tr)
    store = torch.zeros(T + 1, n, d + P, device="cuda")            # step(into=...): the wide row lands in the trainer's storage
    for t in range(T):
        o, _, _, _ = envs.step(acts[T + t], into={"obs": store[t + 1]})
        to = twin.step(acts[T + t])[0]
        assert o.data_ptr() == store[t + 1].data_ptr()
        assert torch.equal(store[t + 1][:, :d], to) and torch.equal(store[t + 1][:, d:], twin.height_scan())
    with pytest.raises(ValueError):
        envs.step(acts[0], into={"obs": torch.zeros(n, d, device="cuda")})
    envs.step(acts[2 * T]); twin.step(acts[2 * T])                 # (a plain step: the env's own wide buffer is current again)
    # capture_rollout: policy sees the wide row, sink receives it
    W = torch.randn(d + P, 21, device="cuda", generator=g) * 0.1
    policy = lambda ob: torch.tanh(ob @ W)
    policy(envs.step(acts[2 * T + 1])[0]); twin.step(acts[2 * T + 1])   # (the matrix product's first call sets its library up: not inside a capture)
    torch.cuda.synchronize()
    rolled = torch.zeros(T, n, d + P, device="cuda")
    graph = envs.capture_rollout(policy, T, sink=lambda t, ob, rw, m, bm, a: rolled[t].copy_(ob), warmup=0)
    graph.replay()
    torch.cuda.synchronize()
    ob = torch.cat([twin.obs, twin.height_scan()], dim=1)
    for t in range(T):
        to = twin.step(policy(ob))[0]
        ob = torch.cat([to, twin.height_scan()], dim=1)
        assert torch.equal(rolled[t], ob), t
    envs.close(); twin.close()
    with pytest.raises(NotImplementedError):
        TorchVecEnv("Walker3DStepperEnv-v0", 8, terminal_observation=True, height_scan=hs)
    with pytest.raises(NotImplementedError):
        TorchVecEnv("Walker3DStepperEnv-v0", 8, sub_batches=2, height_scan=hs)


def test_gym_class_height_scan():
    import mocca_envs_amd
    env = mocca_envs_amd.make("Walker3DCustomEnv-v0").unwrapped
    env.seed(0)
    env.reset()
    v = env.height_scan()
    assert v.shape == (77,) and v.dtype == np.float32 and np.allclose(v, -env.robot.body_xyz[2], atol=1e-6)
    v = env.height_scan(points=[[0.0, 0.0], [0.5, 0.0]], z_above=0.5, max_drop=0.25)
    assert v.tolist() == [-0.25, -0.25]                            # the ground lies further below the base than max_drop
    env.close()


# ---- rotated planks, the hills, the border, outside the grid: synthetic scenes (height_scan_reference.synthetic_scan_records) ---------
def _synthetic_cases():
    return [(n, c) for n in HS.PLANK_SCENES for c in HS.PLANK_CASES] + [("planner", c) for c in HS.PLANNER_CASES]


@pytest.mark.parametrize("name,case", _synthetic_cases())
def test_synthetic_scenes_match_the_reference(name, case):
    """Every synthetic scene and pattern under the rule of this file (class equal and 4 x e32 + 1 ulp on kept points, per env); then, on
    the comparison grid, the kernel's values must FAIL that rule against each mutated reference."""
    model, task_id, kw, st, tk, ter, hf = HS.synthetic_scan_records(name, case)
    _, za, md = (HS.PLANNER_CASES if name == "planner" else HS.PLANK_CASES)[case]
    pts = HS.synthetic_pattern(name, case)
    env_id = HS.RR.PLANNER_ENV if name == "planner" else HS.PLANK_SCENES[name][0]
    env = VecEnv(env_id, st.shape[0], device=0, auto_reset=False, **kw)
    env.reset()
    env.set_state(st)
    env.set_task(task_from_float64(tk))
    env.set_terrain(ter.astype(np.float32))
    env.set_height_scan(pts, za, md)
    assert env.scan_dim == len(pts)
    got = env.height_scan().cpu().numpy()
    st_dev = env.get_state().cpu().numpy()
    assert st_dev.tobytes() == st.tobytes()
    total = dict(compared=0, excluded=0, class_mismatches=0, numpy_f32_err=0.0, kernel_err=0.0, ulp_floor=0.0)
    sat = 0
    for e in range(st.shape[0]):
        skw = HS.scene_kwargs(model, task_id, ter[e].astype(np.float32), hf)
        ok, fig = HS.accepts(got[e], st[e], task_id, pts, za, md, **skw)
        for k in ("compared", "excluded", "class_mismatches"):
            total[k] += fig[k]
        for k in ("numpy_f32_err", "kernel_err", "ulp_floor"):
            total[k] = max(total[k], fig[k])
        sat += int((got[e] == np.float32(za)).sum())
        assert ok, (name, case, e, fig)
    _record(test="synthetic", scene=name, case=case, points=len(pts), z_above=za, max_drop=md, saturated=sat, **total)
    assert total["excluded"] <= HS.MAX_EXCLUDED * got.size
    if case in ("inside", "short_drop"):
        assert sat > 0
    if case == "grid":      # negative controls: every env that sees terrain must reject every wrong reference
        for mut in HS.RR.HF_MUTATIONS if name == "planner" else HS.RR.PLANK_MUTATIONS:
            for e in range(st.shape[0]):
                skw = HS.scene_kwargs(model, task_id, ter[e].astype(np.float32), hf)
                if not HS.sees_terrain(st[e], task_id, pts, za, md, **skw):
                    continue
                bad, fig = HS.accepts(got[e], st[e], task_id, pts, za, md, mutate=mut, **skw)
                _record(test="negative_control", scene=name, env=e, mutation=mut, accepted=bool(bad), **fig)
                assert not bad, (name, mut, e, fig)
    env.close()
