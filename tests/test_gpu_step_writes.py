"""Everything the step kernel writes, held to the oracle -- not only what env.step() returns.

The strict parity tests (test_gpu_parity.py, test_gpu_substep.py) force the task record and the Stepper's terrain record from the oracle before
every step and never read them back afterwards, run with auto_reset=False, and attach the debug buffer.  Here:

A. teacher-forced steps (state / task / terrain forced from the f32 oracle, f64 oracle beside it as the yardstick) of the PRODUCT configuration
   (no debug buffer, no persisted impulses, in-step auto-reset, the in-kernel Monitor attached), after which the task record (word by word, in
   the classes of task_word_classes()), the Stepper terrain record, the new episode an in-step reset starts and the Monitor's episode records are
   compared with the oracle's.  The sample is built so that it holds TimeLimit truncations, terminations, plank advances (Stepper) and
   re-targets (Custom), and the test asserts that it does;
B. the debug buffer and the other diagnostic attachments change no bit of anything a step writes.

Needs a real MI355X: -m gpu."""
import numpy as np
import pytest

from mocca_envs_amd import model as M

pytestmark = pytest.mark.gpu

TW = M.TW   # task record words (include/mocca_model.h MoccaTaskWord)

# How each task word is compared after a step:
#   "exact"   -- must be equal in every env whose done flags agree (counters, flags, draw-derived integers)
#   "contact" -- discrete words that follow the contact decisions of the step: equal wherever the step took the oracle's decisions in every
#                substep (MOCCA_DBG_STEPSIG); elsewhere a flipped contact flips them, exactly as it does between the f32 and f64 oracles
#   "draw"    -- floats drawn at reset / re-target or copied: within the task atol of test_gpu_parity.test_reset_matches_oracle (1e-4)
#   "cont"    -- continuous floats of the step: error units of test_gpu_parity (1e-3 + 1e-3 |x|), held to the f32-vs-f64 oracle yardstick
#   "skip"    -- kernel-private, not part of the oracle's record (the reason is given)
_COMMON = {TW.WALK_TARGET_X: "draw", TW.WALK_TARGET_Y: "draw", TW.WALK_TARGET_Z: "draw", TW.LINEAR_POTENTIAL: "cont",
           TW.ANGULAR_POTENTIAL: "cont", TW.CLOSE_COUNT: "contact", TW.STOP_FRAMES: "draw", TW.DONE: "contact", TW.T: "exact",
           TW.EPISODE: "exact", TW.DRAW: "exact", TW.MIRRORED: "exact", TW.FEET_CONTACT_0: "contact", TW.FEET_CONTACT_1: "contact",
           TW.DIST: "draw", TW.ANGLE: "draw", TW.NEXT_STEP_INDEX: "contact", TW.TARGET_REACHED_COUNT: "contact",
           TW.STOP_ON_NEXT_STEP: "contact", TW.SET_STOP_ON_NEXT_STEP: "contact", TW.CURRICULUM: "exact", TW.APPLIED_GAIN: "draw",
           TW.PREV_BODY_X: "cont", TW.LAST_ROWS: "skip"}
SKIP_REASONS = {TW.LAST_ROWS: "constraint rows of the last substep: the kernel's launch-priority hint for the next step (timing only)"}


def task_word_classes(task: int, n_feet: int) -> dict:
    cls = dict(_COMMON)
    if task == M.TASK_CASSIE:
        for w in range(TW.JVEL, TW.JVEL + 14):
            cls[w] = "cont"                                           # jvel[14]: filtered joint speeds (env_cassie.py:451-468)
        cls[TW.INITIAL_Z], cls[TW.ISTEP] = "cont", "exact"
        return cls
    for w in range(TW.FEET_CONTACT_2, M.TASK_WORDS):
        cls[w] = "exact"                                              # unused words: must come back as they were forced
    if n_feet == 4:
        cls[TW.FEET_CONTACT_2], cls[TW.FEET_CONTACT_3] = "contact", "contact"
    if task == M.TASK_WALKER3D_STEPPER:
        cls[TW.COVER] = "contact"                                     # cover mask of the last substep's contacts
        for k in range(8):
            cls[TW.REWARD_WEIGHTS + k] = "draw"                       # this episode's eight random-reward weights
    return cls


def _err_units(a, b):
    return np.abs(a - b) / (1e-3 + 1e-3 * np.abs(b))                  # test_gpu_parity.ERR_ABS / ERR_REL


RESET_ATOL = dict(obs=2e-6, state=2e-6, task=1e-4, terrain=5e-6)      # test_gpu_parity.test_reset_matches_oracle
TASK_RTOL = 2.0 ** -22      # + 2 fp32 ulps of the value: the planner's potentials (-dist / dt) reach 1e3, where 1e-4 is below one ulp


def _task_close(g, c):
    return np.abs(g - c) <= RESET_ATOL["task"] + TASK_RTOL * np.abs(c)


def _setup(env_id, task, n, seed, kw, oracle_model_edit=None, random_reward=False):
    import torch
    from mocca_envs_amd import lib as L
    from mocca_envs_amd.vec_env import VecEnv, _DEFAULT_PARAMS
    from oracle.oracle import Oracle, PARAM_AUTO_RESET, PARAM_CURRICULUM, PARAM_RANDOM_REWARD
    env = VecEnv(env_id, n, auto_reset=True, seed=seed, **kw)         # the product configuration: no debug buffer, no persisted impulses
    twin = VecEnv(env_id, n, auto_reset=True, seed=seed, **kw)        # ... and a twin with the debug buffer, for the decision signature only
    dbg = twin.set_debug(True)
    ep = env.episode_stats(True, slots=2)
    blob = env.model.to_bytes()
    oblob = blob
    if oracle_model_edit is not None:
        m = M.MoccaModel.from_bytes(blob)
        oracle_model_edit(m)
        oblob = m.to_bytes()
    o32, o64 = Oracle(oblob, task, n, "f32"), Oracle(oblob, task, n, "f64")
    for o in (o32, o64):
        o.set_param(PARAM_AUTO_RESET, 1)
        for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
            o.set_param(pid, val)
        if task == M.TASK_WALKER3D_STEPPER:
            o.set_param(PARAM_CURRICULUM, 9)
        if random_reward:
            o.set_param(PARAM_RANDOM_REWARD, 1)
        if env.trajectory is not None:
            o.set_trajectory(env.trajectory.table(), env.trajectory.max_time(), 0.03)
    for e in (env, twin):
        if task == M.TASK_WALKER3D_STEPPER:
            e.set_param(L.PARAM_CURRICULUM, 9)
        if random_reward:
            e.set_param(L.PARAM_RANDOM_REWARD, 1)
    field = None
    if task == M.TASK_WALKER3D_PLANNER:
        from mocca_envs_amd import host_logic as H
        field = H.random_height_field(np.random.RandomState(5), (64, 64), 2).reshape(64, 64).astype(np.float32)
        for x in (env, twin, o32, o64):
            x.set_heightfield(field, 2)
    env.reset(); twin.reset(); o32.reset(seed=seed); o64.reset(seed=seed)
    return env, twin, dbg, ep, o32, o64, field


def _force(env, o32, task):
    from mocca_envs_amd.vec_env import task_from_float64
    env.set_state(o32.get_state().astype(np.float32))
    env.set_task(task_from_float64(o32.get_task()))
    if task == M.TASK_WALKER3D_STEPPER:
        ter = np.zeros((env.n_envs, 128), np.float32)
        ter[:, :124] = o32.get_terrain()
        env.set_terrain(ter)


def _build_sample(t, env, o32, task, rng, field, n_planks, start):
    """Edit the oracle's state / task before step t so that the sample holds what is being checked (the HIP side is forced from it).
    `start`: {"state", "terrain"} right after the first reset."""
    n = env.n_envs
    st, tk = o32.get_state(), o32.get_task()
    mx = int(env.model.max_episode_steps)
    if t == 0:
        tk[0::3, TW.T] = mx - 3                                    # a third of the envs reach the TimeLimit within 3 steps (test_gpu_edge_cases.py:245)
        if field is not None:                                     # planner: robots scattered over the random field (test_gpu_edge_cases.py:340-344)
            for e in range(n):
                xy = rng.uniform(-13, 13, 2)
                st[e, 0:2], st[e, 2] = xy, o32.height_at(*xy) + 1.34
        if env.model.task_flags & M.TASKF_QUADRUPED_STEPPER:       # LaikagoStepperEnv: done = t > 240 and nsi <= 4 (env_locomotion.py:957-958)
            tk[0::3, TW.NEXT_STEP_INDEX] = 5                                   # ... which would end the TimeLimit third first
            tk[1::6, TW.T], tk[1::6, TW.NEXT_STEP_INDEX] = 240, 3               # ... fires
            tk[2::6, TW.T], tk[2::6, TW.NEXT_STEP_INDEX] = 240, 5               # ... does not
    if t in (0, 12) and task == M.TASK_WALKER3D_STEPPER:
        # plank advances: robots moved onto the target plank's cover (same offset from the plank centre as their reset pose had from the first
        # plank, test_stepper_standing_on_planks) with target_reached_count = 1, so that a foot on it advances next_step_index (trc >= 2);
        # next_step_index = n_planks - 1 also makes the advance rewrite the oldest plank's row (terrain words 120..123)
        ter = o32.get_terrain()
        sel = np.arange(1 + t % 3, n, 3)
        for j, e in enumerate(sel):
            nsi = 1 if j % 2 else n_planks - 1
            st[e] = start["state"][e]
            st[e, 0:3] += ter[e, 6 * nsi:6 * nsi + 3] - start["terrain"][e, 0:3]
            tk[e, TW.NEXT_STEP_INDEX], tk[e, TW.TARGET_REACHED_COUNT], tk[e, TW.STOP_ON_NEXT_STEP], tk[e, TW.SET_STOP_ON_NEXT_STEP] = nsi, 1, 0, 0
            tk[e, TW.T] = min(tk[e, TW.T], mx - 10)
    if t in (0, 12) and task == M.TASK_WALKER3D_CUSTOM:
        # re-targets: the target put 5 cm from the robot with close_count = stop_frames - 1, so randomize_target runs inside the step
        sel = np.arange(2 + t % 3, n, 3)
        tk[sel, TW.WALK_TARGET_X] = st[sel, 0] + 0.05
        tk[sel, TW.WALK_TARGET_Y] = st[sel, 1]
        tk[sel, TW.CLOSE_COUNT] = np.maximum(np.ceil(tk[sel, TW.STOP_FRAMES]) - 1, 0)
    o32.set_state(st)
    o32.set_task(tk)


def run_step_writes(env_id, task, n, steps, seed=9, kw=None, oracle_model_edit=None, corrupt=None, random_reward=False, act_scale=1.0):
    """Part A.  Returns (failures, summary): a list of messages (empty: every check held) and the counts / errors to print."""
    import torch
    from mocca_envs_amd.vec_env import task_to_float64
    kw = kw or {}
    env, twin, dbg, ep, o32, o64, field = _setup(env_id, task, n, seed, kw, oracle_model_edit, random_reward)
    cls = task_word_classes(task, int(env.model.n_feet))
    words = {c: [w for w, k in cls.items() if k == c] for c in ("exact", "contact", "draw", "cont")}
    nd = 13 + 2 * int(env.model.n_joints)
    n_planks = int(env.model.n_planks) if task == M.TASK_WALKER3D_STEPPER else 0
    stepper = task == M.TASK_WALKER3D_STEPPER
    rng = np.random.default_rng(1)
    fails = []
    S = dict(resets=0, timelimits=0, terminations=0, advances=0, ring_writes=0, retargets=0, done_mismatch=0, samples=0, episodes=0,
             contact_flips=0, contact_flips_ref=0)
    cont_g, cont_c, cont_same, cont_ref_same = [], [], [], []
    ret64 = np.zeros(n)                   # f64 sums of the ORACLE's rewards since each env's episode began
    # ... and of the per-step reward tolerance: test_gpu_parity's 5e-2 (its p99 bound on |HIP - f32 oracle|) + 3 x the f32 oracle's own
    # error against the f64 oracle on that step (a flipped contact moves the potential difference x 60 by more, for the f32 oracle too)
    tol_r = np.zeros(n)
    first_serial = ep["first_serial"]
    thr = env.model.termination_height if task != M.TASK_WALKER3D_STEPPER else env.model.term_height_cur[1]

    def fail(msg):
        if len(fails) < 20:
            fails.append(msg)

    start = dict(state=o32.get_state(), terrain=o32.get_terrain() if stepper else None)
    for t in range(steps):
        _build_sample(t, env, o32, task, rng, field, n_planks, start)
        o64.set_state(o32.get_state()); o64.set_task(o32.get_task())
        if stepper:
            o64.set_terrain(o32.get_terrain())
        _force(env, o32, task)
        _force(twin, o32, task)
        tk0, ter0 = o32.get_task(), (o32.get_terrain() if stepper else None)
        a = (act_scale * (1.0 if t % 4 else 0.3) * rng.uniform(-1, 1, (n, env.act_dim))).astype(np.float32)
        at = torch.from_numpy(a).cuda()
        og, rg, dg, ig = (x.cpu().numpy() for x in env.step(at))
        twin.step(at)
        oc, rc, dc, ic = o32.step(a)
        o6, r6, d6, _ = o64.step(a)
        torch.cuda.synchronize()
        sg, sc, s6 = env.get_state().cpu().numpy(), o32.get_state(), o64.get_state()
        tg_raw = env.get_task()
        if corrupt is not None:
            tg_raw = corrupt(t, tg_raw)
        tg, tc, t6 = task_to_float64(tg_raw), o32.get_task(), o64.get_task()
        sig_g, sig_c, sig_6 = dbg.cpu().numpy()[:, 16:19], o32.get_debug()[:, 16:19], o64.get_debug()[:, 16:19]
        same = (sig_g == sig_c).all(axis=1)
        same_ref = (sig_6 == sig_c).all(axis=1)
        ok = np.isfinite(sc).all(axis=1)
        S["samples"] += int(ok.sum())
        # done flags: equal, except where the height sits on the threshold (test_gpu_parity.test_teacher_forced_steps)
        mism = (dg != dc) & ok
        if mism.any():
            S["done_mismatch"] += int(mism.sum())
            if ((dg[mism] & 2) != (dc[mism] & 2)).any():           # the step counter is forced: the TimeLimit bit is exact
                fail(f"t={t}: TimeLimit bits differ: envs {np.nonzero(mism & ((dg & 2) != (dc & 2)))[0][:8].tolist()}")
            h = np.where(dg == 0, og[:, 0], oc[:, 0])[mism]         # relative height of the side that did NOT reset (obs word 0)
            if task != M.TASK_CASSIE and not (np.abs(h - thr) < 1e-3).all():
                fail(f"t={t}: done flags differ away from the height threshold: envs {np.nonzero(mism)[0][:8].tolist()}")
        agree = ok & ~mism
        run = agree & (dc == 0)
        fin = agree & (dc != 0)
        S["resets"] += int(fin.sum()); S["timelimits"] += int((fin & ((dc & 2) != 0)).sum()); S["terminations"] += int((fin & ((dc & 1) != 0)).sum())
        # ---- running envs: the task record, class by class
        run6 = run & (d6 == 0)              # ... and those the f64 oracle also went on with (the yardstick's samples)
        for w in words["exact"]:
            bad = run & (tg[:, w] != tc[:, w])
            if bad.any():
                fail(f"t={t}: exact task word {w} differs in envs {np.nonzero(bad)[0][:8].tolist()}: {tg[bad, w][:4]} vs {tc[bad, w][:4]}")
        for w in words["contact"]:
            bad = run & (tg[:, w] != tc[:, w])
            S["contact_flips"] += int(bad.sum()); S["contact_flips_ref"] += int((run6 & (t6[:, w] != tc[:, w])).sum())
            if (bad & same).any():
                e = np.nonzero(bad & same)[0]
                fail(f"t={t}: task word {w} differs where every substep took the oracle's decisions, envs {e[:8].tolist()}: {tg[e, w][:4]} vs {tc[e, w][:4]}")
        for w in words["draw"]:
            bad = run & ~_task_close(tg[:, w], tc[:, w])
            if bad.any():
                fail(f"t={t}: draw-derived task word {w} differs in envs {np.nonzero(bad)[0][:8].tolist()}: {tg[bad, w][:4]} vs {tc[bad, w][:4]}")
        if words["cont"]:
            cw = words["cont"]
            eg = _err_units(tg[run6][:, cw], t6[run6][:, cw]).max(axis=1)
            ec = _err_units(tc[run6][:, cw], t6[run6][:, cw]).max(axis=1)
            cont_g.append(eg); cont_c.append(ec)
            cont_same.append(_err_units(tg[run & same][:, cw], tc[run & same][:, cw]).max(axis=1) if (run & same).any() else np.zeros(0))
            cont_ref_same.append(ec[same_ref[run6]])
        if stepper:
            tgr, tcr = env.get_terrain().cpu().numpy()[:, :124].astype(np.float64), o32.get_terrain()
            bad = run & (tgr != tcr).any(axis=1)
            if bad.any():
                fail(f"t={t}: terrain record differs in running envs {np.nonzero(bad)[0][:8].tolist()}")
            adv = run & (tc[:, TW.NEXT_STEP_INDEX] > tk0[:, TW.NEXT_STEP_INDEX])
            S["advances"] += int(adv.sum())
            S["ring_writes"] += int((run & (tcr[:, 120:124] != ter0[:, 120:124]).any(axis=1)).sum())
        if task == M.TASK_WALKER3D_CUSTOM:
            S["retargets"] += int((run & (tk0[:, TW.CLOSE_COUNT] >= tk0[:, TW.STOP_FRAMES] - 1) & (tc[:, TW.DRAW] > tk0[:, TW.DRAW])).sum())
        # ---- envs that finished: the new episode the in-step reset started
        if fin.any():
            for name, g, c, atol in (("obs", og, oc, RESET_ATOL["obs"]), ("state", sg[:, :nd], sc[:, :nd], RESET_ATOL["state"])):
                bad = fin & ~(np.abs(g - c) <= atol).all(axis=1)
                if bad.any():
                    fail(f"t={t}: {name} after the in-step reset differs in envs {np.nonzero(bad)[0][:8].tolist()} (max {np.abs(g - c)[bad].max():.3g})")
            for w, c_ in cls.items():
                if c_ == "skip":
                    continue
                if c_ in ("exact", "contact"):
                    bad = fin & (tg[:, w] != tc[:, w])
                else:
                    bad = fin & ~_task_close(tg[:, w], tc[:, w])
                if bad.any():
                    fail(f"t={t}: task word {w} after the in-step reset differs in envs {np.nonzero(bad)[0][:8].tolist()}: {tg[bad, w][:4]} vs {tc[bad, w][:4]}")
            if stepper:
                bad = fin & ~(np.abs(tgr - tcr) <= RESET_ATOL["terrain"]).all(axis=1)
                if bad.any():
                    fail(f"t={t}: terrain after the in-step reset differs in envs {np.nonzero(bad)[0][:8].tolist()}")
        # ---- the Monitor's episode records
        ret64 += rc.astype(np.float64)
        tol_r += 5e-2 + 3 * np.abs(r6.astype(np.float64) - rc.astype(np.float64))
        serial = first_serial + t
        rec = ep["records"][serial % ep["slots"]].numpy()
        got = np.nonzero(rec[:, 0] == np.array(serial, np.uint32).view(np.int32))[0]
        if not np.array_equal(got, np.nonzero(dg != 0)[0]):
            fail(f"t={t}: episode records for envs {got[:8].tolist()}, done in {np.nonzero(dg != 0)[0][:8].tolist()}")
        for e in np.nonzero(fin)[0]:
            if e not in got:
                continue
            S["episodes"] += 1
            r, l, flags = rec[e, 1:2].view(np.float32)[0], int(rec[e, 2]), int(rec[e, 3])
            if l != int(tk0[e, TW.T]) + 1:
                fail(f"t={t}: env {e}: episode length {l}, the oracle's is {int(tk0[e, TW.T]) + 1}")
            if (flags & 2) != (int(dc[e]) & 2):
                fail(f"t={t}: env {e}: TimeLimit bit of the record {flags & 2}, the oracle's done {int(dc[e])}")
            # |r - f64 sum of the oracle's rewards| within the summed per-step tolerance, plus the f32 running sum's rounding
            slack = tol_r[e] + l * 2.0 ** -23 * (abs(ret64[e]) + tol_r[e] + 1.0)
            if np.isfinite(ret64[e]) and not abs(float(r) - ret64[e]) <= slack:
                fail(f"t={t}: env {e}: Monitor return {float(r):.6g}, f64 sum of the oracle's rewards {ret64[e]:.6g} (allowed {slack:.3g})")
        ret64[dc != 0] = 0.0; tol_r[dc != 0] = 0.0
        ret64[mism] = np.nan        # an episode whose end the two sides disagree on: its next return is not compared (one Monitor restarted)
        if (mism & (dc == 0)).any():
            o32.reset(seed=seed, mask=(mism & (dc == 0)).astype(np.uint8))   # the HIP side reset: so does the oracle (HIP is forced from it next)
    summary = dict(S)
    if cont_g:
        eg, ec = np.concatenate(cont_g), np.concatenate(cont_c)
        gs, rs = np.concatenate(cont_same), np.concatenate(cont_ref_same)
        summary.update(cont_med=float(np.median(eg)), cont_med_ref=float(np.median(ec)), cont_p90=float(np.percentile(eg, 90)),
                       cont_p90_ref=float(np.percentile(ec, 90)), cont_p99=float(np.percentile(eg, 99)), cont_p99_ref=float(np.percentile(ec, 99)),
                       cont_worst_same=float(gs.max()) if gs.size else 0.0, cont_worst_same_ref=float(rs.max()) if rs.size else 0.0,
                       cont_tail=int((eg > 30).sum()), cont_tail_ref=int((ec > 30).sum()))
        # the yardstick of the step's state (test_gpu_parity / test_gpu_cassie): the kernel is as close to the f64 oracle as the f32 oracle is
        if not np.median(eg) <= 3 * np.median(ec) + 0.05:
            fail(f"continuous task words: median error vs f64 {np.median(eg):.3g}, f32 oracle's {np.median(ec):.3g}")
        if not np.percentile(eg, 90) <= 3 * np.percentile(ec, 90) + 0.5:
            fail(f"continuous task words: p90 error vs f64 {np.percentile(eg, 90):.3g}, f32 oracle's {np.percentile(ec, 90):.3g}")
        if not np.percentile(eg, 99) <= 3 * np.percentile(ec, 99) + 2.0:
            fail(f"continuous task words: p99 error vs f64 {np.percentile(eg, 99):.3g}, f32 oracle's {np.percentile(ec, 99):.3g}")
        if not (eg > 30).sum() <= (ec > 30).sum() + max(2, len(eg) // 100):
            fail(f"continuous task words: {(eg > 30).sum()} samples beyond 30 units, f32 oracle {(ec > 30).sum()}")
        # steps with the oracle's decisions in every substep: worst sample within 10 x the f32 oracle's worst on ITS matching steps (+ 2 units)
        if gs.size and not gs.max() <= 10 * (rs.max() if rs.size else 0.0) + 2.0:
            fail(f"continuous task words on matching steps: worst {gs.max():.3g}, f32 oracle vs f64 {rs.max() if rs.size else 0.0:.3g}")
    # done flags may differ only in a bounded share of the samples (height on the threshold)
    if S["done_mismatch"] > max(2, S["samples"] // 100):
        fail(f"done flags differ in {S['done_mismatch']} of {S['samples']} samples")
    for e in (env, twin):
        e.close()
    return fails, summary


STEP_WRITE_CASES = (
    [(env_id, task, 64, 40, {}) for env_id, task in [
        ("Walker3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM), ("Walker3DStepperEnv-v0", M.TASK_WALKER3D_STEPPER),
        ("Child3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM), ("MikeStepperEnv-v0", M.TASK_WALKER3D_STEPPER),
        ("Walker2DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM), ("Crab2DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM),
        ("LaikagoCustomEnv-v0", M.TASK_WALKER3D_CUSTOM), ("LaikagoStepperEnv-v0", M.TASK_WALKER3D_STEPPER)]]      # test_gpu_parity.TASKS
    + [("Walker3DPlannerEnv-v0", M.TASK_WALKER3D_PLANNER, 64, 30, {}),
       ("CassieEnv-v0", M.TASK_CASSIE, 16, 10, {}), ("Cassie2DEnv-v0", M.TASK_CASSIE, 16, 10, {}),
       ("CassiePhaseMocca2DEnv-v0", M.TASK_CASSIE, 16, 10, {}),
       ("Walker3DStepperEnv-v0", M.TASK_WALKER3D_STEPPER, 64, 40, {"random_reward": True}),
       ("Walker3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM, 64, 30, {"max_rows": 32}),
       ("Walker3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM, 64, 30, {"max_rows": 64}),
       ("Walker3DStepperEnv-v0", M.TASK_WALKER3D_STEPPER, 64, 30, {"max_rows": 32}),
       ("Walker3DStepperEnv-v0", M.TASK_WALKER3D_STEPPER, 64, 30, {"max_rows": 64})])


def _case_id(c):
    return c[0] + "".join(f"-{k}={v}" for k, v in c[4].items())


@pytest.mark.parametrize("env_id,task,n,steps,kw", STEP_WRITE_CASES, ids=[_case_id(c) for c in STEP_WRITE_CASES])
def test_everything_a_step_writes_matches_the_oracle(env_id, task, n, steps, kw):
    kw = dict(kw)
    rr = kw.pop("random_reward", False)
    cassie = task == M.TASK_CASSIE
    fails, s = run_step_writes(env_id, task, n, steps, kw=kw, random_reward=rr, act_scale=0.3 if cassie else 1.0)
    print(f"\n{_case_id((env_id, task, n, steps, dict(kw, **({'random_reward': 1} if rr else {}))))}: in-step resets {s['resets']} "
          f"(TimeLimit {s['timelimits']}, terminated {s['terminations']}), episode records compared {s['episodes']}, plank advances {s['advances']} "
          f"(ring rows rewritten {s['ring_writes']}), re-targets {s['retargets']}; done flags differing {s['done_mismatch']} / {s['samples']}; "
          f"contact-class word flips {s['contact_flips']} (f64 oracle vs f32: {s['contact_flips_ref']})")
    if "cont_med" in s:
        print(f"  continuous task words vs f64 [units]: median {s['cont_med']:.3g} (f32 oracle {s['cont_med_ref']:.3g}), p90 {s['cont_p90']:.3g} "
              f"({s['cont_p90_ref']:.3g}), p99 {s['cont_p99']:.3g} ({s['cont_p99_ref']:.3g}); worst on matching steps vs f32 oracle "
              f"{s['cont_worst_same']:.3g} (f32 vs f64 on its matching steps {s['cont_worst_same_ref']:.3g}); > 30 units {s['cont_tail']} ({s['cont_tail_ref']})")
    for f in fails:
        print("  FAIL", f)
    assert not fails, fails[:5]
    # the sample really holds what is checked
    assert s["timelimits"] > 0 and s["episodes"] > 0, s
    if not cassie and "2D" not in env_id:
        assert s["terminations"] > 0 and s["resets"] >= n // 3, s
    if task == M.TASK_WALKER3D_STEPPER and "Laikago" not in env_id:
        assert s["advances"] > 0 and s["ring_writes"] > 0, s
    if task == M.TASK_WALKER3D_CUSTOM:
        assert s["retargets"] > 0, s


@pytest.mark.parametrize("control", ["oracle_max_episode_steps", "oracle_electricity_cost", "corrupted_task_word"])
def test_the_step_write_comparison_catches_a_wrong_word(control):
    """Negative controls: the same comparison against an oracle whose blob has one task constant off, or with one word of the HIP task record
    changed after the step, must fail."""
    if control == "oracle_max_episode_steps":
        fails, _ = run_step_writes("Walker3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM, 32, 6,
                                   oracle_model_edit=lambda m: setattr(m, "max_episode_steps", int(m.max_episode_steps) - 1))
    elif control == "oracle_electricity_cost":           # (reaches the reward only: caught by the Monitor's episode returns)
        fails, _ = run_step_writes("Walker3DCustomEnv-v0", M.TASK_WALKER3D_CUSTOM, 32, 6,
                                   oracle_model_edit=lambda m: setattr(m, "electricity_cost", float(m.electricity_cost) * 1.5))
    else:
        def corrupt(t, tk):
            if t == 3:
                tk = tk.clone()
                tk[5:, TW.EPISODE] += 1                # one word of the record, in the envs that did not just reset
            return tk
        fails, _ = run_step_writes("Walker3DStepperEnv-v0", M.TASK_WALKER3D_STEPPER, 32, 6, corrupt=corrupt)
    print(f"\n{control}: {len(fails)} failure(s), first: {fails[0] if fails else None}")
    assert fails, control


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. the debug buffer (and the other attachments that only collect) change no bit

DBG_CASES = [("Walker3DCustomEnv-v0", {}), ("Walker3DCustomEnv-v0", {"max_rows": 32}), ("Walker3DCustomEnv-v0", {"max_rows": 64}),
             ("Walker3DStepperEnv-v0", {}), ("Walker3DStepperEnv-v0", {"max_rows": 32}), ("Walker3DStepperEnv-v0", {"max_rows": 64}),
             ("CassieEnv-v0", {}), ("Walker3DPlannerEnv-v0", {})]


def _free_run_bitwise(env_id, kw, attach, n=192, steps=300):
    import torch
    from mocca_envs_amd.vec_env import VecEnv
    cassie = env_id.startswith("Cassie")
    steps = 60 if cassie else steps
    a_env = VecEnv(env_id, n, auto_reset=True, seed=13, **kw)               # the product path: nothing attached
    b_env = VecEnv(env_id, n, auto_reset=True, seed=13, **kw)
    probe = attach(b_env)
    a_env.reset(); b_env.reset()
    tk = a_env.get_task()                                                   # TimeLimit truncations (and their in-step resets) in the sample
    tk[::3, TW.T] = int(a_env.model.max_episode_steps) - 5
    a_env.set_task(tk); b_env.set_task(tk)
    nd = 13 + 2 * int(a_env.model.n_joints)
    g = torch.Generator(device="cuda").manual_seed(6)
    n_done = 0
    for t in range(steps):
        act = (torch.rand(n, a_env.act_dim, device="cuda", generator=g) * 2 - 1) * (0.2 if cassie else 1.0)
        ra, rb = a_env.step(act), b_env.step(act)
        for name, x, y in zip(("obs", "reward", "done", "info"), ra, rb):
            assert torch.equal(x, y), (env_id, kw, name, t)
        assert torch.equal(a_env.get_state()[:, :nd], b_env.get_state()[:, :nd]), (env_id, kw, "state", t)
        assert torch.equal(a_env.get_task(), b_env.get_task()), (env_id, kw, "task", t)
        if "Stepper" in env_id:
            assert torch.equal(a_env.get_terrain(), b_env.get_terrain()), (env_id, kw, "terrain", t)
        n_done += int((ra[2] != 0).sum())
    torch.cuda.synchronize()
    assert n_done > n // 3, n_done                                          # in-kernel resets happened
    if probe is not None:
        assert bool((probe() != 0).any()), "the attachment collected nothing"
    a_env.close(); b_env.close()
    return n_done


@pytest.mark.parametrize("env_id,kw", DBG_CASES, ids=[_case_id((e, 0, 0, 0, k)) for e, k in DBG_CASES])
def test_debug_buffer_changes_no_bit(env_id, kw):
    """With the debug buffer attached the kernel also writes the active-set words and waits for its stores after every substep
    (dbg_fold_step): what users and bench.py run has no buffer.  Both must write the same bits, in-step resets included."""
    def attach(e):
        d = e.set_debug(True)
        return lambda: d
    n_done = _free_run_bitwise(env_id, kw, attach)
    print(f"\n{env_id} {kw}: bit-identical with and without the debug buffer, {n_done} in-step resets")


def _attach_episode_stats(e):
    ep = e.episode_stats(True)
    return lambda: ep["totals"]


def _attach_terminal_obs(e):
    buf = e.keep_terminal_obs(True)
    return lambda: buf


def _attach_order_and_pace(e):
    from mocca_envs_amd import lib as L
    e.set_param(L.PARAM_ORDER_EVERY, 3)
    e.set_param(L.PARAM_PACE_TICKS, 180000)
    return None


@pytest.mark.parametrize("env_id", ["Walker3DCustomEnv-v0", "Walker3DStepperEnv-v0"])
@pytest.mark.parametrize("what", ["episode_stats", "terminal_obs", "order_and_pace"])
def test_collecting_attachments_change_no_bit(env_id, what):
    """episode_stats(True), a terminal-observation buffer and the ORDER_EVERY / pace settings only collect or reorder: same bits."""
    attach = {"episode_stats": _attach_episode_stats, "terminal_obs": _attach_terminal_obs, "order_and_pace": _attach_order_and_pace}[what]
    n_done = _free_run_bitwise(env_id, {}, attach, steps=200)
    print(f"\n{env_id} {what}: bit-identical, {n_done} in-step resets")
