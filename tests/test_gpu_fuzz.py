"""The step kernel on FUZZED blobs from ADVERSARIAL states (tests/fuzz_blobs.py): every compiled topology and step-kernel instance, with
random hinge axes and joint frames, full inertia tensors, per-geom frictions and random global constants -- values no shipped robot
takes -- started from states a rollout from reset does not reach (upside-down bases, w < 0, joints past their stops, speeds beyond the
clamp, deep penetration at the row cap, bases 500 m out, tilted planks, a steep height field).
  * leg A: one substep (n_substeps = 1, Cassie: n_llc = 1) against the f32 oracle with the f64 oracle as the yardstick, by the
    active-set matching and the bars of test_gpu_substep.test_single_substep_parity_with_matching_active_sets (tests/substep_compare.py);
  * leg B: one full env.step() (the blob's own substeps), teacher-forced: obs, reward, done against the oracle by the error-unit and
    yardstick scheme of test_gpu_parity.test_teacher_forced_steps; then the same state with q -> -q must give the same step;
  * negative controls: the oracle runs a blob B' that differs from the kernel's B in one value -- the leg-A comparison must fail.
tests/test_oracle_fuzz.py holds the f64 oracle to the dense reference on the same blobs.  Needs a real MI355X: -m gpu."""
import numpy as np
import pytest

import fuzz_blobs as F
from mocca_envs_amd import model as M
from substep_compare import SubstepStats

pytestmark = pytest.mark.gpu

N_ENVS, N_BLOBS = 256, 4
# Cases whose samples must reach max_rows (>= 1 %) and truncate contacts at max_contacts.  Not in the first set: the planar walkers at 48
# rows (limit + 3 x contact rows reach at most 7 + 36 = 43 / 6 + 36 = 42 < 48), the quadruped at 64 rows / 20 contacts (a few per mille of
# samples reach either: 20 contacts of one lying quadruped) and Cassie, whose assembled loops keep its legs bent: a flat-laid Cassie touches with at most 10 of its slots,
# so neither cap is met -- a Cassie blob with caps that its contacts do reach runs the same instance (cassie-full, the limit rows of the
# limits class and the six closure rows are in every sample)
ROW_CAP_CASES = {"walker3d-compact", "walker3d-full", "walker3d-wide", "walker3d-massive-full", "walker2d-compact", "crab2d-compact",
                 "laikago-compact", "laikago-full", "stepper-walker3d-full", "stepper-walker3d-compact", "stepper-laikago-full",
                 "stepper-laikago-compact", "planner-steep-full"}
CONTACT_CAP_CASES = ROW_CAP_CASES | {"walker2d-full", "crab2d-full"}
ERR_ABS, ERR_REL = 1e-3, 1e-3     # test_gpu_parity's units for a whole step


def _err_units(a, b):
    return np.abs(a - b) / (ERR_ABS + ERR_REL * np.abs(b))


def _one_substep(m):
    m1 = M.MoccaModel.from_bytes(m.to_bytes())
    m1.n_substeps = 1
    if m1.n_closures:
        m1.n_llc = 1
    return m1


class _Rig:
    """Kernel + f32 oracle + f64 oracle on one blob, set to one batch of adversarial states."""

    def __init__(self, name, m, n=N_ENVS):
        from mocca_envs_amd.vec_env import VecEnv, _DEFAULT_PARAMS
        from oracle.oracle import Oracle, PARAM_CURRICULUM
        _, env_id, task, _, _ = F.CASE_BY_NAME[name]
        self.task, self.n = task, n
        blob = m.to_bytes()
        self.env = VecEnv(env_id, n, auto_reset=False, seed=4, model_blob=blob)
        self.dbg = self.env.set_debug(True)
        self.o32, self.o64 = Oracle(blob, task, n, "f32"), Oracle(blob, task, n, "f64")
        for pid, val in _DEFAULT_PARAMS.get(env_id, {}).items():
            self.o32.set_param(pid, val); self.o64.set_param(pid, val)
        if task == M.TASK_WALKER3D_STEPPER:
            self.env.set_param(2, 9); self.o32.set_param(PARAM_CURRICULUM, 9); self.o64.set_param(PARAM_CURRICULUM, 9)
        if task == M.TASK_WALKER3D_PLANNER:
            self.env.set_heightfield(*F.steep_field())
            self.o32.set_heightfield(*self.env.height_field); self.o64.set_heightfield(*self.env.height_field)
        self.env.reset(); self.o32.reset(seed=4); self.o64.reset(seed=4)
        self.task0 = self.o32.get_task()      # every load() starts from this task record (a step advances the oracles' own)

    def load(self, st, ter=None, negate_quat=False):
        from mocca_envs_amd.vec_env import task_from_float64
        st = st.copy()
        if negate_quat:
            st[:, 3:7] *= -1
        for o in (self.o32, self.o64):
            o.set_state(st)
        self.env.set_state(st.astype(np.float32))
        tk = self.task0
        self.env.set_task(task_from_float64(tk)); self.o32.set_task(tk); self.o64.set_task(tk)
        if ter is not None:
            self.o32.set_terrain(ter); self.o64.set_terrain(ter)
            t = np.zeros((self.n, 128), np.float32); t[:, :124] = ter
            self.env.set_terrain(t)

    def close(self):
        self.env.close()


def _states(name, m, rng, rig):
    """Adversarial states (rounded to fp32: both sides start from the same numbers) and the terrain record of the case."""
    task = rig.task
    ground = (lambda x, y: rig.o32.height_at(x, y)) if task == M.TASK_WALKER3D_PLANNER else None
    st, labels = F.adversarial_states(m, rng, rig.n, ground=ground, far=task in (M.TASK_WALKER3D_CUSTOM, M.TASK_CASSIE))
    if task == M.TASK_WALKER3D_PLANNER:       # scattered over the steep field, at the same clearance over the local surface
        import dense_reference as D
        mdl = D.Model(m)
        for i in range(rig.n):
            st[i, 0:2] = rng.uniform(-14, 14, 2)
            st[i, 2] = 0.0
            st[i, 2] = -F._lowest_point(mdl, st[i, 0:3], st[i, 3:7], st[i, 13:13 + m.n_joints], ground) + rng.uniform(-0.03, 0.02)
    ter = F.plank_terrain(m, rng, st, rig.o32.get_terrain()) if task == M.TASK_WALKER3D_STEPPER else None
    st[:, 3:7] /= np.linalg.norm(st[:, 3:7], axis=1)[:, None]
    return st.astype(np.float32).astype(np.float64), labels, ter


def _leg_a(name, m, st, ter, act, stats, oracle_blob=None):
    """One substep of the kernel on blob m against the oracles on oracle_blob (default: m).  Returns the f32 oracle's debug records."""
    import torch
    m1 = _one_substep(m)
    rig = _Rig(name, m1)
    if oracle_blob is not None:
        ob = _one_substep(oracle_blob)
        from oracle.oracle import Oracle
        rig.o32, rig.o64 = Oracle(ob.to_bytes(), rig.task, rig.n, "f32"), Oracle(ob.to_bytes(), rig.task, rig.n, "f64")
        for o in (rig.o32, rig.o64):
            if rig.task == M.TASK_WALKER3D_STEPPER:
                o.set_param(2, 9)
            if rig.task == M.TASK_WALKER3D_PLANNER:
                o.set_heightfield(*rig.env.height_field)
            o.reset(seed=4)
    rig.load(st, ter)
    rig.o32.clear_debug()
    rig.env.step(torch.from_numpy(act).cuda())
    rig.o32.step(act); rig.o64.step(act)
    dc = rig.o32.get_debug()
    stats.add(rig.env.get_state().cpu().numpy(), rig.o32.get_state(), rig.o64.get_state(), rig.dbg.cpu().numpy(), dc, rig.o64.get_debug())
    lds = rig.env.kernel_info()["lds_bytes"]
    rig.close()
    return dc, lds


def _instance_lds(name, m):
    """LDS bytes of the step-kernel instance the library picks for this blob under each of the three caps."""
    from mocca_envs_amd.vec_env import VecEnv
    _, env_id, _, _, _ = F.CASE_BY_NAME[name]
    out = {}
    for cname, caps in F.CAPS.items():
        mm = _one_substep(m)
        mm.max_rows, mm.max_contacts = caps
        e = VecEnv(env_id, 8, auto_reset=False, seed=4, model_blob=mm.to_bytes())
        out[cname] = e.kernel_info()["lds_bytes"]
        e.close()
    return out


@pytest.mark.parametrize("name", [c[0] for c in F.CASES])
def test_fuzzed_blobs_from_adversarial_states(name):
    import torch
    _, env_id, task, massive, caps = F.CASE_BY_NAME[name]
    nj = None
    stats = None
    counts = {c: 0 for c in F.CLASSES + ("w_negative", "qd_beyond_clamp", "at_max_rows", "contacts_truncated", "terrain_contacts")}
    max_limit_rows, n_samples, lds_seen = 0, 0, set()
    legb = {"state": [], "obs": [], "rew": [], "state_ref": [], "obs_ref": [], "rew_ref": [], "done_diff": 0, "done_diff_ref": 0, "done_detail": []}
    sym_worst = sym_ref = 0.0
    for k in range(N_BLOBS):
        m, rng = F.case_blob(name, k)
        nj = m.n_joints
        if stats is None:
            stats = SubstepStats(13 + 2 * nj)
        probe = _Rig(name, m)
        st, labels, ter = _states(name, m, rng, probe)
        act_dim = probe.env.act_dim
        probe.close()
        act = rng.uniform(-1, 1, (N_ENVS, act_dim)).astype(np.float32)
        # ---- leg A: one substep
        dc, lds = _leg_a(name, m, st, ter, act, stats)
        lds_seen.add(lds)
        for c in F.CLASSES + ("w_negative",):
            counts[c] += int(labels[c].sum())
        counts["qd_beyond_clamp"] += int((np.abs(st[:, 13 + nj:13 + 2 * nj]) > m.max_qd).any(axis=1).sum())
        counts["at_max_rows"] += int((dc[:, 0] == m.max_rows).sum())
        counts["contacts_truncated"] += int((dc[:, 12] > 0).sum())
        counts["terrain_contacts"] += int((dc[:, 3] != 0).sum() + (dc[:, 4] != 0).sum())
        max_limit_rows = max(max_limit_rows, int(dc[:, 1].max()))
        n_samples += N_ENVS
        # ---- leg B: one full env.step(), teacher-forced; then the same states with q -> -q
        rig = _Rig(name, m)
        rig.load(st, ter)
        og, rg, dg, _ = (x.cpu().numpy() for x in rig.env.step(torch.from_numpy(act).cuda()))
        sg = rig.env.get_state().cpu().numpy()
        oc, rc, dc_, _ = rig.o32.step(act)
        o6, r6, d6, _ = rig.o64.step(act)
        sc, s6 = rig.o32.get_state(), rig.o64.get_state()
        ok = np.isfinite(sc).all(axis=1) & np.isfinite(s6).all(axis=1) & np.isfinite(oc).all(axis=1)
        assert np.isfinite(sg[ok]).all() and np.isfinite(og[ok]).all() and np.isfinite(rg[ok]).all(), "kernel non-finite where the oracles are finite"
        nd = 13 + 2 * nj
        legb["state"].append(_err_units(sg[ok][:, :nd], s6[ok][:, :nd]).max(axis=1))
        legb["state_ref"].append(_err_units(sc[ok][:, :nd], s6[ok][:, :nd]).max(axis=1))
        legb["obs"].append(_err_units(og[ok], o6[ok]).max(axis=1))
        legb["obs_ref"].append(_err_units(oc[ok], o6[ok]).max(axis=1))
        legb["rew"].append(np.abs(rg[ok] - r6[ok]))
        legb["rew_ref"].append(np.abs(rc[ok] - r6[ok]))
        legb["done_diff"] += int(((dg != d6) & ok).sum())
        legb["done_diff_ref"] += int(((dc_ != d6) & ok).sum())
        h, thr = _termination_height(m, task, s6, o6)
        for e in np.flatnonzero(ok & (dg != d6) & (dc_ == d6)):     # what a flag the f32 oracle gets right looks like on the kernel's side
            legb["done_detail"].append(f"blob {k} env {e}: height {h[e]:.4f} (threshold {thr:.3f}), kernel state {_err_units(sg[e, :nd], s6[e, :nd]).max():.3g} "
                                       f"units from f64 (f32 oracle {_err_units(sc[e, :nd], s6[e, :nd]).max():.3g}), classes {[c for c in labels if labels[c][e]]}")
        rig.load(st, ter, negate_quat=True)
        og2, rg2, dg2, _ = (x.cpu().numpy() for x in rig.env.step(torch.from_numpy(act).cuda()))
        sg2 = rig.env.get_state().cpu().numpy()
        oc2, rc2, _, _ = rig.o32.step(act)        # the f32 oracle's own q -> -q difference: the yardstick of the symmetry check
        sc2 = rig.o32.get_state()
        rig.close()
        fo = ok & np.isfinite(sc2).all(axis=1)
        qs = np.where((sc[fo][:, 3:7] * sc2[fo][:, 3:7]).sum(axis=1) < 0, -1.0, 1.0)[:, None]
        sc2 = sc2.copy(); sc2[fo, 3:7] *= qs
        for a_, b_ in ((oc[fo], oc2[fo]), (rc[fo], rc2[fo]), (sc[fo][:, :nd], sc2[fo][:, :nd])):
            sym_ref = max(sym_ref, float((np.abs(a_ - b_) / (1e-5 * (1 + np.abs(a_)))).max()) if a_.size else 0.0)
        fin = np.isfinite(sg).all(axis=1) & np.isfinite(og).all(axis=1) & np.isfinite(rg)
        # the -q step is finite wherever the +q step is (a NaN must not drop out of the comparison below)
        assert (np.isfinite(sg2[fin]).all(axis=1) & np.isfinite(og2[fin]).all(axis=1) & np.isfinite(rg2[fin])).all()
        qa, qb = sg[fin][:, 3:7], sg2[fin][:, 3:7]
        qsign = np.where((qa * qb).sum(axis=1) < 0, -1.0, 1.0)[:, None]
        sg2 = sg2.copy(); sg2[fin, 3:7] = qb * qsign
        tol = lambda a: 1e-5 * (1 + np.abs(a))
        for a_, b_ in ((og[fin], og2[fin]), (rg[fin], rg2[fin]), (sg[fin][:, :nd], sg2[fin][:, :nd])):
            sym_worst = max(sym_worst, float((np.abs(a_ - b_) / tol(a_)).max()) if a_.size else 0.0)
        np.testing.assert_array_equal(dg[fin], dg2[fin])
    # ---- which instance ran
    inst = _instance_lds(name, m)
    assert lds_seen == {inst[caps]}, (lds_seen, inst)
    if not env_id.startswith("Cassie"):            # a tree with loop closures never runs the compact instance
        assert inst["compact"] < inst["full"], inst
    assert inst["full"] < inst["wide"], inst
    bad, msg = stats.failures()
    cat = {k: np.concatenate(v) for k, v in legb.items() if isinstance(v, list) and k != "done_detail"}
    q = lambda x, p: float(np.percentile(x, p))
    print(f"\n{name} [{caps} instance, {inst[caps]} B LDS, {N_BLOBS} blobs x {N_ENVS} envs]: leg A: {msg}")
    print(f"  sample: " + ", ".join(f"{k} {v}" for k, v in counts.items()) + f", most limit rows {max_limit_rows}")
    print(f"  leg B (one env.step, units of 1e-3 (1+|x|) against the f64 oracle): state GPU median {q(cat['state'], 50):.3g} p99 "
          f"{q(cat['state'], 99):.3g} | f32 oracle median {q(cat['state_ref'], 50):.3g} p99 {q(cat['state_ref'], 99):.3g}; obs GPU p99 "
          f"{q(cat['obs'], 99):.3g} | f32 {q(cat['obs_ref'], 99):.3g}; reward abs p99 GPU {q(cat['rew'], 99):.3g} | f32 {q(cat['rew_ref'], 99):.3g}; "
          f"done differs GPU {legb['done_diff']} | f32 {legb['done_diff_ref']}; q -> -q worst {sym_worst:.3g} units of 1e-5 (1+|x|) "
          f"(f32 oracle's own {sym_ref:.3g})" + "".join(f"\n    done differs: {d}" for d in legb["done_detail"]))
    # the sample really holds every class
    for c in ("orientation", "limits", "speed", "penetration", "warm", "w_negative", "qd_beyond_clamp"):
        assert counts[c] > 0, c
    if task in (M.TASK_WALKER3D_CUSTOM, M.TASK_CASSIE):
        assert counts["position"] > 0
    assert max_limit_rows >= 5
    if name in ROW_CAP_CASES:
        assert counts["at_max_rows"] >= 0.01 * n_samples, counts["at_max_rows"]
    if name in CONTACT_CAP_CASES:
        assert counts["contacts_truncated"] > 0
    if task in (M.TASK_WALKER3D_STEPPER, M.TASK_WALKER3D_PLANNER):
        assert counts["terrain_contacts"] >= 0.1 * n_samples      # plank / height-field contacts
    # leg A: the bars of test_single_substep_parity_with_matching_active_sets
    assert not bad, bad
    # leg B: the kernel is as close to the f64 oracle as the f32 oracle is (test_gpu_parity.test_teacher_forced_steps)
    for k in ("state", "obs", "rew"):
        assert q(cat[k], 50) <= 3 * q(cat[k + "_ref"], 50) + (0.01 if k != "rew" else 1e-5), (k, q(cat[k], 50), q(cat[k + "_ref"], 50))
        assert q(cat[k], 99) <= 3 * q(cat[k + "_ref"], 99) + (0.1 if k != "rew" else 1e-3), (k, q(cat[k], 99), q(cat[k + "_ref"], 99))
    assert legb["done_diff"] <= 2 * legb["done_diff_ref"] + 0.002 * n_samples, legb["done_detail"]
    # q and -q are one rotation: the same step to fp32 -- 1 unit of 1e-5 (1 + |x|), or 3 x what the f32 oracle itself shows, whichever
    # is larger (a step of several substeps amplifies a last-bit difference of the first one exactly as any other rounding)
    assert sym_worst < max(1.0, 3 * sym_ref), (sym_worst, sym_ref)


def _termination_height(m, task, s6, o6):
    """The height the termination test reads (from the f64 oracle's new state) and its threshold: Cassie, the base above its lower foot
    (its foot points) against alive_height; the walkers, observation word 0 against the termination height (the Stepper's at curriculum 9)."""
    if task == M.TASK_CASSIE:
        import dense_reference as D
        mdl = D.Model(m)
        h = np.full(len(s6), np.inf)
        for e in range(len(s6)):
            if np.isfinite(s6[e]).all():
                R, o = D.fk(mdl, s6[e, 0:3], D._quat_mat(s6[e, 3:7]), np.concatenate([[0.0], s6[e, 13:13 + m.n_joints]]))
                h[e] = s6[e, 2] - min((o[m.foot_body[f]] + R[m.foot_body[f]] @ np.array(list(m.foot_point[f])))[2] for f in range(m.n_feet))
        return h, float(m.alive_height)
    return o6[:, 0], float(m.term_height_cur[1] if task == M.TASK_WALKER3D_STEPPER else m.termination_height)


def _perturbed(m, what):
    """Blob B' = B with one value changed."""
    mp = M.MoccaModel.from_bytes(m.to_bytes())
    if what == "jaxis rotated 2e-3 rad":
        b = 3
        a = np.array(list(mp.jaxis[b]), float)
        perp = np.cross(a, [1.0, 0.0, 0.0]); perp /= np.linalg.norm(perp)
        a2 = a * np.cos(2e-3) + perp * np.sin(2e-3)
        for k in range(3):
            mp.jaxis[b][k] = a2[k]
    elif what == "xy <-> xz in one link's inertia":
        b = max(range(mp.n_bodies), key=lambda b: abs(mp.inertia[b][3] - mp.inertia[b][4]))
        mp.inertia[b][3], mp.inertia[b][4] = mp.inertia[b][4], mp.inertia[b][3]
    elif what == "one jrot transposed":
        b = 2
        R = np.array(list(mp.jrot[b]), float).reshape(3, 3).T
        for k in range(9):
            mp.jrot[b][k] = R.flat[k]
    elif what == "one geom's friction x 1.1":
        g = max((g for g in range(mp.n_geoms) if mp.g_foot[g] >= 0), key=lambda g: mp.g_friction[g])
        mp.g_friction[g] *= 1.1
    return mp.finalize_tables()


@pytest.mark.parametrize("what", ["jaxis rotated 2e-3 rad", "xy <-> xz in one link's inertia", "one jrot transposed", "one geom's friction x 1.1"])
def test_negative_controls_fail_the_comparison(what):
    """The oracle runs B' while the kernel runs B: the leg-A comparison must report a failure -- the fuzz can see each of these errors."""
    name = "walker3d-full"
    m, rng = F.case_blob(name, 0)
    probe = _Rig(name, m)
    st, _, ter = _states(name, m, rng, probe)
    act = rng.uniform(-1, 1, (N_ENVS, probe.env.act_dim)).astype(np.float32)
    probe.close()
    # the same comparison on B itself passes ...
    ok_stats = SubstepStats(13 + 2 * m.n_joints)
    _leg_a(name, m, st, ter, act, ok_stats)
    bad0, _ = ok_stats.failures()
    # ... and on B against B' it fails
    stats = SubstepStats(13 + 2 * m.n_joints)
    _leg_a(name, m, st, ter, act, stats, oracle_blob=_perturbed(m, what))
    bad, msg = stats.failures()
    print(f"\nnegative control '{what}': the comparison reports {bad} ({msg})")
    assert not bad0, bad0
    assert bad, "the comparison did not see the perturbed blob"
