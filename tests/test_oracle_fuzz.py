"""The f64 oracle against the dense reference on the FUZZED blobs of tests/test_gpu_fuzz.py (tests/fuzz_blobs.py, same seeds), from
adversarial states: with it the chain  HIP kernel -> f32 oracle -> f64 oracle -> dense reference  holds on exactly the blobs the GPU test
runs -- random hinge axes and joint frames, full inertia tensors, per-geom frictions, random global constants.  CPU only."""
import numpy as np
import pytest

import dense_reference as D
import fuzz_blobs as F
from mocca_envs_amd import model as M
from oracle.oracle import Oracle
from test_oracle_dense import _compare

# one case per topology / task (the caps variants run the same recursions: the wide caps are in the list for rows beyond 48)
DENSE_CASES = ["walker3d-wide", "walker3d-massive-full", "walker2d-full", "crab2d-compact", "laikago-full", "cassie-full",
               "cassie-massive-full", "cassie2d-full", "stepper-walker3d-full", "stepper-laikago-compact", "planner-steep-full"]


def _setup(name, m, rng, n):
    """Oracle (f64, one env), adversarial states and the terrain of the case: (orc, states, labels, planks-of-state fn, heightfield)."""
    _, env_id, task, _, _ = F.CASE_BY_NAME[name]
    orc = Oracle(m.to_bytes(), task, 1, "f64")
    hf = None
    if task == M.TASK_WALKER3D_PLANNER:
        data, scale = F.steep_field()
        orc.set_heightfield(data, scale)
        hf = (data.astype(np.float64), scale)
    if task == M.TASK_WALKER3D_STEPPER:
        orc.set_param(2, 9)
    orc.reset(seed=1)
    ground = (lambda x, y: orc.height_at(x, y)) if hf is not None else None
    st, labels = F.adversarial_states(m, rng, n, ground=ground, far=task in (M.TASK_WALKER3D_CUSTOM, M.TASK_CASSIE))
    if hf is not None:
        st[:, 0:2] = st[:, 0:2] * 0 + rng.uniform(-14, 14, (n, 2))     # scattered over the field ...
        for i in range(n):                                              # ... at the same clearance over the local surface
            lo = F._lowest_point(D.Model(m), st[i, 0:3] * [1, 1, 0], st[i, 3:7], st[i, 13:13 + m.n_joints], ground)
            st[i, 2] = -lo + rng.uniform(-0.03, 0.02)
    ter = None
    if task == M.TASK_WALKER3D_STEPPER:
        ter = F.plank_terrain(m, rng, st, np.repeat(orc.get_terrain(), n, axis=0))
    return orc, st, labels, ter, hf


def test_generator_self_check():
    """No coordinate axis is left, every inertia is SPD and obeys the triangle inequality, frictions are distinct, every adversarial
    class is drawn -- for every case of the GPU test."""
    cosmin = np.cos(F.AXIS_MIN_ANGLE)
    for name, env_id, task, massive, caps in F.CASES:
        m, rng = F.case_blob(name, 0)
        from mocca_envs_amd.vec_env import compile_model_for
        c = compile_model_for(env_id)
        assert (m.max_rows, m.max_contacts) == F.CAPS[caps]
        for b in range(c.n_bodies):
            assert m.parent[b] == c.parent[b] and m.anc_mask[b] == c.anc_mask[b]
        assert (m.n_geoms, m.n_slots, m.n_pairs, m.n_closures, m.n_feet, m.planar) == (c.n_geoms, c.n_slots, c.n_pairs, c.n_closures, c.n_feet, c.planar)
        for g in range(m.n_geoms):
            assert (m.g_terrain[g], m.g_foot[g], m.g_torso[g], m.g_slot[g], m.g_body[g]) == (c.g_terrain[g], c.g_foot[g], c.g_torso[g], c.g_slot[g], c.g_body[g])
        for b in range(1, m.n_bodies):
            ax = np.array(list(m.jaxis[b]), float)
            assert abs(np.linalg.norm(ax) - 1) < 1e-6 and np.abs(ax).max() < cosmin, (name, b, ax)
            R = np.array(list(m.jrot[b]), float).reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0
            assert np.abs(R - np.eye(3)).max() > 1e-3
        n_full = 0
        for b in range(m.n_bodies):
            if m.mass[b] == 0.0:
                assert not massive or b == 0 or c.mass[b] != 0.0
                continue
            I = F.inertia_matrix(m.inertia[b])
            ev = np.linalg.eigvalsh(I)
            assert ev[0] > 0 and ev[2] < ev[0] + ev[1] + 1e-12, (name, b, ev)
            n_full += min(abs(m.inertia[b][3]), abs(m.inertia[b][4]), abs(m.inertia[b][5])) > 1e-9
        assert n_full >= m.n_bodies // 2, (name, n_full)
        if massive:
            assert all(m.mass[b] > 0 for b in range(1, m.n_bodies))
        fr = [m.g_friction[g] for g in range(m.n_geoms)]
        assert len(set(fr)) == len(fr) and min(fr) >= 0.3 and max(fr) <= 1.5
        lo, hi = M.joint_limits(m)
        fin = hi - lo < 1e20
        assert ((hi - lo)[fin] > 1.5 * np.pi).any() or fin.sum() < 3, name     # some ranges beyond +-3 pi / 4
        st, labels = F.adversarial_states(m, rng, 24, far=task in (M.TASK_WALKER3D_CUSTOM, M.TASK_CASSIE))
        for cls in F.CLASSES + ("w_negative",):
            if cls == "position" and task not in (M.TASK_WALKER3D_CUSTOM, M.TASK_CASSIE):
                continue
            assert labels[cls].any(), (name, cls)
        assert (st[labels["w_negative"], 6] < 0).all()
        assert (np.abs(st[labels["speed"], 13 + m.n_joints:13 + 2 * m.n_joints]) > m.max_qd).any()


@pytest.mark.parametrize("name", DENSE_CASES)
def test_fuzzed_blobs_against_the_dense_reference(name):
    """Two fuzzed blobs of the case (seeds of the GPU test's blobs 0 and 1), three adversarial states each: one f64-oracle substep against
    the dense reference at the tolerance of the random mechanisms (5e-7)."""
    seen = []
    for k in range(2):
        m, rng = F.case_blob(name, k)
        mdl = D.Model(m)
        orc, st, labels, ter, hf = _setup(name, m, rng, 6)
        # orientation, penetration, limits, speed | penetration, position / warm, warm / orientation, speed.  Of the speed class, two joints
        # keep their speed beyond max_qd (the clamp); the other joints are slowed to 5 rad/s and the base spin (up to 30 rad/s) to 3 rad/s,
        # because _compare's orientation bar does not scale with the speeds -- the full class is held to the oracle on the GPU
        for i in (0, 3, 1, 2) if k == 0 else (3, 4, 5, 2):
            if labels["speed"][i]:
                st[i, 10:13] *= min(1.0, 3.0 / np.linalg.norm(st[i, 10:13]))
                qd = st[i, 13 + m.n_joints:13 + 2 * m.n_joints]
                cand = np.setdiff1d(np.arange(m.n_joints), F.loop_joints(m))      # (a closure row would take a loop joint's speed away)
                fast = cand[np.argsort(-np.abs(qd[cand]))[:2]]
                slow = np.setdiff1d(np.arange(m.n_joints), fast)
                qd[slow] = np.clip(qd[slow], -5.0, 5.0)
                qd[fast] = np.sign(qd[fast]) * np.maximum(np.abs(qd[fast]), 1.2 * m.max_qd)
            planks = None
            if ter is not None:
                orc.set_terrain(ter[i:i + 1])
                planks = D.live_planks(mdl, ter[i], 1)
                if m.n_planks == 4:
                    planks = _live_planks4(mdl, ter[i])
            tau = rng.uniform(-40, 40, m.n_joints)
            info = _compare(orc, m, mdl, st[i], tau, planks=planks, tol=5e-7, heightfield=hf)
            seen.append(info["rows"])
            if labels["speed"][i]:       # the speed clamp engaged, on both sides (the new speeds of the two agree to _compare's bar)
                assert np.abs(orc.get_state()[0][13 + m.n_joints:13 + 2 * m.n_joints]).max() == np.float32(m.max_qd)
    print(f"\n{name}: rows per substep {seen}")
    assert max(seen) >= 9


def _live_planks4(mdl, ter):
    """The quadruped Stepper's four live planks (dense_reference.live_planks reads three)."""
    table, info = np.asarray(ter[:120]).reshape(20, 6), np.asarray(ter[120:124]).astype(int)
    out = []
    for k in range(4):
        x, y, z, phi, xt, yt = table[info[k]]
        Rb = D._euler_mat(xt, yt, phi)
        cz = mdl.plank_com_z
        out.append((np.array([x, y, z]) + Rb @ np.array([0, 0, -mdl.plank_half[2] - cz]) + np.array([0, 0, cz]), Rb, False))
    return out


def _swap_xy_xz(m):
    for b in range(m.n_bodies):
        m.inertia[b][3], m.inertia[b][4] = m.inertia[b][4], m.inertia[b][3]
    return m


def test_the_compiled_sample_cannot_see_an_inertia_index_swap():
    """The gap this fuzzing closes, shown in CPU code: on the compiled Walker3D blob (diagonal inertias) swapping xy <-> xz of every link
    leaves an f64-oracle substep bit-identical; on a fuzzed blob the same swap moves it far beyond any tolerance."""
    from mocca_envs_amd.vec_env import compile_model_for

    def one_substep(m, row, tau):
        o = Oracle(m.to_bytes(), 0, 1, "f64")
        o.reset(seed=0)
        o.set_state(row[None])
        o.physics_substeps(0, tau, 1)
        return o.get_state()[0]

    rng = np.random.default_rng(3)
    c = compile_model_for("Walker3DCustomEnv-v0")
    f, frng = F.case_blob("walker3d-full", 0)
    for m in (c, f):
        st, _ = F.adversarial_states(m, frng, 6)
        tau = rng.uniform(-40, 40, m.n_joints)
        a = np.stack([one_substep(m, st[i], tau) for i in range(6)])
        b = np.stack([one_substep(_swap_xy_xz(M.MoccaModel.from_bytes(m.to_bytes())), st[i], tau) for i in range(6)])
        nd = 13 + 2 * m.n_joints
        diff = np.abs(a[:, :nd] - b[:, :nd]) / (1 + np.abs(a[:, :nd]))
        print(f"\n{'compiled' if m is c else 'fuzzed'} Walker3D: xy <-> xz swap moves the substep by {diff.max():.3g} (relative)")
        if m is c:
            np.testing.assert_array_equal(a, b)
        else:
            assert diff.max() > 1e-3


def test_regression_cassie_wide_blob_3_loops_stay_assembled():
    """Regression (cassie-wide, blob 3, seed case_seed("cassie-wide", 3)): redrawn joint frames left Cassie's two loops open by 0.94 m and
    0.48 m, so the closure rows carried impulses whose fp32 rounding alone moved a joint speed by 33 units of 1e-5 (1 + |x|) under 1-ulp
    changes of the start state -- the kernel's 78 units on env 31 against a yardstick of 12 came from there, not from the kernel (the f64
    oracle agreed with the dense reference on that state).  The generator now re-places the pivots at the initial pose and keeps the loop
    joints near it: the loops close to millimetres, open to centimetres in the adversarial states, and the oracle holds to the dense
    reference on them."""
    m, rng = F.case_blob("cassie-wide", 3)
    q0 = np.array([m.init_q[b] for b in range(1, m.n_bodies)], float)
    assert max(F.closure_gaps(m, q0)) < 3e-3
    orc, st, labels, _, _ = _setup("cassie-wide", m, rng, 48)
    gaps = [max(F.closure_gaps(m, s[13:13 + m.n_joints], s[0:3], s[3:7])) for s in st]
    assert max(gaps) < 0.15, max(gaps)
    mdl = D.Model(m)
    for i in (31, 1, 7):                # env 31 (limits class) and two more limits-class states
        assert labels["limits"][i]
        info = _compare(orc, m, mdl, st[i], rng.uniform(-20, 20, m.n_joints), tol=1e-7)
        assert info["kinds"].count(3) == 6


def test_regression_cassie2d_states_stay_near_the_plane():
    """Regression (cassie2d-full, blobs 0-3): the adversarial states put the planar base up to 500 m off its plane and a quarter turn out of
    it, where the planar rows (small-angle errors of R e_y, v_y) ask for kilometres per second in one substep -- the source of the
    non-finite kernel state of one full step.  A planar base now stays within centimetres and degrees of its plane, and the three planar
    rows hold to the dense reference there."""
    for k in range(4):
        m, rng = F.case_blob("cassie2d-full", k)
        orc, st, labels, _, _ = _setup("cassie2d-full", m, rng, 24)
        assert np.abs(st[:, 1] - m.init_pos[1]).max() < 0.1
        ey = np.array([D._quat_mat(s[3:7])[:, 1] for s in st])
        assert (ey[:, 1] > 0.99).all(), ey[:, 1].min()
        if k == 0:
            mdl = D.Model(m)
            for i in (0, 3, 4):
                info = _compare(orc, m, mdl, st[i], rng.uniform(-20, 20, m.n_joints), tol=1e-7)
                assert info["n_planar"] == 3


def test_regression_cassie_termination_reads_the_foot_points():
    """Regression (cassie-full blob 3 env 55, and a dozen more samples of the four Cassie cases of tests/test_gpu_fuzz.py): the kernel's Cassie termination
    height is the base above the lower FOOT POINT (MoccaModel.foot_point, what the walkers read too), the oracle's was the base above the
    lower foot link's centre of mass.  The compiled blob puts the one on the other; a fuzzed blob moves the centre of mass, and done flags
    differed 1-2 cm from alive_height on states that agreed to 1e-7.  Here the two heights straddle alive_height: done follows the foot points."""
    m = M.compile_cassie()
    m.n_llc, m.dt = 1, 1e-5
    orc = Oracle(m.to_bytes(), M.TASK_CASSIE, 1, "f64")
    orc.reset(seed=0)
    st = orc.get_state()
    mdl = D.Model(m)
    R, o = D.fk(mdl, st[0, 0:3], D._quat_mat(st[0, 3:7]), np.concatenate([[0.0], st[0, 13:13 + m.n_joints]]))
    fb = [m.foot_body[f] for f in range(m.n_feet)]
    h_fp = st[0, 2] - min((o[b] + R[b] @ np.array(list(m.foot_point[f])))[2] for f, b in enumerate(fb))
    for dz in (0.05, -0.05):                # the feet's centres of mass 5 cm above / below their foot points (the kinematics do not change)
        for f, b in enumerate(fb):
            c = np.array(list(m.foot_point[f])) + R[b].T @ np.array([0.0, 0.0, dz])
            for k in range(3):
                m.com[b][k] = c[k]
        m.alive_height = h_fp - 0.5 * dz     # between the foot-point height and the centre-of-mass height
        orc2 = Oracle(m.to_bytes(), M.TASK_CASSIE, 1, "f64")
        orc2.reset(seed=0)
        orc2.set_state(st)
        _, _, done, _ = orc2.step(np.zeros((1, m.n_ctrl), np.float32))
        assert int(done[0] & 1) == int(not h_fp > m.alive_height), (dz, h_fp, m.alive_height, done)
