"""The terrain height scan, the part that needs no GPU: the ABI, the pattern builder, and the numpy reference (tests/height_scan_reference.py)
held to closed forms and to the validity condition of the GPU comparison (tests/test_gpu_height_scan.py)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import height_scan_reference as HS  # noqa: E402

from mocca_envs_amd import lib  # noqa: E402


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_scan_symbols():
    hdr = open(os.path.join(ROOT, "include", "mocca.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {
        "mocca_set_height_scan": r"int\s+mocca_set_height_scan\s*\(\s*mocca_handle\s+h\s*,\s*const\s+float\s*\*\s*points_host\s*,\s*int\s+n_points\s*,\s*double\s+z_above\s*,\s*double\s+max_drop\s*\)",
        "mocca_scan_dim": r"int\s+mocca_scan_dim\s*\(\s*mocca_handle\s+h\s*\)",
        "mocca_height_scan": r"int\s+mocca_height_scan\s*\(\s*mocca_handle\s+h\s*,\s*float\s*\*\s*out_dev\s*,\s*int\s+row_stride\s*,\s*const\s+float\s*\*\s*obs_dev\s*,\s*void\s*\*\s*stream\s*\)",
    }
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    sig = {"mocca_set_height_scan": (i, [vp, vp, i, d, d]), "mocca_scan_dim": (i, [vp]), "mocca_height_scan": (i, [vp, vp, i, vp, vp])}
    for name, pat in decl.items():
        assert re.search(pat, code), name + " is not declared in include/mocca.h as the binding assumes"
        assert lib.SYMBOLS[name] == sig[name]
    assert re.search(r"#define\s+MOCCA_SCAN_MAX_POINTS\s+256\b", hdr) and lib.SCAN_MAX_POINTS == 256
    assert re.search(r"#define\s+MOCCA_ABI_VERSION\s+8\b", hdr) and lib.ABI_VERSION == 8
    assert "use_egl" in hdr and "no reference counterpart" in hdr
    from mocca_envs_amd.build import build_lib
    so = build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in decl:
        assert re.search(r"\sT\s+%s$" % name, syms, re.M), name + " is not exported by the library"
    assert C.CDLL(so).mocca_abi_version() == 8


def test_intersections_are_defined_once():
    """the ray caster and the scan share one header: neither unit keeps a copy of the intersections"""
    csrc = os.path.join(ROOT, "mocca_envs_amd", "csrc")
    for fn in ("hit_box", "hit_cylinder", "cell_height", "stage_plank"):
        owners = [f for f in sorted(os.listdir(csrc)) if re.search(r"\bDI\s+\w+\s+%s\s*\(" % fn, open(os.path.join(csrc, f)).read())]
        assert owners == ["mocca_rays.h"], (fn, owners)


def test_trainer_surface_takes_the_keyword_without_a_gpu():
    from mocca_envs_amd import trainer_api
    assert "height_scan" in inspect.signature(trainer_api.TorchVecEnv.__init__).parameters
    with pytest.raises(NotImplementedError, match="terminal"):      # refused before anything touches a device
        trainer_api.TorchVecEnv("Walker3DPlannerEnv-v0", 4, terminal_observation=True, height_scan=dict(points=[[0.0, 0.0]]))
    with pytest.raises(NotImplementedError, match="sub_batches"):
        trainer_api.TorchVecEnv("Walker3DPlannerEnv-v0", 4, sub_batches=2, height_scan=dict(points=[[0.0, 0.0]]))


# ---- the pattern builder -----------------------------------------------------------------------------------------------------------
def test_scan_grid_order_and_shape():
    from mocca_envs_amd.perception import scan_grid
    g = scan_grid((-0.45, 1.05), (-0.45, 0.45), 11, 7)
    assert g.shape == (77, 2) and g.dtype == np.float32
    xs, ys = np.linspace(-0.45, 1.05, 11), np.linspace(-0.45, 0.45, 7)
    for ix in (0, 3, 10):
        for iy in (0, 2, 6):
            assert np.allclose(g[ix * 7 + iy], (xs[ix], ys[iy]), atol=1e-7)       # x-major: x ahead, then y to the left
    assert np.allclose(np.diff(g.reshape(11, 7, 2)[:, 0, 0]), 0.15, atol=1e-6) and np.allclose(np.diff(g.reshape(11, 7, 2)[0, :, 1]), 0.15, atol=1e-6)
    assert scan_grid((0.2, 0.9), (0.1, 0.5), 1, 1).tolist() == [[np.float32(0.2), np.float32(0.1)]]
    assert np.allclose(HS.comparison_grid(), g, atol=1e-6)
    for bad in ((0, 3), (3, 0), (17, 16)):
        with pytest.raises(ValueError):
            scan_grid((0, 1), (0, 1), *bad)


# ---- the reference against closed forms --------------------------------------------------------------------------------------------
def _quat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]   # xyzw


def _state(pos, rpy=(0, 0, 0)):
    return np.array([*pos, *_quat(*rpy)], np.float64)


def _plank_model(half, shape=0, com_z=0.0):
    return SimpleNamespace(plank_half=list(half), plank_com_z=com_z, plank_shape=shape, n_planks=1)


def _terrain(x, y, z, yaw=0.0, roll=0.0, pitch=0.0):
    ter = np.zeros(128)
    ter[0:6] = x, y, z, yaw, roll, pitch       # the row layout render_reference.scene_from_records reads: position, then yaw, roll, pitch
    ter[120] = 0
    return ter


def test_heading_matches_the_yaw_of_a_tilted_base():
    for yaw in (-2.5, -0.3, 0.0, 1.1, 3.0):
        for dt in (np.float64, np.float32):
            cy, sy = HS.heading(_quat(0.2, -0.15, yaw), dt)
            assert abs(cy - np.cos(yaw)) < 1e-6 and abs(sy - np.sin(yaw)) < 1e-6
    cy, sy = HS.heading(_quat(0.0, np.pi / 2, 0.4), np.float64)      # the gimbal branch: still a unit vector
    assert abs(cy * cy + sy * sy - 1) < 1e-12


def test_flat_ground_gives_minus_base_z():
    pts = HS.comparison_grid()
    for task in (HS.TASK_CUSTOM, HS.TASK_CASSIE):
        for dt in (np.float64, np.float32):
            v, c = HS.scan(_state((3.0, -2.0, 1.25), (0.3, -0.2, 0.7)), task, pts, dtype=dt)
            assert (v == -1.25).all() and (c == HS.CLS_GROUND).all()
    v, c = HS.scan(_state((0, 0, 2.5)), HS.TASK_CUSTOM, pts)            # further below than max_drop: nothing, and the clamp
    assert (v == -HS.MAX_DROP).all() and (c == HS.CLS_NONE).all()
    v, c = HS.scan(_state((0, 0, -1.5)), HS.TASK_CUSTOM, pts)           # the start point lies under the surface: saturates at +z_above
    assert (v == HS.Z_ABOVE).all() and (c == HS.CLS_GROUND).all()
    assert not HS.excluded(_state((0, 0, 1.0)), HS.TASK_CUSTOM, pts).any()


def test_tilted_box_top_face_is_its_plane():
    half, pos = (0.6, 0.5, 0.1), np.array([0.4, 0.1, 0.3])
    yaw, roll, pitch = 0.5, 0.12, -0.2
    model, ter = _plank_model(half), _terrain(*pos, yaw, roll, pitch)
    R = HS.euler_to_mat(roll, pitch, yaw).reshape(3, 3)
    n, top = R[:, 2], pos + R[:, 2] * 0.0      # the record's position is the centre of the TOP face (com_z = 0: centre = pos - n * half_z)
    base = _state((0.3, 0.0, 1.0), (0.05, 0.1, -0.4))
    pts = np.array([[0.0, 0.0], [0.15, 0.1], [-0.1, 0.2], [0.3, -0.15]], np.float32)
    v, c = HS.scan(base, HS.TASK_STEPPER, pts, model=model, terrain=ter)
    cy, sy = np.cos(-0.4), np.sin(-0.4)
    for (px, py), got, cls in zip(pts.astype(np.float64), v, c):
        x, y = 0.3 + cy * px - sy * py, 0.0 + sy * px + cy * py
        z = top[2] - (n[0] * (x - top[0]) + n[1] * (y - top[1])) / n[2]
        assert cls == HS.CLS_PLANK0 and abs(got - (z - 1.0)) < 1e-6, (px, py, got, z - 1.0)
    v32, _ = HS.scan(base, HS.TASK_STEPPER, pts, model=model, terrain=ter, dtype=np.float32)
    assert np.abs(v32 - v).max() < 1e-5
    far = np.array([[5.0, 5.0]], np.float32)                             # beside the plank there is no ground
    v, c = HS.scan(base, HS.TASK_STEPPER, far, model=model, terrain=ter)
    assert v[0] == -HS.MAX_DROP and c[0] == HS.CLS_NONE
    inside = _state((0.4, 0.1, 0.25 - HS.Z_ABOVE))                       # the ray starts inside the slab: saturates
    v, c = HS.scan(inside, HS.TASK_STEPPER, np.zeros((1, 2), np.float32), model=model, terrain=ter)
    assert v[0] == HS.Z_ABOVE and c[0] == HS.CLS_PLANK0


def test_cylinder_cap_is_its_height_and_its_rim_is_excluded():
    model, ter = _plank_model((0.25, 0.25, 0.4), shape=1), _terrain(1.0, 0.5, 0.2)
    base = _state((1.0, 0.5, 0.9), (0, 0, 1.3))
    pts = np.array([[0.0, 0.0], [0.1, -0.1], [0.2495, 0.0], [0.3, 0.0]], np.float32)
    v, c = HS.scan(base, HS.TASK_STEPPER, pts, model=model, terrain=ter)
    assert np.allclose(v[:3], 0.2 - 0.9, atol=1e-12) and (c[:3] == HS.CLS_PLANK0).all()      # the cap: the record's z
    assert v[3] == -HS.MAX_DROP and c[3] == HS.CLS_NONE
    assert HS.excluded(base, HS.TASK_STEPPER, pts, model=model, terrain=ter).tolist() == [False, False, True, False]


def test_height_field_cell_is_interpolated_and_continuous():
    rng = np.random.default_rng(0)
    hts, scale = rng.uniform(-0.3, 0.3, (9, 11)).astype(np.float32), 4.0
    hf = (hts, scale)
    base = _state((0.0, 0.0, 1.0))
    # grid vertex (i, j) sits at ((i - 5) / 4, (j - 4) / 4): at a vertex the scan is that height
    pts = np.array([[(i - 5) / 4, (j - 4) / 4] for i in (2, 5, 9) for j in (1, 4, 7)], np.float32)
    v, c = HS.scan(base, HS.TASK_PLANNER, pts, hf=hf)
    want = np.array([hts[j, i] for i in (2, 5, 9) for j in (1, 4, 7)], np.float64) - 1.0
    assert np.allclose(v, want, atol=1e-12) and (c == HS.CLS_HEIGHTFIELD).all()
    # on the diagonal of cell (5, 4) -- from vertex (6, 4) to (5, 5) -- the surface is the mean of those two
    v, _ = HS.scan(base, HS.TASK_PLANNER, np.array([[0.125, 0.125]], np.float32), hf=hf)
    assert abs(v[0] - (0.5 * (float(hts[4, 6]) + float(hts[5, 5])) - 1.0)) < 1e-12
    # continuous across the diagonal and across cell borders; outside the grid: nothing
    for a, b in (((0.1249, 0.1249), (0.1251, 0.1251)), ((0.2499, 0.1), (0.2501, 0.1)), ((0.1, 0.4999), (0.1, 0.5001))):
        va, _ = HS.scan(base, HS.TASK_PLANNER, np.array([a, b], np.float32), hf=hf)
        assert abs(va[0] - va[1]) < 5e-3
    v, c = HS.scan(base, HS.TASK_PLANNER, np.array([[1.3, 0.0], [0.0, -1.01]], np.float32), hf=hf)
    assert (v == -HS.MAX_DROP).all() and (c == HS.CLS_NONE).all()


# ---- the validity condition of the GPU comparison ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HS.SCENES))
def test_scenes_exclude_at_most_five_percent(name):
    """Over the committed scenes and the comparison grid the float64 reference alone decides which points are excluded (the class differs
    1 mm away: a plank's silhouette edge); a scene may lose at most 5 % of its points, so the comparison stays a comparison."""
    model, task_id, kw, st, tk, ter, hf = HS.scene_records(name)
    pts = HS.comparison_grid(name)
    lost, seen = 0, 0
    for e in range(st.shape[0]):
        skw = HS.scene_kwargs(model, task_id, ter[e], hf)
        ex = HS.excluded(st[e], task_id, pts, **skw)
        _, cls = HS.scan(st[e], task_id, pts, **skw)
        lost, seen = lost + int(ex.sum()), seen + len(pts)
        print(name, "env", e, "excluded", int(ex.sum()), "of", len(pts), "classes", sorted(set(cls.tolist())))
        if task_id != HS.TASK_STEPPER:
            assert not ex.any()          # the plane and the height field are continuous: nothing is excluded
    assert lost <= HS.MAX_EXCLUDED * seen, (name, lost, seen)


# ---- the synthetic scenes: rotated live planks, the hills, the border, outside the grid -------------------------------------------
def _scan_cases():
    return [(n, c) for n in HS.PLANK_SCENES for c in HS.PLANK_CASES] + [("planner", c) for c in HS.PLANNER_CASES]


@pytest.mark.parametrize("name,case", _scan_cases())
def test_synthetic_scan_scenes_exclude_at_most_five_percent(name, case):
    """the cap of the committed scenes, unchanged, on every synthetic scene and pattern; and each case shows what it is there for"""
    model, task_id, kw, st, tk, ter, hf = HS.synthetic_scan_records(name, case)
    pat, za, md = (HS.PLANNER_CASES if name == "planner" else HS.PLANK_CASES)[case]
    pts = HS.synthetic_pattern(name, case)
    lost = seen = sat = none = hit = 0
    for e in range(st.shape[0]):
        skw = HS.scene_kwargs(model, task_id, ter[e], hf)
        ex = HS.excluded(st[e], task_id, pts, z_above=za, max_drop=md, **skw)
        v, c = HS.scan(st[e], task_id, pts, z_above=za, max_drop=md, **skw)
        keep = ~ex
        lost, seen = lost + int(ex.sum()), seen + len(pts)
        sat, none, hit = sat + int((v == np.float64(np.float32(za)))[keep].sum()), none + int((c == HS.CLS_NONE)[keep].sum()), hit + int((c != HS.CLS_NONE)[keep].sum())
    print(name, case, "excluded", lost, "of", seen, "saturated", sat, "none", none, "hit", hit)
    assert lost <= HS.MAX_EXCLUDED * seen, (name, case, lost, seen)
    assert hit >= 0.1 * seen
    if case in ("inside", "short_drop"):
        assert sat > 0                       # rays that start inside a solid / under the surface
    if case in ("short_drop", "wide_256", "dense_256"):
        assert none > 0.1 * seen and len(pts) == 256


def test_scan_reference_equals_the_vertical_brute_force():
    """height_scan_reference.scan on the planner bases (hills, border, outside, low) against the vertical brute-force ray over every
    triangle near the point: hit / miss equal on every kept point, heights within 1e-12 m (measured: 8.9e-16)."""
    model, task_id, kw, st, tk, ter, hf = HS.synthetic_scan_records("planner", "wide_256")
    worst, top = 0.0, float(np.max(hf[0])) + 1.0
    for pat, za, md in (HS.PLANNER_CASES["grid"], HS.PLANNER_CASES["wide_256"]):
        pts = pat()
        for e in range(st.shape[0]):
            v, c = HS.scan(st[e], task_id, pts, z_above=za, max_drop=md, hf=hf)
            keep = ~HS.excluded(st[e], task_id, pts, z_above=za, max_drop=md, hf=hf)
            cy, sy = HS.heading(st[e, 3:7].astype(np.float64))
            b = st[e, 0:3].astype(np.float64)
            for p in np.nonzero(keep)[0]:
                px, py = pts[p].astype(np.float64)
                z = HS.RR.drop_heightfield_brute(b[0] + cy * px - sy * py, b[1] + sy * px + cy * py, top, hf[0], hf[1], 1e3)      # from above the highest vertex: a height field has one surface
                seen = z is not None and z - b[2] > -md
                assert seen == (c[p] == HS.CLS_HEIGHTFIELD), (e, p)
                if seen:
                    worst = max(worst, abs(min(z - b[2], float(np.float32(za))) - v[p]))
    print("scan vs vertical brute force: largest difference", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("name,mutation", [(n, m) for n in HS.PLANK_SCENES for m in HS.RR.PLANK_MUTATIONS] + [("planner", m) for m in HS.RR.HF_MUTATIONS])
def test_the_scan_rule_rejects_a_mutated_reference(name, mutation):
    """the float32 reference of the true scene passes the GPU comparison's rule (4 x e32 + 1 ulp on kept points) against the right float64
    reference in every env, and fails it against one with a wrong plank frame / the other cell split in EVERY env whose pattern sees
    terrain at all (the planner's env outside the grid sees none)"""
    model, task_id, kw, st, tk, ter, hf = HS.synthetic_scan_records(name, "grid")
    pts = HS.synthetic_pattern(name, "grid")
    for e in range(st.shape[0]):
        skw = HS.scene_kwargs(model, task_id, ter[e], hf)
        got, _ = HS.scan(st[e], task_id, pts, dtype=np.float32, **skw)
        assert HS.accepts(got, st[e], task_id, pts, **skw)[0], (name, e)
        if HS.sees_terrain(st[e], task_id, pts, **skw):
            ok, fig = HS.accepts(got, st[e], task_id, pts, mutate=mutation, **skw)
            assert not ok, (name, mutation, e, fig)
        else:
            assert name == "planner" and e == HS.RR.PLANNER_ENV_OF["outside"]
