"""The terrain height scan of include/mocca.h mocca_height_scan in numpy, float64 or float32: what the HIP kernel (csrc/mocca_scan.hip) is
held to in tests/test_gpu_height_scan.py, itself held to closed forms in tests/test_height_scan.py.  The intersections, the cell height and
the plank frames are those of the ray caster's reference (tests/render_reference.py).

`scan(...)` returns (values [P], cls [P]): cls says what the vertical ray met -- CLS_NONE, CLS_GROUND, CLS_PLANK0 + k, CLS_HEIGHTFIELD
(render_reference's id codes); a hit that lies max_drop or more below the base counts as none, like the value it clamps to.
"""
from __future__ import annotations

import numpy as np

import render_reference as RR
from render_reference import SCENES, TASK_CASSIE, TASK_CUSTOM, TASK_PLANNER, TASK_STEPPER, _cell_height, euler_to_mat, hit_box, hit_cylinder, scene_records  # noqa: F401

CLS_NONE, CLS_GROUND, CLS_PLANK0, CLS_HEIGHTFIELD = RR.ID_NONE, RR.ID_GROUND, RR.ID_PLANK0, RR.ID_HEIGHTFIELD
MAX_TERRAIN_STEPS = 20

# the pattern of the comparisons: 11 x 7 points, 0.15 m apart, x from -0.45 m (ahead is +x), y centred
GRID_NX, GRID_NY, GRID_STEP, GRID_X0 = 11, 7, 0.15, -0.45
Z_ABOVE, MAX_DROP = 1.0, 2.0
EDGE_DELTA = 1e-3            # a point is excluded when the float64 class differs 1 mm away along +-x or +-y
MAX_EXCLUDED = 0.05          # ... and a scene may lose at most this share of its points
GRID_OFFSET = {}             # per scene: (dx, dy) added to the pattern, should a scene exceed the cap at (0, 0)


def comparison_grid(name=None) -> np.ndarray:
    from mocca_envs_amd.perception import scan_grid
    g = scan_grid((GRID_X0, GRID_X0 + GRID_STEP * (GRID_NX - 1)), (-GRID_STEP * (GRID_NY - 1) / 2, GRID_STEP * (GRID_NY - 1) / 2), GRID_NX, GRID_NY)
    return (g + np.asarray(GRID_OFFSET.get(name, (0.0, 0.0)), np.float32)).astype(np.float32)


def heading(q, dtype=np.float64):
    """(cos yaw, sin yaw) from the quaternion xyzw, with the branches of mocca_device.h quat_to_rp_heading"""
    dt = np.dtype(dtype).type
    x, y, z, w = (dt(v) for v in q)
    sarg = dt(-2) * (x * z - w * y)
    if sarg <= dt(-0.99999):
        yaw = dt(2) * np.arctan2(x, -y)
        return dt(np.cos(yaw)), dt(np.sin(yaw))
    if sarg >= dt(0.99999):
        yaw = dt(2) * np.arctan2(-x, y)
        return dt(np.cos(yaw)), dt(np.sin(yaw))
    A, B = dt(2) * (x * y + w * z), w * w + x * x - y * y - z * z
    n = dt(1) / np.sqrt(A * A + B * B)
    return dt(B * n), dt(A * n)


def plank_frames(model, terrain, dtype=np.float64):
    """[n_planks][12]: rotation (9, world <- plank) and centre (3) of the live planks of one env's terrain record, as
    render_reference.scene_from_records stages them"""
    dt = np.dtype(dtype).type
    ter = np.asarray(terrain, np.float32).astype(dtype)       # the device record is float32
    half2, cz = dt(model.plank_half[2]), dt(model.plank_com_z)
    dz = -half2 - cz
    out = []
    for k in range(int(model.n_planks)):
        row = int(np.clip(int(ter[6 * MAX_TERRAIN_STEPS + k]), 0, MAX_TERRAIN_STEPS - 1))
        ti = ter[6 * row:6 * row + 6]
        Rb = euler_to_mat(ti[4], ti[5], ti[3]).astype(dtype)
        out.append([*Rb, ti[0] + Rb[2] * dz, ti[1] + Rb[5] * dz, ti[2] + Rb[8] * dz + cz])
    return np.array(out, dtype).reshape(-1, 12)


def scan(state, task_id, points, z_above=Z_ABOVE, max_drop=MAX_DROP, model=None, terrain=None, hf=None, dtype=np.float64):
    """One env: `state` its state record (words 0..6 are read), `points` [P][2] float32 in the heading frame, `terrain` the env's terrain
    record and `model` the blob (Stepper), `hf` = (heights [rows][cols], scale) (planner)."""
    dt = np.dtype(dtype).type
    st = np.asarray(state, np.float32)[:7].astype(dtype)
    bx, by, bz = st[0], st[1], st[2]
    cy, sy = heading(st[3:7], dtype)
    pts = np.asarray(points, np.float32).astype(dtype)
    za, md = dt(np.float32(z_above)), dt(np.float32(max_drop))
    zs, tfar = bz + za, za + md
    planks = plank_frames(model, terrain, dtype) if task_id == TASK_STEPPER else np.zeros((0, 12), dtype)
    if task_id == TASK_STEPPER:
        half = np.asarray(model.plank_half[:], np.float32).astype(dtype)
        cylinder = int(model.plank_shape) == 1
    if task_id == TASK_PLANNER:
        hts, sc = np.asarray(hf[0], np.float32).astype(dtype), dt(np.float32(hf[1]))
        rows, cols = hts.shape
    down = np.array([[0, 0, -1]], dtype)
    vals, cls = np.zeros(len(pts), dtype), np.zeros(len(pts), np.int32)
    for p, (px, py) in enumerate(pts):
        x, y = bx + (cy * px - sy * py), by + (sy * px + cy * py)
        v, c = -md, CLS_NONE
        if task_id in (TASK_CUSTOM, TASK_CASSIE):
            v, c = dt(0) - bz, CLS_GROUND
        best = tfar
        o = np.array([x, y, zs], dtype)
        for k, P in enumerate(planks):
            lo = (o - P[9:12]) @ P[0:9].reshape(3, 3)
            if cylinder:
                inside = lo[0] * lo[0] + lo[1] * lo[1] <= half[0] * half[0] and abs(lo[2]) <= half[2]
            else:
                inside = bool((np.abs(lo) <= half).all())
            t = dt(0) if inside else (hit_cylinder if cylinder else hit_box)(o, down, P[0:9], P[9:12], half)[0]
            if t >= 0 and t < best:
                best, c = t, CLS_PLANK0 + k
        if best < tfar:
            v = (zs - best) - bz
        if task_id == TASK_PLANNER:
            gx, gy = x * sc + dt(0.5) * dt(cols - 1), y * sc + dt(0.5) * dt(rows - 1)
            if 0 <= gx <= cols - 1 and 0 <= gy <= rows - 1:
                i, j = min(int(np.floor(gx)), cols - 2), min(int(np.floor(gy)), rows - 2)
                v = dt(_cell_height(hts[j, i], hts[j, i + 1], hts[j + 1, i], hts[j + 1, i + 1], gx - dt(i), gy - dt(j))) - bz
                c = CLS_HEIGHTFIELD
        if not v > -md:          # max_drop or more below the base (or nothing at all): none
            c = CLS_NONE
        vals[p], cls[p] = min(max(v, -md), za), c
    return vals, cls


def excluded(state, task_id, points, **kw):
    """bool [P]: the float64 class differs at one of the four offsets (+-EDGE_DELTA, 0), (0, +-EDGE_DELTA) -- a plank's silhouette edge,
    where hit against miss is discontinuous"""
    pts = np.asarray(points, np.float64)
    _, c0 = scan(state, task_id, pts.astype(np.float32), dtype=np.float64, **kw)
    out = np.zeros(len(pts), bool)
    for dx, dy in ((EDGE_DELTA, 0), (-EDGE_DELTA, 0), (0, EDGE_DELTA), (0, -EDGE_DELTA)):
        _, c = scan(state, task_id, (pts + np.array([dx, dy])).astype(np.float32), dtype=np.float64, **kw)
        out |= c != c0
    return out


def scene_kwargs(model, task_id, terrain_row, hf):
    """the keyword arguments of scan() / excluded() for one env of a scene"""
    kw = {}
    if task_id == TASK_STEPPER:
        kw.update(model=model, terrain=terrain_row)
    if task_id == TASK_PLANNER:
        kw.update(hf=hf)
    return kw
