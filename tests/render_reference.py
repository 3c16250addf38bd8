"""A numpy ray caster over the primitive list of include/mocca.h mocca_render, in float64 or float32: the reference the GPU ray
caster is held to (tests/test_gpu_render.py), itself held to analytic cases (tests/test_render.py).

A scene is a dict:
  prims   [P][9]: p1 (3), p2 (3), radius, id, kind (0 sphere, 1 capsule)     robot geoms and the target marker, world space
  planks  [K][12]: rotation (9, world <- plank), centre (3); plank_half (3), plank_shape (0 box, 1 upright cylinder)
  ground  bool: the plane z = 0
  hf      None or (heights [rows][cols], scale): vertex (i, j) at ((i - (cols - 1) / 2) / scale, (j - (rows - 1) / 2) / scale), every
          cell split from (i + 1, j) to (i, j + 1)
`render(scene, camera, W, H, dtype)` returns (depth [H][W], id [H][W]) with the header's pixel-centre convention.
"""
from __future__ import annotations

import numpy as np

ID_NONE, ID_GROUND, ID_PLANK0, ID_HEIGHTFIELD, ID_TARGET, ID_LINK0 = -1, 32, 33, 37, 38, 64
SKELETON_RADIUS, MAX_PRIMS = 0.04, 33


def is_robot(ids):
    """pixels that show the robot: a geom, or a link of a skeleton"""
    return ((ids >= 0) & (ids < 32)) | (ids >= ID_LINK0)
TASK_CUSTOM, TASK_STEPPER, TASK_CASSIE, TASK_PLANNER = 0, 1, 2, 3


def rays(camera, W, H, dtype):
    cam = np.asarray(camera, dtype)
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    half = dtype(0.5)
    sx = (dtype(2) * (i.astype(dtype) + half) / dtype(W) - dtype(1)) * cam[12] * cam[13]
    sy = (dtype(1) - dtype(2) * (j.astype(dtype) + half) / dtype(H)) * cam[12]
    d = cam[9:12] + sx[..., None] * cam[3:6] + sy[..., None] * cam[6:9]
    return cam[0:3], d.astype(dtype)


def _dot(a, b):
    return (a * b).sum(-1)


def hit_sphere(o, d, c, r):
    """entry parameter per ray, -1 for a miss"""
    oc = o - c
    dd, b, cc = _dot(d, d), _dot(d, oc), _dot(oc, oc) - r * r
    h = b * b - dd * cc
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(np.maximum(h, 0))) / dd
    return np.where(h < 0, -1, t).astype(d.dtype)


def hit_tube(o, d, pa, pb, r):
    ba, oa = pb - pa, o - pa
    dd, baba = _dot(d, d), _dot(ba, ba)
    bard, baoa, rdoa, oaoa = _dot(d, ba), _dot(ba, oa), _dot(d, oa), _dot(oa, oa)
    A, B, C = baba * dd - bard * bard, baba * rdoa - baoa * bard, baba * oaoa - baoa * baoa - r * r * baba
    h = B * B - A * C
    ok = (A > 1e-12 * baba * dd) & (h >= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-B - np.sqrt(np.maximum(h, 0))) / np.where(ok, A, 1)
    y = baoa + t * bard
    return np.where(ok & (y > 0) & (y < baba), t, -1).astype(d.dtype)


def hit_capsule(o, d, pa, pb, r):
    best = hit_sphere(o, d, pa, r)
    for t in (hit_sphere(o, d, pb, r), hit_tube(o, d, pa, pb, r)):
        best = np.where((t >= 0) & ((best < 0) | (t < best)), t, best)
    return best


def _local(o, d, R, c):
    R = R.reshape(3, 3)
    return (o - c) @ R, d @ R      # R^T applied to row vectors


def hit_box(o, d, R, c, half):
    lo, ld = _local(o, d, R, c)
    t0 = np.full(d.shape[:-1], -1e30, d.dtype)
    t1 = np.full(d.shape[:-1], 1e30, d.dtype)
    miss = np.zeros(d.shape[:-1], bool)
    for k in range(3):
        par = np.abs(ld[..., k]) < 1e-20
        miss |= par & (np.abs(lo[k]) > half[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1 / np.where(par, 1, ld[..., k])
        ta, tb = (-half[k] - lo[k]) * inv, (half[k] - lo[k]) * inv
        ta, tb = np.minimum(ta, tb), np.maximum(ta, tb)
        t0 = np.where(par, t0, np.maximum(t0, ta))
        t1 = np.where(par, t1, np.minimum(t1, tb))
    return np.where(miss | (t0 > t1), -1, t0).astype(d.dtype)


def hit_cylinder(o, d, R, c, half):
    lo, ld = _local(o, d, R, c)
    rad, hz = half[0], half[2]
    A, B, C = ld[..., 0] ** 2 + ld[..., 1] ** 2, lo[0] * ld[..., 0] + lo[1] * ld[..., 1], lo[0] ** 2 + lo[1] ** 2 - rad * rad
    disc = B * B - A * C
    ok = (A > 1e-20) & (disc >= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-B - np.sqrt(np.maximum(disc, 0))) / np.where(ok, A, 1)
    best = np.where(ok & (np.abs(lo[2] + t * ld[..., 2]) <= hz), t, -1)
    okc = np.abs(ld[..., 2]) > 1e-20
    with np.errstate(invalid="ignore", divide="ignore"):
        tc = (np.where(ld[..., 2] < 0, hz, -hz) - lo[2]) / np.where(okc, ld[..., 2], 1)
    px, py = lo[0] + tc * ld[..., 0], lo[1] + tc * ld[..., 1]
    cap = okc & (px * px + py * py <= rad * rad)
    best = np.where(cap & ((best < 0) | (tc < best)), tc, best)
    return best.astype(d.dtype)


def _cell_height(h00, h10, h01, h11, u, v):
    return np.where(u + v <= 1, h00 + u * (h10 - h00) + v * (h01 - h00), h11 + (1 - u) * (h01 - h11) + (1 - v) * (h10 - h11))


def hit_heightfield(o, d, heights, scale, tnear, tfar):
    """The march of mocca_render.hip hit_heightfield, over all rays at once: g(t) = z(t) - height(x(t), y(t)) is sampled at every
    cell's entry, diagonal crossing and exit; the first sign change is the hit."""
    dt = d.dtype.type
    shape = d.shape[:-1]
    hts = np.asarray(heights, d.dtype)
    rows, cols = hts.shape
    sc = dt(scale)
    hx, hy = dt(0.5 * (cols - 1)), dt(0.5 * (rows - 1))
    ox, oy, oz = o[0] * sc + hx, o[1] * sc + hy, o[2]
    dx, dy, dz = d[..., 0] * sc, d[..., 1] * sc, d[..., 2]
    zmin, zmax = hts.min(), hts.max()
    zpad = dt(1e-3) * (zmax - zmin) + dt(1e-4)
    ta = np.broadcast_to(np.asarray(tnear, d.dtype), shape).copy()
    tb = np.broadcast_to(np.asarray(tfar, d.dtype), shape).copy()
    alive = np.ones(shape, bool)
    for o3, d3, lo, hi in ((ox, dx, dt(0), dt(cols - 1)), (oy, dy, dt(0), dt(rows - 1)), (oz, dz, zmin - zpad, zmax + zpad)):
        par = np.abs(d3) < 1e-20
        alive &= ~(par & ((o3 < lo) | (o3 > hi)))
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1 / np.where(par, 1, d3)
        t0, t1 = (lo - o3) * inv, (hi - o3) * inv
        t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)
        ta = np.where(par, ta, np.maximum(ta, t0))
        tb = np.where(par, tb, np.minimum(tb, t1))
    alive &= ta <= tb
    tm0 = ta + dt(1e-4) * (tb - ta)
    ci, cj = cols - 2, rows - 2
    with np.errstate(invalid="ignore"):
        i = np.clip(np.floor(np.where(alive, ox + tm0 * dx, 0)), 0, ci).astype(np.int64)
        j = np.clip(np.floor(np.where(alive, oy + tm0 * dy, 0)), 0, cj).astype(np.int64)
    si, sj = np.where(dx > 0, 1, -1), np.where(dy > 0, 1, -1)
    nzx, nzy = np.abs(dx) > 1e-20, np.abs(dy) > 1e-20
    with np.errstate(divide="ignore", invalid="ignore"):
        idx, idy = 1 / np.where(nzx, dx, 1), 1 / np.where(nzy, dy, 1)
    t0 = ta.copy()
    gprev = np.zeros(shape, d.dtype)
    have = np.zeros(shape, bool)
    out = np.full(shape, -1, d.dtype)
    big = dt(1e30)
    for _ in range(cols + rows - 1):
        if not alive.any():
            break
        tx = np.where(nzx, (np.where(dx > 0, i + 1, i).astype(d.dtype) - ox) * idx, big)
        ty = np.where(nzy, (np.where(dy > 0, j + 1, j).astype(d.dtype) - oy) * idy, big)
        t1 = np.maximum(np.minimum(np.minimum(tx, ty), tb), t0)
        h00, h10, h01, h11 = hts[j, i], hts[j, i + 1], hts[j + 1, i], hts[j + 1, i + 1]
        z0, z1 = oz + t0 * dz, oz + t1 * dz
        fi, fj = i.astype(d.dtype), j.astype(d.dtype)
        u0, v0, u1, v1 = ox + t0 * dx - fi, oy + t0 * dy - fj, ox + t1 * dx - fi, oy + t1 * dy - fj
        s0, s1 = u0 + v0, u1 + v1
        g0 = z0 - _cell_height(h00, h10, h01, h11, u0, v0)
        g1 = z1 - _cell_height(h00, h10, h01, h11, u1, v1)
        cross = ((s0 < 1) != (s1 < 1)) & (s0 != s1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tm = t0 + (1 - s0) / np.where(cross, s1 - s0, 1) * (t1 - t0)
        tm = np.where(cross, np.minimum(np.maximum(tm, t0), t1), t1)
        um, vm = ox + tm * dx - fi, oy + tm * dy - fj
        gm = np.where(cross, oz + tm * dz - (h00 + um * (h10 - h00) + vm * (h01 - h00)), g1)
        tp, gp = t0, np.where(have, gprev, g0)
        found = np.zeros(shape, bool)
        for tk, gk in ((t0, g0), (tm, gm), (t1, g1)):
            flip = alive & ~found & ((gp > 0) != (gk > 0))
            den = gp - gk
            with np.errstate(divide="ignore", invalid="ignore"):
                th = np.where(den != 0, tp + gp / np.where(den != 0, den, 1) * (tk - tp), tp)
            out = np.where(flip, th, out)
            found |= flip
            tp, gp = tk, gk
        have |= alive
        gprev = np.where(alive, gp, gprev)
        alive &= ~found
        alive &= ~(t1 >= tb)
        stepx = tx <= ty
        i = np.where(alive & stepx, i + si, i)
        j = np.where(alive & ~stepx, j + sj, j)
        alive &= (i >= 0) & (i <= ci) & (j >= 0) & (j <= cj)
        i, j = np.clip(i, 0, ci), np.clip(j, 0, cj)
        t0 = np.where(alive, t1, t0)
    return out


def render(scene, camera, W, H, dtype=np.float64):
    dtype = np.dtype(dtype).type
    o, d = rays(camera, W, H, dtype)
    cam = np.asarray(camera, dtype)
    tnear, tfar = cam[14], cam[15]
    best = np.full((H, W), tfar, dtype)
    ids = np.full((H, W), ID_NONE, np.int32)

    def take(t, code):
        nonlocal best, ids
        m = (t >= tnear) & (t < best)
        best = np.where(m, t, best).astype(dtype)
        ids = np.where(m, code, ids).astype(np.int32)

    for p in np.asarray(scene["prims"], np.float64).reshape(-1, 9):
        pa, pb, r = p[0:3].astype(dtype), p[3:6].astype(dtype), dtype(p[6])
        take(hit_capsule(o, d, pa, pb, r) if int(p[8]) else hit_sphere(o, d, pa, r), int(p[7]))
    half = np.asarray(scene.get("plank_half", (0, 0, 0)), dtype)
    for k, p in enumerate(np.asarray(scene.get("planks", ()), np.float64).reshape(-1, 12)):
        fn = hit_cylinder if scene.get("plank_shape", 0) == 1 else hit_box
        take(fn(o, d, p[0:9].astype(dtype), p[9:12].astype(dtype), half), ID_PLANK0 + k)
    if scene.get("ground"):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where((d[..., 2] < 0) & (o[2] > 0), -o[2] / np.where(d[..., 2] < 0, d[..., 2], -1), -1).astype(dtype)
        take(t, ID_GROUND)
    if scene.get("hf") is not None:
        take(hit_heightfield(o, d, scene["hf"][0], scene["hf"][1], tnear, best), ID_HEIGHTFIELD)
    return best, ids


def edge_mask(ids):
    """pixels whose 3 x 3 neighbourhood in the id image is not uniform (the image border compares with itself)"""
    p = np.pad(ids, 1, mode="edge")
    H, W = ids.shape
    e = np.zeros(ids.shape, bool)
    for dj in range(3):
        for di in range(3):
            e |= p[dj:dj + H, di:di + W] != ids
    return e


def euler_to_mat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                     -sp, cp * sr, cp * cr])


def scene_from_records(model, task_id, frames, walk_target, terrain=None, hf=None):
    """The primitive list of one env: `frames` [n_bodies][15] (the oracle's link_frames), walk_target (3), terrain the env's record
    (20 rows of 6, then the live planks' rows) for the Stepper, hf = (heights, scale) for the planner envs."""
    fr = np.asarray(frames, np.float64)
    prims = []
    nb = model.n_bodies
    if any(model.g_radius[g] > 0 for g in range(model.n_geoms)):
        for g in range(model.n_geoms):
            b = model.g_body[g]
            R, org = fr[b, 0:9].reshape(3, 3), fr[b, 9:12]
            p1 = R @ np.array(model.g_p1[g][:], np.float64) + org
            p2 = R @ np.array(model.g_p2[g][:], np.float64) + org
            prims.append([*p1, *p2, model.g_radius[g], g, 1 if model.g_type[g] == 1 else 0])
    else:   # every geom is a point: the skeleton (include/mocca.h mocca_render)
        for b in range(1, nb):
            prims.append([*fr[model.parent[b], 9:12], *fr[b, 9:12], SKELETON_RADIUS, ID_LINK0 + b, 1])
        for b in range(1, nb):
            if not any(model.parent[c] == b for c in range(1, nb)):
                prims.append([*fr[b, 9:12], *(2 * fr[b, 12:15] - fr[b, 9:12]), SKELETON_RADIUS, ID_LINK0 + b, 1])
        prims = prims[:MAX_PRIMS - 1]
    if task_id != TASK_CASSIE:
        wt = np.asarray(walk_target, np.float64)
        prims.append([*wt, *wt, 0.15, ID_TARGET, 0])
    scene = dict(prims=np.array(prims), ground=task_id in (TASK_CUSTOM, TASK_CASSIE), hf=hf if task_id == TASK_PLANNER else None)
    if task_id == TASK_STEPPER:
        ter = np.asarray(terrain, np.float64)
        half = np.array(model.plank_half[:], np.float64)
        cz = float(model.plank_com_z)
        dz = -half[2] - cz
        planks = []
        for k in range(model.n_planks):
            ti = ter[6 * int(ter[120 + k]):][:6]
            Rb = euler_to_mat(ti[4], ti[5], ti[3])
            planks.append([*Rb, ti[0] + Rb[2] * dz, ti[1] + Rb[5] * dz, ti[2] + Rb[8] * dz + cz])
        scene.update(planks=np.array(planks), plank_half=half, plank_shape=int(model.plank_shape))
    return scene


# ---- the scenes of the GPU comparison: states come from the CPU oracle (float32 physics, a seed), so the CPU tests can hold the reference
# ---- to the validity conditions of the comparison without a GPU ----
SCENES = {
    "custom": ("Walker3DCustomEnv-v0", TASK_CUSTOM, {}),
    "stepper_box": ("Walker3DStepperEnv-v0", TASK_STEPPER, {}),
    "stepper_pillar": ("Walker3DStepperEnv-v0", TASK_STEPPER, {"plank_class": "Pillar"}),
    "mikeplanner": ("MikePlannerEnv-v0", TASK_PLANNER, {}),
    "cassie": ("CassieEnv-v0", TASK_CASSIE, {}),
}
RESOLUTIONS = ((160, 120), (320, 240))
SCENE_ENVS, SCENE_ENV, SCENE_SEED, SCENE_STEPS = 2, 1, 7, 5


def scene_cameras(base_pos, aspect):
    """the follow camera (yaw 0, pitch -5, looking at the base) and one fixed oblique camera; both closer than the gym classes' 2.5 m,
    so that at 160 x 120 even Cassie's thin skeleton still fills 2 % of the image away from its outlines"""
    from mocca_envs_amd.render import Camera
    follow, oblique = Camera(dist=1.5), Camera(yaw=40.0, pitch=-30.0, dist=1.3)
    follow.lookat(base_pos)
    oblique.lookat(base_pos)
    return {"follow": follow.pack(aspect), "oblique": oblique.pack(aspect)}


def scene_records(name):
    """(model, task_id, model_kw, state f32 [n][state_dim], task f64 [n][40] in the oracle's layout, terrain f64 [n][124], hf or None) after
    SCENE_STEPS random-action steps of the float32 oracle from reset(SCENE_SEED)"""
    from mocca_envs_amd.vec_env import compile_model_for
    from oracle.oracle import Oracle
    env_id, task_id, kw = SCENES[name]
    model = compile_model_for(env_id, **kw)
    orc = Oracle(model.to_bytes(), task_id, SCENE_ENVS, "f32")
    hf = None
    if task_id == TASK_PLANNER:
        from mocca_envs_amd.terrain import load_height_field
        hf = load_height_field()
        orc.set_heightfield(*hf)
    orc.reset(seed=SCENE_SEED)
    rng = np.random.default_rng(SCENE_SEED)
    for _ in range(SCENE_STEPS):
        orc.step(rng.uniform(-1, 1, (SCENE_ENVS, orc.act_dim)).astype(np.float32))
    return model, task_id, kw, orc.get_state().astype(np.float32), orc.get_task(), orc.get_terrain(), hf


def reference_scene(model, task_id, state32, task, terrain, hf, env=SCENE_ENV):
    """the float64 primitive list of env `env`: link frames from the float64 oracle on the float32 state"""
    from oracle.oracle import Oracle
    o64 = Oracle(model.to_bytes(), task_id, state32.shape[0], "f64")
    if hf is not None:
        o64.set_heightfield(*hf)
    o64.set_state(state32.astype(np.float64))
    frames = o64.link_frames(env, model.n_bodies)
    return scene_from_records(model, task_id, frames, np.asarray(task[env, 0:3], np.float32), terrain[env], hf)
