"""A numpy ray caster over the primitive list of include/mocca.h mocca_render, in float64 or float32: the reference the GPU ray
caster is held to (tests/test_gpu_render.py), itself held to analytic cases and, for the height-field march, to a brute-force float64
ray / triangle test over the whole field (hit_heightfield_brute; tests/test_render.py).

A scene is a dict:
  prims   [P][9]: p1 (3), p2 (3), radius, id, kind (0 sphere, 1 capsule)     robot geoms and the target marker, world space
  planks  [K][12]: rotation (9, world <- plank), centre (3); plank_half (3), plank_shape (0 box, 1 upright cylinder)
  ground  bool: the plane z = 0
  hf      None or (heights [rows][cols], scale): vertex (i, j) at ((i - (cols - 1) / 2) / scale, (j - (rows - 1) / 2) / scale), every
          cell split from (i + 1, j) to (i, j + 1)
  prim_rgb optional [P][3]: base colour per prim (scene_from_records fills it from the palette)
`render(scene, camera, W, H, dtype)` returns (depth [H][W], id [H][W]) with the header's pixel-centre convention; with shading=True a
third value, a dict: normal [H][W][3] (unit, world), part [H][W] (which face / cap / triangle / checker square / capsule part was hit,
PART_* below) and colour [H][W][3], the UNROUNDED base x (0.35 + 0.65 max(0, n . l)) x 255 of include/mocca.h.
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


def hit_heightfield_brute(o, d, heights, scale, tnear, tfar, other_diagonal=False, return_triangle=False):
    """Nearest hit of every ray with EVERY triangle of the documented split (cell (i, j): (i, j) (i + 1, j) (i, j + 1) and (i + 1, j + 1)
    (i, j + 1) (i + 1, j); other_diagonal: the split from (i, j) to (i + 1, j + 1) instead), Moeller-Trumbore in float64 whatever the
    inputs' type.  No cell walk, no entry nudge, nothing shared with hit_heightfield: the only economy is that a ray is tested against
    the triangles of the cells under the xy bounding box of its segment [tnear, tfar] (grown by a cell), which leaves no triangle out
    that the segment could touch.  Entry parameter per ray, -1 for a miss (tnear <= t < tfar, as render() takes hits); with
    return_triangle also the triangle 2 (j (cols - 1) + i) + (0 lower, 1 upper), -1 for a miss."""
    o = np.asarray(o, np.float64)
    dirs = np.asarray(d, np.float64)
    shape = dirs.shape[:-1]
    dirs = dirs.reshape(-1, 3)
    hts = np.asarray(heights, np.float64)
    rows, cols = hts.shape
    sc = float(scale)
    X, Y = (np.arange(cols) - 0.5 * (cols - 1)) / sc, (np.arange(rows) - 0.5 * (rows - 1)) / sc
    tn = np.broadcast_to(np.asarray(tnear, np.float64), shape).reshape(-1)
    tf = np.broadcast_to(np.asarray(tfar, np.float64), shape).reshape(-1)
    out, tri = np.full(len(dirs), -1.0), np.full(len(dirs), -1, np.int64)
    for r, dr in enumerate(dirs):
        xa, xb = sorted((o[0] + tn[r] * dr[0], o[0] + tf[r] * dr[0]))
        ya, yb = sorted((o[1] + tn[r] * dr[1], o[1] + tf[r] * dr[1]))
        if not (xb >= X[0] and xa <= X[-1] and yb >= Y[0] and ya <= Y[-1]):
            continue
        i0, i1 = max(int(np.searchsorted(X, xa)) - 2, 0), min(int(np.searchsorted(X, xb)) + 1, cols - 2)
        j0, j1 = max(int(np.searchsorted(Y, ya)) - 2, 0), min(int(np.searchsorted(Y, yb)) + 1, rows - 2)
        I, J = (a.ravel() for a in np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1)))
        V = lambda ii, jj: np.stack([X[ii], Y[jj], hts[jj, ii]], -1)
        v00, v10, v01, v11 = V(I, J), V(I + 1, J), V(I, J + 1), V(I + 1, J + 1)
        if other_diagonal:
            A, B, C = np.concatenate([v00, v11]), np.concatenate([v10, v01]), np.concatenate([v11, v00])
        else:
            A, B, C = np.concatenate([v00, v11]), np.concatenate([v10, v01]), np.concatenate([v01, v10])
        e1, e2 = B - A, C - A
        pv = np.cross(dr, e2)
        det = _dot(e1, pv)
        ok = np.abs(det) > 1e-300
        inv = 1 / np.where(ok, det, 1)
        tv = o - A
        u = _dot(tv, pv) * inv
        qv = np.cross(tv, e1)
        v = _dot(qv, dr[None, :]) * inv
        t = _dot(e2, qv) * inv
        hit = ok & (u >= -1e-12) & (v >= -1e-12) & (u + v <= 1 + 1e-12) & (t >= tn[r]) & (t < tf[r])
        if hit.any():
            k = int(np.argmin(np.where(hit, t, np.inf)))
            out[r] = t[k]
            tri[r] = 2 * (int(J[k % len(I)]) * (cols - 1) + int(I[k % len(I)])) + (1 if k >= len(I) else 0)
    out = out.reshape(shape)
    return (out, tri.reshape(shape)) if return_triangle else out


def drop_heightfield_brute(x, y, z_start, heights, scale, reach):
    """The vertical-ray form for the height scan: the z where the ray DOWN from (x, y, z_start) first meets a triangle within `reach`,
    None when it meets none (float64, through hit_heightfield_brute: every triangle near the point, no cell lookup)."""
    t = hit_heightfield_brute(np.array([x, y, z_start], np.float64), np.array([[0.0, 0.0, -1.0]]), heights, scale, 0.0, reach)[0]
    return None if t < 0 else float(z_start - t)


def heightfield_triangle(x, y, heights, scale):
    """(i, j, upper) of the triangle over the world point (x, y): the cell under it (clamped to the grid) and the side of its diagonal;
    arrays in the points' own type"""
    rows, cols = np.asarray(heights).shape
    dt = x.dtype.type
    gx, gy = x * dt(scale) + dt(0.5 * (cols - 1)), y * dt(scale) + dt(0.5 * (rows - 1))
    i = np.clip(np.floor(gx), 0, cols - 2).astype(np.int64)
    j = np.clip(np.floor(gy), 0, rows - 2).astype(np.int64)
    return i, j, (gx - i.astype(x.dtype)) + (gy - j.astype(x.dtype)) > 1


# ---- shading (include/mocca.h mocca_render: cosmetic, but a wrong normal is a wrong frame).  The colour table restates mocca_render.hip's.
PALETTE = ((0.85, 0.55, 0.20), (0.25, 0.55, 0.85), (0.35, 0.75, 0.40), (0.80, 0.35, 0.35), (0.65, 0.45, 0.80), (0.90, 0.80, 0.30), (0.30, 0.75, 0.75), (0.70, 0.70, 0.70))
BG_RGB, GROUND_RGB, PLANK_RGB, TARGET_RGB = (0.53, 0.71, 0.90), ((0.80, 0.80, 0.78), (0.55, 0.58, 0.60)), (0.72, 0.53, 0.33), (0.90, 0.15, 0.15)
HF_LOW_RGB, HF_HIGH_RGB, LIGHT, AMBIENT = (0.30, 0.50, 0.25), (0.85, 0.80, 0.65), (0.36, -0.48, 0.80), 0.35
# `part`: sphere 0; capsule 0 / 1 the end spheres at p1 / p2, 2 the tube; box 2 axis + (1 the face on the +axis side); cylinder 0 side, 1 / 2 the
# cap at +z / -z; ground the checker parity; height field the triangle 2 (j (cols - 1) + i) + upper; nothing -1
PART_NONE = -1


def _shade(scene, o, d, best, ids, src, dtype):
    """normal, part and unrounded colour of every pixel from what render() found: src = the prim index, n_prims + k for plank k,
    -2 ground, -3 height field, -1 nothing"""
    H, W = ids.shape
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    nrm = np.zeros((H, W, 3), dtype)
    nrm[..., 2] = 1
    part = np.full((H, W), PART_NONE, np.int64)
    base = np.broadcast_to(f(BG_RGB), (H, W, 3)).copy()
    hp = (o + best[..., None] * d).astype(dtype)
    prims = np.asarray(scene["prims"], np.float64).reshape(-1, 9)
    rgbs = np.asarray(scene["prim_rgb"], np.float64).reshape(-1, 3) if scene.get("prim_rgb") is not None else np.tile(PALETTE[7], (len(prims), 1))
    for k, p in enumerate(prims):
        m = src == k
        if not m.any():
            continue
        pa, pb, r = f(p[0:3]), f(p[3:6]), dtype(p[6])
        dm, hm = d[m], hp[m]
        c = np.broadcast_to(pa, hm.shape).copy()
        pt = np.zeros(len(hm), np.int64)
        if int(p[8]):
            t, t2, t3 = hit_sphere(o, dm, pa, r), hit_sphere(o, dm, pb, r), hit_tube(o, dm, pa, pb, r)
            m2 = (t2 >= 0) & ((t < 0) | (t2 < t))
            t = np.where(m2, t2, t)
            m3 = (t3 >= 0) & ((t < 0) | (t3 < t))
            pt = np.where(m3, 2, np.where(m2, 1, 0))
            ba = pb - pa
            s = _dot(hm - pa, ba) / _dot(ba, ba)
            c = np.where((pt == 1)[:, None], pb, c)
            c = np.where((pt == 2)[:, None], pa + s[:, None] * ba, c).astype(dtype)
        nrm[m], part[m], base[m] = (hm - c) * (dtype(1) / r), pt, f(rgbs[k])
    half = f(scene.get("plank_half", (0, 0, 0)))
    for k, p in enumerate(np.asarray(scene.get("planks", ()), np.float64).reshape(-1, 12)):
        m = src == len(prims) + k
        if not m.any():
            continue
        R = f(p[0:9]).reshape(3, 3)
        lo, ld = _local(o, d[m], f(p[0:9]), f(p[9:12]))
        ln = np.zeros(ld.shape, dtype)
        if scene.get("plank_shape", 0) == 1:
            tm = best[m]
            side = hit_cylinder(o, d[m], f(p[0:9]), f(p[9:12]), half)
            rad, hz = half[0], half[2]
            A, B, C = ld[:, 0] ** 2 + ld[:, 1] ** 2, lo[0] * ld[:, 0] + lo[1] * ld[:, 1], lo[0] ** 2 + lo[1] ** 2 - rad * rad
            disc = B * B - A * C
            ok = (A > 1e-20) & (disc >= 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                ts = (-B - np.sqrt(np.maximum(disc, 0))) / np.where(ok, A, 1)
            on_side = ok & (np.abs(lo[2] + ts * ld[:, 2]) <= hz) & (side == ts)      # hit_cylinder kept the side's root: no nearer cap
            ir = dtype(1) / rad
            ln[:, 0] = np.where(on_side, (lo[0] + tm * ld[:, 0]) * ir, 0)
            ln[:, 1] = np.where(on_side, (lo[1] + tm * ld[:, 1]) * ir, 0)
            ln[:, 2] = np.where(on_side, 0, np.where(ld[:, 2] < 0, 1, -1))
            pt = np.where(on_side, 0, np.where(ld[:, 2] < 0, 1, 2))
        else:
            par = np.abs(ld) < 1e-20
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1 / np.where(par, 1, ld)
            ta = np.minimum((-half - lo) * inv, (half - lo) * inv)
            ax = np.argmax(np.where(par, -np.inf, ta), axis=1)         # the slab entered last; the first of equals
            sg = np.where(np.take_along_axis(ld, ax[:, None], 1)[:, 0] < 0, 1, -1)
            ln[np.arange(len(ax)), ax] = sg
            pt = 2 * ax + (sg > 0)
        nrm[m], part[m], base[m] = ln @ R.T, pt, f(PLANK_RGB)
    m = src == -2
    if m.any():
        odd = ((np.floor(hp[m][:, 0]).astype(np.int64) + np.floor(hp[m][:, 1]).astype(np.int64)) & 1) != 0
        part[m], base[m] = odd.astype(np.int64), np.where(odd[:, None], f(GROUND_RGB[1]), f(GROUND_RGB[0]))
    m = src == -3
    if m.any():
        hts, sc = f(scene["hf"][0]), dtype(scene["hf"][1])
        i, j, up = heightfield_triangle(hp[m][:, 0], hp[m][:, 1], hts, sc)
        h00, h10, h01, h11 = hts[j, i], hts[j, i + 1], hts[j + 1, i], hts[j + 1, i + 1]
        gx, gy = np.where(up, h11 - h01, h10 - h00), np.where(up, h11 - h10, h01 - h00)      # the triangle's slope per cell
        n = np.stack([-gx * sc, -gy * sc, np.ones_like(gx)], -1)
        nrm[m] = n * (dtype(1) / np.sqrt(_dot(n, n)))[:, None]
        part[m] = 2 * (j * (hts.shape[1] - 1) + i) + up
        zmin, zmax = hts.min(), hts.max()
        w = np.clip((hp[m][:, 2] - zmin) / (zmax - zmin), 0, 1) if zmax > zmin else np.zeros(int(m.sum()), dtype)
        base[m] = f(HF_LOW_RGB) + w[:, None] * (f(HF_HIGH_RGB) - f(HF_LOW_RGB))
    shade = np.where(ids >= 0, dtype(AMBIENT) + (dtype(1) - dtype(AMBIENT)) * np.maximum(_dot(nrm, f(LIGHT)), 0), 1).astype(dtype)
    return dict(normal=nrm, part=part, colour=(base * shade[..., None] * dtype(255)).astype(dtype))


def render(scene, camera, W, H, dtype=np.float64, shading=False):
    dtype = np.dtype(dtype).type
    o, d = rays(camera, W, H, dtype)
    cam = np.asarray(camera, dtype)
    tnear, tfar = cam[14], cam[15]
    best = np.full((H, W), tfar, dtype)
    ids = np.full((H, W), ID_NONE, np.int32)
    src = np.full((H, W), -1, np.int64)

    def take(t, code, what):
        nonlocal best, ids, src
        m = (t >= tnear) & (t < best)
        best = np.where(m, t, best).astype(dtype)
        ids = np.where(m, code, ids).astype(np.int32)
        src = np.where(m, what, src)

    prims = np.asarray(scene["prims"], np.float64).reshape(-1, 9)
    for k, p in enumerate(prims):
        pa, pb, r = p[0:3].astype(dtype), p[3:6].astype(dtype), dtype(p[6])
        if not r > 0:          # a point (a hull support point of a mesh link): nothing a ray can enter, though float32 rounding can make h >= 0
            continue
        take(hit_capsule(o, d, pa, pb, r) if int(p[8]) else hit_sphere(o, d, pa, r), int(p[7]), k)
    half = np.asarray(scene.get("plank_half", (0, 0, 0)), dtype)
    for k, p in enumerate(np.asarray(scene.get("planks", ()), np.float64).reshape(-1, 12)):
        fn = hit_cylinder if scene.get("plank_shape", 0) == 1 else hit_box
        take(fn(o, d, p[0:9].astype(dtype), p[9:12].astype(dtype), half), ID_PLANK0 + k, len(prims) + k)
    if scene.get("ground"):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where((d[..., 2] < 0) & (o[2] > 0), -o[2] / np.where(d[..., 2] < 0, d[..., 2], -1), -1).astype(dtype)
        take(t, ID_GROUND, -2)
    if scene.get("hf") is not None:
        take(hit_heightfield(o, d, scene["hf"][0], scene["hf"][1], tnear, best), ID_HEIGHTFIELD, -3)
    if shading:
        return best, ids, _shade(scene, o, d, best, ids, src, dtype)
    return best, ids


def edge_mask(ids, part=None):
    """pixels whose 3 x 3 neighbourhood in the id image is not uniform (the image border compares with itself); with `part`, in the image
    of the pair (id, part): the faces of one plank, the triangles of the height field and the squares of the checker share an id and a
    continuous depth, but not a colour"""
    H, W = ids.shape
    e = np.zeros(ids.shape, bool)
    for img in (ids,) if part is None else (ids, part):
        p = np.pad(img, 1, mode="edge")
        for dj in range(3):
            for di in range(3):
                e |= p[dj:dj + H, di:di + W] != img
    return e


def euler_to_mat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                     -sp, cp * sr, cp * cr])


# wrong scenes the comparisons must tell from the right one: three wrong plank frames (stage_plank, height_scan_reference.plank_frames) and
# the height field's cells split along the other diagonal (mirrored_x; height_scan_reference.scan)
PLANK_MUTATIONS, HF_MUTATIONS = ("transposed", "roll_pitch_swapped", "com_rotated"), ("other_diagonal",)
MUTATIONS = PLANK_MUTATIONS + HF_MUTATIONS


def stage_plank(row, half_z, com_z, mutate=None):
    """[12] rotation (world <- plank) and centre of the plank of one terrain row (x, y, z, yaw, roll, pitch): the row's position is the
    centre of the top face when com_z = 0; the inertial offset com_z is along WORLD z, not rotated with the plank.  `mutate`: one of the
    wrong frames the comparisons must tell from the right one (MUTATIONS)."""
    assert mutate is None or mutate in PLANK_MUTATIONS, mutate
    ti = np.asarray(row, np.float64)
    Rb = euler_to_mat(ti[5], ti[4], ti[3]) if mutate == "roll_pitch_swapped" else euler_to_mat(ti[4], ti[5], ti[3])
    if mutate == "transposed":
        Rb = Rb.reshape(3, 3).T.ravel()
    dz = -half_z - com_z
    if mutate == "com_rotated":
        return np.array([*Rb, ti[0] + Rb[2] * (dz + com_z), ti[1] + Rb[5] * (dz + com_z), ti[2] + Rb[8] * (dz + com_z)])
    return np.array([*Rb, ti[0] + Rb[2] * dz, ti[1] + Rb[5] * dz, ti[2] + Rb[8] * dz + com_z])


def scene_from_records(model, task_id, frames, walk_target, terrain=None, hf=None, mutate=None):
    """The primitive list of one env: `frames` [n_bodies][15] (the oracle's link_frames), walk_target (3), terrain the env's record
    (20 rows of 6, then the live planks' rows) for the Stepper, hf = (heights, scale) for the planner envs."""
    fr = np.asarray(frames, np.float64)
    prims, rgbs = [], []
    nb = model.n_bodies
    if any(model.g_radius[g] > 0 for g in range(model.n_geoms)):
        for g in range(model.n_geoms):
            b = model.g_body[g]
            R, org = fr[b, 0:9].reshape(3, 3), fr[b, 9:12]
            p1 = R @ np.array(model.g_p1[g][:], np.float64) + org
            p2 = R @ np.array(model.g_p2[g][:], np.float64) + org
            prims.append([*p1, *p2, model.g_radius[g], g, 1 if model.g_type[g] == 1 else 0])
            rgbs.append(PALETTE[b & 7])
    else:   # every geom is a point: the skeleton (include/mocca.h mocca_render)
        for b in range(1, nb):
            prims.append([*fr[model.parent[b], 9:12], *fr[b, 9:12], SKELETON_RADIUS, ID_LINK0 + b, 1])
            rgbs.append(PALETTE[b & 7])
        for b in range(1, nb):
            if not any(model.parent[c] == b for c in range(1, nb)):
                prims.append([*fr[b, 9:12], *(2 * fr[b, 12:15] - fr[b, 9:12]), SKELETON_RADIUS, ID_LINK0 + b, 1])
                rgbs.append(PALETTE[b & 7])
        prims, rgbs = prims[:MAX_PRIMS - 1], rgbs[:MAX_PRIMS - 1]
    if task_id != TASK_CASSIE:
        wt = np.asarray(walk_target, np.float64)
        prims.append([*wt, *wt, 0.15, ID_TARGET, 0])
        rgbs.append(TARGET_RGB)
    scene = dict(prims=np.array(prims), prim_rgb=np.array(rgbs), ground=task_id in (TASK_CUSTOM, TASK_CASSIE), hf=hf if task_id == TASK_PLANNER else None)
    if task_id == TASK_STEPPER:
        ter = np.asarray(terrain, np.float64)
        half = np.array(model.plank_half[:], np.float64)
        planks = [stage_plank(ter[6 * int(ter[120 + k]):][:6], half[2], float(model.plank_com_z), mutate) for k in range(model.n_planks)]
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


def reference_scene(model, task_id, state32, task, terrain, hf, env=SCENE_ENV, mutate=None):
    """the float64 primitive list of env `env`: link frames from the float64 oracle on the float32 state"""
    from oracle.oracle import Oracle
    o64 = Oracle(model.to_bytes(), task_id, state32.shape[0], "f64")
    if hf is not None:
        o64.set_heightfield(*hf)
    o64.set_state(state32.astype(np.float64))
    frames = o64.link_frames(env, model.n_bodies)
    return scene_from_records(model, task_id, frames, np.asarray(task[env, 0:3], np.float32), terrain[env], hf, mutate=mutate)


# ---- synthetic scenes: hand-made terrain records with ROTATED live planks, and planner bases over the hills, at the grid's border and
# ---- outside it.  The oracle only supplies a valid robot pose (reset); the base is then moved by set_state. ----
NEW_ENVS, NEW_SEED = 3, 11
STRESS_MAX = 0.5             # rad: the stress set draws yaw, roll and pitch with 0.2 <= |angle| <= 0.5, all three non-zero at once
PLANK_SCENES = {             # name: (env id, model keywords, "model" = the model's own ranges at curriculum 9 | "stress")
    "tilt_box": ("Walker3DStepperEnv-v0", {}, "model"),
    "stress_box": ("Walker3DStepperEnv-v0", {}, "stress"),
    "stress_plank": ("Walker3DStepperEnv-v0", {"plank_class": "Plank"}, "stress"),
    "stress_pillar": ("Walker3DStepperEnv-v0", {"plank_class": "Pillar"}, "stress"),
    "tilt_laikago": ("LaikagoStepperEnv-v0", {}, "model"),
    "stress_laikago": ("LaikagoStepperEnv-v0", {}, "stress"),
}
PLANNER_ENV = "Walker3DPlannerEnv-v0"
# env 0 over sloped terrain, env 1 within a cell (0.25 m) of the grid's border x = 15.875, env 2 outside the grid
PLANNER_BASES = {"hills": (1.7, -2.3), "border": (15.7, 3.1), "outside": (17.0, -4.2)}
PLANNER_ENV_OF = {"hills": 0, "border": 1, "outside": 2}
BASE_CLEARANCE = 1.3         # base z above the middle live plank / the terrain under it
FIRST_LIVE_ROW = 3           # rows 0-2 stay flat as the oracle lays them; the live planks are rows 3, 4, ... whose angles are drawn


def synthetic_terrain(model, kind, rng):
    """One full 128-float terrain record: 20 rows (x, y, z, yaw, roll, pitch), the live planks' row numbers at 120 .. 120 + n_planks,
    zeros after.  Positions follow the Stepper's layout (rows init_step_separation apart along x, z from the polar-angle range);
    the angles of rows >= 3 come from `rng`."""
    ter = np.zeros(128)
    sep = float(model.init_step_separation)
    deg = np.pi / 180
    for r in range(20):
        row = ter[6 * r:6 * r + 6]
        row[0] = r * sep
        if r < FIRST_LIVE_ROW:
            continue
        if kind == "model":
            yr, tr, pr = float(model.yaw_range_deg) * deg, float(model.tilt_range_deg) * deg, float(model.pitch_range_deg) * deg
            row[3], row[4], row[5] = rng.uniform(-yr, yr), rng.uniform(-tr, tr), rng.uniform(-tr, tr)
            row[2] = ter[6 * (r - 1) + 2] + sep * np.sin(rng.uniform(-pr, pr)) * 0.3
        else:
            row[3:6] = rng.uniform(0.2, STRESS_MAX, 3) * rng.choice([-1.0, 1.0], 3)
            row[2] = rng.uniform(-0.1, 0.1)
        row[1] = rng.uniform(-0.1, 0.1)
    ter[120:120 + int(model.n_planks)] = FIRST_LIVE_ROW + np.arange(int(model.n_planks))
    return ter


def synthetic_records(name):
    """The tuple of scene_records() for a synthetic scene: a name of PLANK_SCENES, or "planner" (PLANNER_BASES, one env each)."""
    from mocca_envs_amd.vec_env import compile_model_for
    from oracle.oracle import Oracle
    planner = name == "planner"
    env_id, kw, kind = (PLANNER_ENV, {}, None) if planner else PLANK_SCENES[name]
    task_id = TASK_PLANNER if planner else TASK_STEPPER
    model = compile_model_for(env_id, **kw)
    orc = Oracle(model.to_bytes(), task_id, NEW_ENVS, "f32")
    hf = None
    if planner:
        from mocca_envs_amd.terrain import load_height_field
        hf = load_height_field()
        orc.set_heightfield(*hf)
    orc.reset(seed=NEW_SEED)
    st, tk, ter = orc.get_state().astype(np.float32), orc.get_task(), np.zeros((NEW_ENVS, 128))
    ter[:, :orc.get_terrain().shape[1]] = orc.get_terrain()
    rng = np.random.default_rng([NEW_SEED, sorted(PLANK_SCENES).index(name) if not planner else 99])
    for e in range(NEW_ENVS):
        if planner:
            x, y = list(PLANNER_BASES.values())[e]
            from mocca_envs_amd import host_logic as HL
            inside = abs(x) <= 0.5 * (hf[0].shape[1] - 1) / hf[1] and abs(y) <= 0.5 * (hf[0].shape[0] - 1) / hf[1]
            st[e, 0:3] = x, y, (HL.height_at(hf[0], hf[1], x, y) if inside else 0.0) + BASE_CLEARANCE
        else:
            ter[e] = synthetic_terrain(model, kind, rng)
            mid = ter[e, 6 * (FIRST_LIVE_ROW + 1):][:3]
            st[e, 0:3] = mid[0], mid[1], mid[2] + BASE_CLEARANCE
    return model, task_id, kw, st, tk, ter, hf


def _record(target, yaw, pitch, dist, aspect, far=100.0):
    """a camera record whose axes are EXACT at the quarter turns (cos 90 degrees is 6e-17 in floating point, not 0): with an odd image size
    the centre column and row then carry rays with exactly zero components"""
    from mocca_envs_amd.render import Camera
    c = Camera(yaw=yaw, pitch=pitch, dist=dist, far=far)
    c.lookat(target)
    rec = c.pack(aspect)
    rec[3:12][np.abs(rec[3:12]) < 1e-7] = 0.0
    return rec


# planner cases that are left out, and why: from outside the grid a level camera that looks away from it sees no terrain at all, and there is
# no surface under the base to be under or close to
PLANNER_LEFT_OUT = {("outside", "level0"), ("outside", "below_up"), ("outside", "close"), ("outside", "close2")}


def new_cameras(kind, base_pos, aspect, hf=None, where=None):
    """The cameras of the synthetic scenes: `kind` "plank" or "planner" (`where` a name of PLANNER_BASES); base_pos the env's base.  Plank
    scenes are looked at three quarters of the way from the base to the planks under it.  From outside the grid the cameras that have a free yaw look
    back at it (yaw + 180)."""
    b = np.asarray(base_pos, np.float64)
    at = b - np.array([0.0, 0.0, 0.75 * BASE_CLEARANCE]) if kind == "plank" else b
    yaw0 = 180.0 if where == "outside" else 0.0
    cams = {"follow": _record(at, yaw0, -5.0, 1.2 if kind == "plank" else 1.5, aspect),
            "oblique": _record(at, yaw0 + 40.0, -30.0, 1.0 if kind == "plank" else 1.3, aspect),
            "down": _record(at, 0.0, -90.0, 1.6, aspect)}
    for yaw in (0, 90, 180, 270):
        cams["level%d" % yaw] = _record(at, float(yaw), 0.0, 1.7, aspect)
    # far ends inside the scene: beyond it depth is exactly far
    cams["short_far"] = _record(at, yaw0 + 40.0, -30.0, 1.3, aspect, far=1.9 if kind == "plank" else 3.5)
    if kind == "planner":
        edge = 0.5 * (hf[0].shape[1] - 1) / hf[1]
        ground = b - np.array([0.0, 0.0, BASE_CLEARANCE])
        cams["outside_in"] = _record((edge + 2.0, b[1], 2.5), 180.0, -20.0, 0.0, aspect)      # 2 m outside the grid, looking in
        cams["below_up"] = _record(ground - np.array([0.0, 0.0, 0.3]), 30.0, 50.0, 0.0, aspect)   # 0.3 m under the surface, looking up
        cams["close"] = _record(ground, yaw0 + 25.0, -80.0, 0.5, aspect)                      # triangles many pixels wide: the colour comparison's view
        cams["close2"] = _record(ground, yaw0 + 205.0, -65.0, 0.6, aspect)                    # a second one from the other side: other faces of the slopes lit
        cams = {k: v for k, v in cams.items() if (where, k) not in PLANNER_LEFT_OUT}
    return cams


NEW_RESOLUTIONS = ((1, 1), (17, 33), (161, 121))        # on every new camera; the existing two sizes on follow and oblique
TINY = 17 * 33                                          # up to this many pixels an image is exempt from the share conditions
# (scene or planner base, camera, width): cases whose (id, part) mask leaves out more than MAX_COLOUR_EDGE -- height-field triangles a few pixels
# wide -- are compared in ids and depth but NOT in colour; the planner's colour is held on the close, close2, below_up, short_far and border views
NO_COLOUR = {("hills", c, w) for c, w in (("follow", 161), ("oblique", 161), ("down", 161), ("level0", 161), ("level90", 161), ("level180", 161), ("level270", 161),
                                           ("outside_in", 161), ("follow", 160), ("oblique", 160), ("follow", 320), ("oblique", 320))} \
    | {("border", c, 161) for c in ("down", "level180", "outside_in")} \
    | {("outside", c, w) for c, w in (("follow", 161), ("oblique", 161), ("level180", 161), ("outside_in", 161), ("follow", 160), ("oblique", 160), ("oblique", 320))}
MAX_ID_EDGE, MIN_SHARE, MAX_COLOUR_EDGE = 0.15, 0.02, 0.35


def new_cases(kind, base_pos, hf=None, where=None):
    """[(camera name, record, width, height)] for one env of a synthetic scene"""
    out = []
    for (w, h) in NEW_RESOLUTIONS + RESOLUTIONS:
        for cname, cam in new_cameras(kind, base_pos, w / h, hf, where).items():
            if (w, h) in NEW_RESOLUTIONS or cname in ("follow", "oblique"):
                out.append((cname, cam, w, h))
    return out


def mirrored_x(scene, camera):
    """(scene, camera) reflected in the plane x = 0: the same image, but the height field's cells end up split along the OTHER diagonal
    (from (i, j) to (i + 1, j + 1)) -- the mutation "other_diagonal" without a second march.  Scenes without planks only."""
    assert "planks" not in scene
    out = dict(scene)
    pr = np.array(scene["prims"], np.float64).reshape(-1, 9)
    pr[:, [0, 3]] *= -1
    hts, sc = scene["hf"]
    out.update(prims=pr, hf=(np.ascontiguousarray(np.asarray(hts)[:, ::-1]), sc))
    cam = np.array(camera, np.float32)
    cam[[0, 3, 6, 9]] *= -1
    return out, cam


def accepts(dep, ids, d64, i64, d32, far):
    """The GPU comparison's own rule for ids and depth (tests/test_gpu_render.py), on a candidate image (dep, ids) against the float64
    reference (d64, i64) with the float32 reference's depth d32 as the yardstick: (ok, figures)."""
    keep = ~edge_mask(i64)
    hit = keep & (i64 >= 0)
    wrong = int((ids != i64)[keep].sum())
    e32 = float((np.abs(d32.astype(np.float64) - d64)[hit] / d64[hit]).max()) if hit.any() else 0.0
    ek = float((np.abs(dep.astype(np.float64) - d64)[hit] / d64[hit]).max()) if hit.any() else 0.0
    far_ok = bool((dep[ids == -1] == np.float32(far)).all())
    fig = dict(compared=int(keep.sum()), id_mismatches=wrong, numpy_f32_depth_err=e32, kernel_depth_err=ek)
    return wrong == 0 and ek <= 4 * e32 and far_ok, fig


def colour_accepts(rgb, s64, s32, i64):
    """|rgb - v64| <= 0.5 + 4 e32 in levels on the pixels the (id, part) mask keeps; v64 the unrounded float64 colour, e32 the float32
    reference's largest error on the same pixels: (ok, figures)"""
    keep = ~edge_mask(i64, s64["part"])
    if not keep.any():
        return True, dict(colour_compared=0, numpy_f32_colour_err=0.0, kernel_colour_err=0.0)
    e32 = float(np.abs(s32["colour"].astype(np.float64) - s64["colour"])[keep].max())
    ek = float(np.abs(np.asarray(rgb, np.float64) - s64["colour"])[keep].max())
    return ek <= 0.5 + 4 * e32, dict(colour_compared=int(keep.sum()), numpy_f32_colour_err=e32, kernel_colour_err=ek)


# ---- negative controls: one camera and size per scene, rendered by the comparisons anyway ----
CONTROL_CAMERA, CONTROL_SIZE = "oblique", (160, 120)


def control_cases():
    """[(scene, mutation, env, where)]: every plank scene under the three wrong frames, the hills and the border under the other split"""
    out = [(name, m, 0, None) for name in PLANK_SCENES for m in PLANK_MUTATIONS]
    return out + [("planner", m, e, where) for m in HF_MUTATIONS for where, e in PLANNER_ENV_OF.items() if where != "outside"]


def mutated_references(mutation, rec, e, cam, w, h):
    """(d64, i64, d32) of the float64 / float32 references of env e of a scene that is wrong in one way.  other_diagonal: the mirrored
    scene through the mirrored camera -- pixel for pixel the same view, of cells split the other way."""
    model, task_id, kw, st, tk, ter, hf = rec
    if mutation in HF_MUTATIONS:
        scene, mcam = mirrored_x(reference_scene(model, task_id, st, tk, ter, hf, env=e), cam)
    else:
        scene, mcam = reference_scene(model, task_id, st, tk, ter, hf, env=e, mutate=mutation), cam
    d64, i64 = render(scene, mcam, w, h, np.float64)
    d32, _ = render(scene, mcam, w, h, np.float32)
    return d64, i64, d32


def compared_cases(name, rec):
    """[(label, where, env, camera name, record, width, height)]: what the GPU comparison renders of a synthetic scene and the validity
    test holds to its caps -- plank scenes: env 0 at every size, envs 1 and 2 at 161 x 121; planner: one env per base, every size"""
    model, task_id, kw, st, tk, ter, hf = rec
    out = []
    if name == "planner":
        for where, e in PLANNER_ENV_OF.items():
            out += [(where, where, e, *c) for c in new_cases("planner", st[e, 0:3], hf, where)]
    else:
        for e in range(NEW_ENVS):
            out += [(name, None, e, *c) for c in new_cases("plank", st[e, 0:3]) if e == 0 or (c[2], c[3]) == (161, 121)]
    return out
