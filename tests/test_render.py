"""Rendering, the part that needs no GPU: the ABI, the camera, and the numpy reference ray caster held to analytic cases and to the
validity conditions of the GPU comparison (tests/test_gpu_render.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import render_reference as RR  # noqa: E402

from mocca_envs_amd import lib  # noqa: E402
from mocca_envs_amd.render import Camera  # noqa: E402


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_render_symbols():
    hdr = open(os.path.join(ROOT, "include", "mocca.h")).read()
    for name in ("mocca_get_link_frames", "mocca_render"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in include/mocca.h"
        assert name in lib.SYMBOLS
    for name, val in (("NONE", -1), ("GROUND", 32), ("PLANK0", 33), ("HEIGHTFIELD", 37), ("TARGET", 38), ("LINK0", 64)):
        assert re.search(r"MOCCA_RENDER_ID_%s\s*=\s*%d\b" % (name, val), hdr)
        assert getattr(lib, "RENDER_ID_" + name) == val == getattr(RR, "ID_" + name)
    assert re.search(r"#define\s+MOCCA_CAMERA_FLOATS\s+16\b", hdr) and lib.CAMERA_FLOATS == 16
    assert re.search(r"#define\s+MOCCA_ABI_VERSION\s+8\b", hdr) and lib.ABI_VERSION == 8
    from mocca_envs_amd.build import build_lib
    so = build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("mocca_get_link_frames", "mocca_render"):
        assert re.search(r"\sT\s+%s$" % name, syms, re.M), name + " is not exported by the library"
    import ctypes
    assert ctypes.CDLL(so).mocca_abi_version() == 8


# ---- camera ----------------------------------------------------------------------------------------------------------------------
def _axes(rec):
    return rec[0:3], rec[3:6], rec[6:9], rec[9:12]


@pytest.mark.parametrize("yaw,pitch,right,up,forward", [
    (0, 0, (0, -1, 0), (0, 0, 1), (1, 0, 0)),
    (90, 0, (1, 0, 0), (0, 0, 1), (0, 1, 0)),
    (0, -90, (0, -1, 0), (1, 0, 0), (0, 0, -1)),
    (90, -90, (1, 0, 0), (0, 1, 0), (0, 0, -1)),
])
def test_camera_pack_closed_forms(yaw, pitch, right, up, forward):
    cam = Camera(yaw=yaw, pitch=pitch, dist=2.5)
    target = np.array([0.3, -1.2, 0.9])
    cam.lookat(target)
    rec = cam.pack(4 / 3).astype(np.float64)
    eye, r, u, f = _axes(rec)
    assert np.allclose(r, right, atol=1e-7) and np.allclose(u, up, atol=1e-7) and np.allclose(f, forward, atol=1e-7)
    assert np.allclose(eye, target - 2.5 * np.array(forward), atol=1e-6)
    assert np.allclose(np.cross(f, u), r, atol=1e-7)
    assert np.allclose(rec[12:16], [np.tan(np.pi / 6), 4 / 3, 0.1, 100.0], rtol=1e-6)


def test_camera_defaults_and_orthonormal():
    cam = Camera()
    assert (cam.yaw, cam.pitch, cam.dist, cam.fov, cam.near, cam.far) == (0, -5, 2.5, 60, 0.1, 100)
    rec = Camera(yaw=37, pitch=-23).pack().astype(np.float64)
    A = np.stack(_axes(rec)[1:])
    assert np.allclose(A @ A.T, np.eye(3), atol=1e-6)
    assert rec[9 + 2] < 0 and rec[6 + 2] > 0      # a negative pitch looks down; up keeps a positive z


def test_camera_track_smoothing():
    cam = Camera()
    cam.lookat([1.0, 2.0, 1.0])
    cam.track(np.array([2.0, 4.0, 2.0]))               # (1, 1, 0.1): x and y jump, z moves a tenth of the way
    assert np.allclose(cam.target, [2.0, 4.0, 1.1])
    cam.track(np.array([3.0, 3.0, 0.1]))
    assert np.allclose(cam.target, [3.0, 3.0, 0.9 * 1.1 + 0.1 * 0.1])
    cam.track(np.array([0.0, 0.0, 0.0]), smooth_coef=np.array([0.5, 0.5, 0.5]))
    assert np.allclose(cam.target, [1.5, 1.5, 0.5])
    with pytest.raises(AssertionError):
        cam.track(np.zeros(3), smooth_coef=np.array([2.0, 1.0, 1.0]))


# ---- the reference ray caster against analytic cases -----------------------------------------------------------------------------
W, H = 33, 25           # odd: pixel (12, 16) looks straight down the view axis
CJ, CI = 12, 16
TOL = {np.float64: 2e-7, np.float32: 2e-6}   # relative; float64 too sees the camera RECORD, which is float32 by definition (half an ulp = 6e-8 per entry)


def _cam(eye=(0, 0, 0), yaw=0, pitch=0):
    c = Camera(yaw=yaw, pitch=pitch, dist=0.0)
    c.lookat(eye)
    return c.pack(W / H)


def _prim(p1, p2, r, gid, kind):
    return [*p1, *p2, r, gid, kind]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_sphere_dead_ahead(dtype):
    d, r = 3.0, 0.4
    dep, ids = RR.render(dict(prims=[_prim((d, 0, 0), (d, 0, 0), r, 5, 0)]), _cam(), W, H, dtype)
    assert ids[CJ, CI] == 5 and abs(dep[CJ, CI] - (d - r)) <= TOL[dtype] * d
    assert ids[0, 0] == -1 and dep[0, 0] == dtype(100.0)
    # off-axis pixel: depth is the distance ALONG THE VIEW AXIS of the hit point of that pixel's ray
    o, dirs = RR.rays(_cam(), W, H, np.float64)
    dv = dirs[CJ, CI + 1]
    t = (d * dv[0] - np.sqrt((d * dv[0]) ** 2 - (dv @ dv) * (d * d - r * r))) / (dv @ dv)
    assert ids[CJ, CI + 1] == 5 and abs(dep[CJ, CI + 1] - t) <= TOL[dtype] * d


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_capsule_end_on_and_side_on(dtype):
    r = 0.25
    end_on = dict(prims=[_prim((2.0, 0, 0), (3.0, 0, 0), r, 1, 1)])       # axis along the view axis: the near end sphere
    dep, ids = RR.render(end_on, _cam(), W, H, dtype)
    assert ids[CJ, CI] == 1 and abs(dep[CJ, CI] - (2.0 - r)) <= TOL[dtype] * 2
    side_on = dict(prims=[_prim((2.5, -1.0, 0), (2.5, 1.0, 0), r, 2, 1)])  # axis across: the tube
    dep, ids = RR.render(side_on, _cam(), W, H, dtype)
    assert ids[CJ, CI] == 2 and abs(dep[CJ, CI] - (2.5 - r)) <= TOL[dtype] * 2.5
    # beyond the end of the axis only the end sphere is there: looking at (2.5, 1.0 + r / 2, 0) meets it at x = 2.5 - sqrt(r^2 - (r/2)^2)
    y = 1.0 + r / 2
    c = Camera(yaw=0, pitch=0, dist=0.0)
    c.lookat((0, y, 0))
    dep, ids = RR.render(side_on, c.pack(W / H), W, H, dtype)
    assert ids[CJ, CI] == 2 and abs(dep[CJ, CI] - (2.5 - np.sqrt(r * r - (r / 2) ** 2))) <= TOL[dtype] * 2.5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_plane_normal_and_grazing(dtype):
    scene = dict(prims=[], ground=True)
    dep, ids = RR.render(scene, _cam(eye=(0, 0, 2.0), pitch=-90), W, H, dtype)     # straight down from 2 m
    assert ids[CJ, CI] == RR.ID_GROUND and abs(dep[CJ, CI] - 2.0) <= TOL[dtype] * 2
    assert (ids == RR.ID_GROUND).all() and np.allclose(dep, 2.0, rtol=1e-5)          # depth along the axis is the same for every pixel
    graze = np.degrees(np.arctan2(1.0, 50.0))
    rec = _cam(eye=(0, 0, 1.0), pitch=-graze)                                       # 1 m up, meeting the ground 50 m ahead
    dep, ids = RR.render(scene, rec, W, H, dtype)
    want = -float(rec[2]) / float(rec[11])      # from the float32 record itself: at this angle its rounding moves the hit by micrometres
    assert abs(want - np.hypot(50.0, 1.0)) < 1e-4
    assert ids[CJ, CI] == RR.ID_GROUND and abs(dep[CJ, CI] - want) <= (1e-9 if dtype is np.float64 else 2e-5) * want
    assert ids[0, CI] == -1 and dep[0, CI] == dtype(100.0)                          # above the horizon


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_box_face_and_cylinder(dtype):
    yawp = np.radians(30.0)
    R = RR.euler_to_mat(0.0, 0.0, yawp)
    scene = dict(prims=[], planks=[[*R, 4.0, 0.0, 0.0]], plank_half=(0.5, 1.0, 0.2), plank_shape=0)
    cam = _cam(yaw=30.0)                       # along the box's own x axis, from its side: the face x = -0.5
    c = Camera(yaw=30.0, pitch=0.0, dist=3.0)
    c.lookat((4.0, 0.0, 0.0))
    dep, ids = RR.render(scene, c.pack(W / H), W, H, dtype)
    assert ids[CJ, CI] == RR.ID_PLANK0 and abs(dep[CJ, CI] - 2.5) <= TOL[dtype] * 3
    dep, ids = RR.render(scene, _cam(eye=(4.0, 0.0, 3.0), pitch=-90), W, H, dtype)  # from above: the top face z = 0.2
    assert ids[CJ, CI] == RR.ID_PLANK0 and abs(dep[CJ, CI] - 2.8) <= TOL[dtype] * 3
    del cam
    pillar = dict(prims=[], planks=[[*np.eye(3).ravel(), 4.0, 0.0, 0.0]], plank_half=(0.5, 0.5, 0.2), plank_shape=1)
    dep, ids = RR.render(pillar, _cam(), W, H, dtype)                              # side of the cylinder
    assert ids[CJ, CI] == RR.ID_PLANK0 and abs(dep[CJ, CI] - 3.5) <= TOL[dtype] * 4
    dep, ids = RR.render(pillar, _cam(eye=(4.2, 0.1, 3.0), pitch=-90), W, H, dtype)  # its cap
    assert ids[CJ, CI] == RR.ID_PLANK0 and abs(dep[CJ, CI] - 2.8) <= TOL[dtype] * 3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_heightfield_cell(dtype):
    # one cell, 1 m wide (scale 1): corners (-.5, -.5) -> 0.1, (.5, -.5) -> 0.4, (-.5, .5) -> 0.7, (.5, .5) -> 0.2, split from (.5, -.5) to (-.5, .5)
    hts = np.array([[0.1, 0.4], [0.7, 0.2]])
    scene = dict(prims=[], hf=(hts, 1.0))
    for (x, y) in ((-0.2, -0.1), (0.25, 0.3), (0.1, -0.4), (-0.3, 0.45)):
        u, v = x + 0.5, y + 0.5
        z = 0.1 + u * 0.3 + v * 0.6 if u + v <= 1 else 0.2 + (1 - u) * 0.5 + (1 - v) * 0.2
        dep, ids = RR.render(scene, _cam(eye=(x, y, 5.0), pitch=-90), W, H, dtype)
        assert ids[CJ, CI] == RR.ID_HEIGHTFIELD and abs(dep[CJ, CI] - (5.0 - z)) <= TOL[dtype] * 5
    # an oblique ray from outside the cell, against the lower triangle's plane z = 0.1 + 0.3 u + 0.6 v
    eye, look = np.array([-3.0, -0.2, 2.0]), np.array([-0.2, -0.2, 0.1 + 0.3 * 0.3 + 0.6 * 0.3])
    f = (look - eye) / np.linalg.norm(look - eye)
    c = Camera(yaw=np.degrees(np.arctan2(f[1], f[0])), pitch=np.degrees(np.arcsin(f[2])), dist=0.0)
    c.lookat(eye)
    dep, ids = RR.render(scene, c.pack(W / H), W, H, dtype)
    assert ids[CJ, CI] == RR.ID_HEIGHTFIELD and abs(dep[CJ, CI] - np.linalg.norm(look - eye)) <= TOL[dtype] * 10
    assert ids[0, 0] == -1                         # outside the grid there is no ground


# ---- validity of the GPU comparison's exclusion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RR.SCENES))
def test_comparison_scenes_are_valid(name):
    """On every scene the GPU tests use, the float64 reference alone must leave at most 15 % edge pixels and at least 2 % robot pixels
    (a geom, or a link of Cassie's skeleton) that are not edge."""
    model, task_id, kw, st, tk, ter, hf = RR.scene_records(name)
    scene = RR.reference_scene(model, task_id, st, tk, ter, hf)
    for (w, h) in RR.RESOLUTIONS:
        for cname, cam in RR.scene_cameras(st[RR.SCENE_ENV, 0:3], w / h).items():
            _, ids = RR.render(scene, cam, w, h, np.float64)
            edge = RR.edge_mask(ids)
            robot = RR.is_robot(ids) & ~edge
            print(f"{name} {w}x{h} {cname}: edge {edge.mean():.4f} robot-not-edge {robot.mean():.4f}")
            assert edge.mean() <= 0.15, (name, w, cname, edge.mean())
            assert robot.mean() >= 0.02, (name, w, cname, robot.mean())
