"""The egocentric depth camera without a GPU: the ABI's declarations and bindings, perception.DepthCamera's arguments, the mirror table of
the image, and the validity conditions of the GPU comparison (tests/test_gpu_depth_camera.py) held by the float64 reference alone."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import depth_camera_reference as DR  # noqa: E402
import render_reference as RR  # noqa: E402

from mocca_envs_amd import build, lib  # noqa: E402
from mocca_envs_amd import perception as P  # noqa: E402
from mocca_envs_amd.symmetry import check_tables, mirror_tables  # noqa: E402


# ---- 1. declarations, arguments, tables ---------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_depth_camera():
    hdr = open(os.path.join(ROOT, "include", "mocca.h")).read()
    for name, value in (("MOCCA_DEPTH_MAX_PIXELS", 256), ("MOCCA_DEPTH_STABILISED", 1), ("MOCCA_DEPTH_SEE_ROBOT", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert (lib.DEPTH_MAX_PIXELS, lib.DEPTH_STABILISED, lib.DEPTH_SEE_ROBOT) == (256, 1, 2)
    assert (P.DEPTH_MAX_PIXELS, P.DEPTH_STABILISED, P.DEPTH_SEE_ROBOT) == (256, 1, 2)
    so = ctypes.CDLL(build.build_lib())
    for name in ("mocca_set_depth_camera", "mocca_depth_dim", "mocca_depth_camera"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in lib.SYMBOLS and hasattr(so, name), name
    assert "mocca_depth.hip" in build.SOURCES and {"mocca_depth.h", "mocca_scene.h"} <= set(build.DEPS)
    # one definition of the shared geometry, several users
    csrc = os.path.join(ROOT, "mocca_envs_amd", "csrc")
    for fn in ("walk_frames", "hit_sphere", "hit_tube", "hit_heightfield", "stage_robot", "nearest_hit"):
        defs = [f for f in os.listdir(csrc) if re.search(r"^DI \w+ %s\(" % fn, open(os.path.join(csrc, f)).read(), re.M)]
        assert defs == ["mocca_scene.h"], (fn, defs)
    for user in ("mocca_render.hip", "mocca_depth.hip"):
        text = open(os.path.join(csrc, user)).read()
        assert "walk_frames(" in text and "stage_robot(" in text and "nearest_hit<" in text, user      # one ray routine: no copy of its loops
        assert "hit_sphere(" not in text and "hit_box(" not in text and "hit_heightfield(" not in text, user


def test_depth_camera_packs_the_abi_arguments():
    cam = P.DepthCamera(body=3, offset=(0.1, -0.2, 0.3), yaw=30.0, pitch=-35.0, roll=10.0, width=16, height=12, fov_y=90.0, near=0.05, far=6.0,
                        stabilised=True, see_robot=True)
    a = cam.pack()
    assert a["body"] == 3 and a["width"] == 16 and a["height"] == 12 and a["flags"] == 3 and cam.shape == (12, 16)
    assert a["mount"].dtype == np.float32 and a["mount"].shape == (6,)
    # offset, then roll, pitch, yaw in radians; render.Camera's pitch < 0 (down) is the ABI's pitch > 0
    assert np.allclose(a["mount"], [0.1, -0.2, 0.3, np.deg2rad(10.0), np.deg2rad(35.0), np.deg2rad(30.0)], atol=1e-7)
    assert a["fov_y"] == pytest.approx(np.pi / 2) and a["near"] == 0.05 and a["far"] == 6.0
    assert P.DepthCamera().pack()["flags"] == 0 and P.DepthCamera().fov_y == 60.0
    # the camera's axes agree with render.Camera's for the same yaw and pitch
    from mocca_envs_amd.render import camera_axes
    m = a["mount"].astype(np.float64)
    R = RR.euler_to_mat(0.0, m[4], m[5]).reshape(3, 3)
    right, up, forward = camera_axes(30.0, -35.0)
    assert np.allclose(R[:, 0], forward, atol=1e-6) and np.allclose(R[:, 2], up, atol=1e-6) and np.allclose(np.cross(R[:, 0], R[:, 2]), right, atol=1e-6)
    assert forward[2] < 0                                                    # a negative pitch looks down
    for bad in (dict(width=0), dict(height=65), dict(width=64, height=5), dict(fov_y=0.0), dict(fov_y=180.0), dict(near=0.0), dict(near=1.0, far=1.0),
                dict(far=np.inf), dict(near=np.nan), dict(offset=(0.0, np.nan, 0.0)), dict(offset=(0.0, 0.0)), dict(yaw=np.inf), dict(body=-1)):
        with pytest.raises(ValueError):
            P.DepthCamera(**bad)
    assert P.DepthCamera(width=64, height=4).shape == (4, 64) and P.DepthCamera(width=1, height=1).pack()["width"] == 1
    assert P.DepthCamera(offset=(0.2, 0.0, 0.1), pitch=-20.0).sagittal
    for off in (dict(body=1), dict(offset=(0.0, 0.01, 0.0)), dict(yaw=5.0), dict(roll=-2.0)):
        assert not P.DepthCamera(**off).sagittal


def test_mirror_tables_flip_the_image_columns():
    mi = ([0], [1], [2], [1], [], [])
    H, W = 3, 5
    in_perm, in_sign, act_perm, act_sign = mirror_tables(mi, 4, 2, depth_shape=(H, W))
    assert in_perm.shape == (4 + H * W,) and in_perm.dtype == np.int32 and in_sign.dtype == np.float32
    assert in_perm[:4].tolist() == [0, 2, 1, 3] and in_sign[:4].tolist() == [-1, 1, 1, 1]
    img = np.arange(H * W).reshape(H, W)
    assert (in_perm[4:] - 4).reshape(H, W).tolist() == img[:, ::-1].tolist() and (in_sign[4:] == 1).all()
    assert np.array_equal(in_perm[in_perm], np.arange(4 + H * W))             # an involution
    check_tables((in_perm, in_sign, act_perm, act_sign), in_dim=4 + H * W, act_dim=2)
    # after a scan: [obs | scan | depth]
    pts = np.array([[0.5, 0.2], [0.5, -0.2], [1.0, 0.0]], np.float32)
    both = mirror_tables(mi, 4, 2, scan_points=pts, depth_shape=(H, W))[0]
    assert both[:7].tolist() == [0, 2, 1, 3, 5, 4, 6] and (both[7:] - 7).reshape(H, W).tolist() == img[:, ::-1].tolist()
    assert np.array_equal(both[both], np.arange(7 + H * W))
    one = mirror_tables(mi, 4, 2, depth_shape=(1, 1))[0]
    assert one.tolist() == [0, 2, 1, 3, 4]
    odd = mirror_tables(mi, 4, 2, depth_shape=(2, 3))[0]
    assert odd[4:].tolist() == [6, 5, 4, 9, 8, 7]                             # the middle column maps to itself
    for bad in ((0, 4), (3,), (2, 2.5), (2, -1)):
        with pytest.raises(ValueError):
            mirror_tables(mi, 4, 2, depth_shape=bad)


# ---- 2. the validity of the GPU comparison --------------------------------------------------------------------------------------------
def _image_reference(kind, name, e, flags, label, w, h, frames):
    model, task_id, kw, st, tk, ter, hf = DR.records_of(kind, name)
    cam = DR.camera_for(flags, label, w, h)
    rec = DR.camera_record(frames[e], st[e, 3:7], cam.pack(), np.float64).astype(np.float32)
    scene = DR.depth_scene(model, task_id, frames[e], ter[e], hf, bool(flags & DR.SEE_ROBOT))
    return scene, rec, DR.references(scene, rec, w, h)


def test_reference_holds_the_comparisons_validity_conditions():
    """For every image the GPU test compares: at most MAX_EXCLUDED of the pixels are left out, and wherever terrain is in view at least one
    kept pixel hits terrain.  The float64 reference alone, from its own camera record."""
    frames, seen_terrain = {}, 0
    worst = (1.0, None)
    for kind, name, e, flags, label, w, h in DR.compared_images():
        if (kind, name) not in frames:
            model, task_id, kw, st, tk, ter, hf = DR.records_of(kind, name)
            frames[kind, name] = DR.oracle_frames(model, task_id, st, hf)
        scene, rec, (d64, i64, d32, keep) = _image_reference(kind, name, e, flags, label, w, h, frames[kind, name])
        share = float(keep.mean())
        worst = min(worst, (share, (kind, name, e, label, w, h)))
        hit_share = float((keep & (i64 >= 0)).mean())
        print(kind, name, e, label, w, h, "kept %.3f, kept hits %.3f" % (share, hit_share))
        if w * h > 1:
            assert 1.0 - share <= DR.MAX_EXCLUDED, (kind, name, e, label, w, h, share)
        else:      # one pixel is compared for hit / miss only: its ray must hit something well inside [near, far) in both references
            assert i64[0, 0] >= 0 and 2 * rec[14] < d64[0, 0] < 0.5 * rec[15] and abs(d32[0, 0] - d64[0, 0]) < 1e-4
        terrain = np.isin(i64, DR.TERRAIN_IDS)
        if terrain.any() and w * h > 1:
            seen_terrain += 1
            assert (terrain & keep).any(), (kind, name, e, label)
        assert DR.accepts(d64.astype(np.float32), d64, i64, d32, keep, rec[15])[0]       # the reference passes its own rule
        if not flags & DR.SEE_ROBOT:
            assert not RR.is_robot(i64).any()
        assert not (i64 == RR.ID_TARGET).any()                                            # the walk target is never seen
        if label == DR.BACK:
            assert (i64 == RR.ID_HEIGHTFIELD).mean() > 0.2                                # turned round, the border and outside bases see the grid
    print("worst image keeps", worst)
    assert seen_terrain >= 0.8 * len(DR.compared_images())                                # the camera looks at the ground
