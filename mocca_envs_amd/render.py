"""Cameras for `VecEnv.render()` (include/mocca.h mocca_render).

`Camera` is the reference's follow camera (bullet_utils.py:383-418: dist 2.5, yaw 0, pitch -5, a target that trails the robot with
smoothing (1, 1, 0.1)) with the projection of EnvBase.render (env_base.py:141-146: FOV 60, near 0.1, far 100).  Angles are in
degrees.  Yaw is counted from +x about +z: yaw 0, pitch 0 looks along +x with +z up; a negative pitch looks down from above.
"""
from __future__ import annotations

import numpy as np

from .lib import CAMERA_FLOATS

# the reference's image size (env_base.py _render_width / _render_height)
RENDER_WIDTH, RENDER_HEIGHT = 960, 720


def camera_axes(yaw_deg, pitch_deg):
    """(right, up, forward) of the pinhole, each [..., 3]; works on numpy arrays and on torch tensors (pass radians-free degrees)."""
    y, p = np.deg2rad(np.asarray(yaw_deg, np.float64)), np.deg2rad(np.asarray(pitch_deg, np.float64))
    cy, sy, cp, sp = np.cos(y), np.sin(y), np.cos(p), np.sin(p)
    forward = np.stack([cp * cy, cp * sy, sp], -1)
    up = np.stack([-sp * cy, -sp * sy, cp], -1)
    right = np.stack([sy, -cy, np.zeros_like(sy)], -1)      # forward x up
    return right, up, forward


class Camera:
    def __init__(self, yaw=0.0, pitch=-5.0, dist=2.5, fov=60.0, near=0.1, far=100.0):
        self.yaw, self.pitch, self.dist, self.fov, self.near, self.far = float(yaw), float(pitch), float(dist), float(fov), float(near), float(far)
        self.target = np.zeros(3)
        self._coef = np.array([1.0, 1.0, 0.1])      # bullet_utils.py:390

    def lookat(self, pos):
        """Camera.lookat (bullet_utils.py:414-418): the target jumps to pos."""
        self.target = np.asarray(pos, np.float64).copy()

    def track(self, pos, smooth_coef=None):
        """Camera.track (bullet_utils.py:398-412): target <- (1 - c) target + c pos, per component; default c = (1, 1, 0.1)."""
        c = self._coef if smooth_coef is None else np.asarray(smooth_coef, np.float64)
        assert (c <= 1).all(), "Invalid camera smoothing parameters"
        self.target = (1 - c) * self.target + c * np.asarray(pos, np.float64)

    @property
    def eye(self):
        return self.target - self.dist * camera_axes(self.yaw, self.pitch)[2]

    def pack(self, aspect=RENDER_WIDTH / RENDER_HEIGHT) -> np.ndarray:
        """The MOCCA_CAMERA_FLOATS record: eye, right, up, forward, tan(fov_y / 2), aspect, near, far (float32)."""
        right, up, forward = camera_axes(self.yaw, self.pitch)
        out = np.concatenate([self.target - self.dist * forward, right, up, forward,
                              [np.tan(np.deg2rad(self.fov) / 2), aspect, self.near, self.far]]).astype(np.float32)
        assert out.size == CAMERA_FLOATS
        return out


def follow_cameras(base_pos, aspect, camera: Camera = None):
    """One record per row of base_pos ([K, 3] torch tensor on the device): `camera` (default Camera()) looking at each position.
    Built with torch operations on the positions' device; nothing comes to the host."""
    import torch
    cam = Camera() if camera is None else camera
    rec = torch.from_numpy(cam.pack(aspect)).to(base_pos.device).repeat(base_pos.shape[0], 1)
    forward = rec[:, 9:12]
    rec[:, 0:3] = base_pos.to(torch.float32) - cam.dist * forward
    return rec.contiguous()
