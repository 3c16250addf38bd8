"""Exteroception for the policy: point patterns of the terrain height scan (include/mocca.h mocca_height_scan, VecEnv.height_scan) and
the mount of the egocentric depth camera (mocca_depth_camera, VecEnv.depth_camera).

A pattern is a float32 array [P, 2] of points (x, y) in metres in the robot's heading frame: x ahead, y to the left.  No numpy-only
fallback lives here: the scan itself is the HIP kernel of csrc/mocca_scan.hip, the camera that of csrc/mocca_depth.hip.
"""
from __future__ import annotations

import numpy as np

SCAN_MAX_POINTS = 256   # MOCCA_SCAN_MAX_POINTS
DEPTH_MAX_PIXELS, DEPTH_MAX_SIDE, DEPTH_STABILISED, DEPTH_SEE_ROBOT = 256, 64, 1, 2   # MOCCA_DEPTH_*


def scan_grid(x_range, y_range, nx: int, ny: int) -> np.ndarray:
    """A regular grid of nx x ny points over [x_range[0], x_range[1]] x [y_range[0], y_range[1]] (both ends included; a single point along
    an axis sits at the range's start).  Returns float32 [nx * ny, 2], x-major: row ix * ny + iy is (x[ix], y[iy]) -- the scan of one env
    reshapes to [nx, ny] with x (ahead) along the first axis and y (to the left) along the second."""
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1:
        raise ValueError("scan_grid: nx and ny must be at least 1")
    if nx * ny > SCAN_MAX_POINTS:
        raise ValueError(f"scan_grid: at most {SCAN_MAX_POINTS} points")
    xs = np.linspace(float(x_range[0]), float(x_range[1]), nx)
    ys = np.linspace(float(y_range[0]), float(y_range[1]), ny)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1).astype(np.float32)


class DepthCamera:
    """The depth camera of one handle: a pinhole on link `body` (0: the base), its eye `offset` (x, y, z, metres) in the link's frame.
    `yaw`, `pitch`, `roll` in degrees with render.Camera's signs -- yaw about the mount's +z counted from +x, a NEGATIVE pitch looks down --
    and `fov_y` in degrees; `width` x `height` pixels (each 1 .. 64, at most 256 together); depths in [near, far) metres, `far` where
    nothing is.  `stabilised`: the orientation follows the base's heading only (R_z(yaw) of the height scan) instead of the link's full
    rotation; `see_robot`: the robot's own geoms (or skeleton) occlude."""

    def __init__(self, body: int = 0, offset=(0.0, 0.0, 0.0), yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, width: int = 16,
                 height: int = 12, fov_y: float = 60.0, near: float = 0.05, far: float = 10.0, stabilised: bool = False, see_robot: bool = False):
        self.body, self.offset = int(body), tuple(float(v) for v in offset)
        self.yaw, self.pitch, self.roll = float(yaw), float(pitch), float(roll)
        self.width, self.height, self.fov_y, self.near, self.far = int(width), int(height), float(fov_y), float(near), float(far)
        self.stabilised, self.see_robot = bool(stabilised), bool(see_robot)
        if len(self.offset) != 3 or not all(np.isfinite(self.offset + (self.yaw, self.pitch, self.roll))):
            raise ValueError("DepthCamera: offset is three finite numbers, the angles are finite")
        if self.body < 0:
            raise ValueError("DepthCamera: body is a link index, 0 the base")
        if not (1 <= self.width <= DEPTH_MAX_SIDE and 1 <= self.height <= DEPTH_MAX_SIDE and self.width * self.height <= DEPTH_MAX_PIXELS):
            raise ValueError(f"DepthCamera: width and height are 1 .. {DEPTH_MAX_SIDE}, at most {DEPTH_MAX_PIXELS} pixels together")
        if not 0.0 < self.fov_y < 180.0:
            raise ValueError("DepthCamera: fov_y lies in (0, 180) degrees")
        if not (np.isfinite(self.near) and np.isfinite(self.far) and 0.0 < self.near < self.far):
            raise ValueError("DepthCamera: needs finite 0 < near < far")

    @property
    def shape(self):
        """(height, width): what one env's row reshapes to"""
        return self.height, self.width

    @property
    def sagittal(self) -> bool:
        """the camera lies in the robot's plane of symmetry: on the base, no sideways offset, no yaw, no roll -- the mirrored robot in the
        mirrored world then sees the column-flipped image"""
        return self.body == 0 and self.offset[1] == 0.0 and self.yaw == 0.0 and self.roll == 0.0

    def pack(self) -> dict:
        """mocca_set_depth_camera's arguments: body, mount float32 [6] (offset, then roll, pitch, yaw in RADIANS with the ABI's signs: a
        positive pitch looks down), width, height, fov_y in radians, near, far, flags"""
        mount = np.array([*self.offset, np.deg2rad(self.roll), -np.deg2rad(self.pitch), np.deg2rad(self.yaw)], np.float32)
        flags = (DEPTH_STABILISED if self.stabilised else 0) | (DEPTH_SEE_ROBOT if self.see_robot else 0)
        return dict(body=self.body, mount=mount, width=self.width, height=self.height, fov_y=float(np.deg2rad(self.fov_y)), near=self.near,
                    far=self.far, flags=flags)
