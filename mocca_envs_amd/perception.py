"""Exteroception for the policy: point patterns of the terrain height scan (include/mocca.h mocca_height_scan, VecEnv.height_scan).

A pattern is a float32 array [P, 2] of points (x, y) in metres in the robot's heading frame: x ahead, y to the left.  No numpy-only
fallback lives here: the scan itself is the HIP kernel of csrc/mocca_scan.hip.
"""
from __future__ import annotations

import numpy as np

SCAN_MAX_POINTS = 256   # MOCCA_SCAN_MAX_POINTS


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
