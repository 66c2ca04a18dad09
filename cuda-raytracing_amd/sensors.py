"""Direction tables for Sensor (pure numpy): one camera-space direction per pixel, [height, width, 3] float32 unit vectors in the
convention of "sensor frames" in include/rt_hip.h -- +y the optical axis, +x image right, +z image up.  Row 0 is the top of the
image, column 0 its left edge, samples at pixel centres.

Conveniences: they promise the geometry their docstrings state to float32 rounding, not a bit pattern (the library's promise is the
rule of rt_hip.h for whatever table it is given).  Every generator takes with_mask=False; with_mask=True returns (directions, valid),
valid [height, width] bool: the pixels the model can see.  The others hold FALLBACK, a finite direction that renders like any other.
"""
import math

import numpy as np

FALLBACK = (0.0, 1.0, 0.0)                  # what a pixel the model cannot see looks along: the optical axis


def _finish(d, valid, with_mask):
    d = np.asarray(d, np.float64)
    n = np.linalg.norm(d, axis=-1, keepdims=True)
    valid = valid & np.isfinite(d).all(-1) & (n[..., 0] > 0)
    d = np.where(valid[..., None], d / np.where(n > 0, n, 1.0), np.asarray(FALLBACK))
    d = np.ascontiguousarray(d, np.float32)
    return (d, valid) if with_mask else d


def _angles(az, el):
    """azimuth to the RIGHT of the optical axis, elevation UP from the x-y plane -> unit vectors"""
    return np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el) + 0.0 * az], -1)


def equirectangular(width, height, azimuth=(-math.pi, math.pi), elevation=(-math.pi / 2, math.pi / 2), with_mask=False):
    """A panorama: column x looks azimuth[0] + (x + 0.5) / width * (azimuth[1] - azimuth[0]) to the right of +y (azimuth increases
    with x, towards +x), row y looks elevation[1] - (y + 0.5) / height * (elevation[1] - elevation[0]) above the x-y plane (elevation
    DEcreases with y: row 0 is the top).  Every pixel is valid."""
    az = azimuth[0] + (np.arange(width) + 0.5) / width * (azimuth[1] - azimuth[0])
    el = elevation[1] - (np.arange(height) + 0.5) / height * (elevation[1] - elevation[0])
    d = _angles(az[None, :], el[:, None])
    return _finish(d, np.ones((height, width), bool), with_mask)


def spinning_lidar(elevations, azimuth_steps, azimuth=(-math.pi, math.pi), with_mask=False):
    """A spinning lidar: one ROW per beam, of the constant elevation (radians above the x-y plane) elevations[row]; column k looks
    azimuth[0] + (k + 0.5) / azimuth_steps * (azimuth[1] - azimuth[0]) to the right of +y.  Every pixel is valid."""
    el = np.asarray(elevations, np.float64).reshape(-1)
    az = azimuth[0] + (np.arange(azimuth_steps) + 0.5) / azimuth_steps * (azimuth[1] - azimuth[0])
    d = _angles(az[None, :], el[:, None])
    return _finish(d, np.ones((el.size, azimuth_steps), bool), with_mask)


def fisheye_equidistant(width, height, fov, centre=None, with_mask=False):
    """An equidistant fisheye (r = f * theta) whose image circle touches the nearer pair of image edges: a pixel centre at distance r
    from `centre` (default the image's middle, (width / 2, height / 2) in the frame where pixel (x, y) has its centre at
    (x + 0.5, y + 0.5)) looks theta = r / R * fov / 2 off the optical axis, R = min(width, height) / 2, towards the pixel's side
    (right of centre -> +x, above centre -> +z).  Pixels outside the image circle are invalid and hold FALLBACK."""
    cx, cy = (width / 2.0, height / 2.0) if centre is None else centre
    u = (np.arange(width) + 0.5 - cx)[None, :] + np.zeros((height, 1))
    v = (np.arange(height) + 0.5 - cy)[:, None] + np.zeros((1, width))
    r = np.hypot(u, v)
    R = min(width, height) / 2.0
    theta = r / R * (fov / 2.0)
    s = np.where(r > 0, np.sin(theta) / np.where(r > 0, r, 1.0), 0.0)
    d = np.stack([s * u, np.cos(theta), -s * v], -1)
    return _finish(d, r <= R, with_mask)


def rolling_poses(start, end, slices):
    """The poses of one rolling frame (Sensor.render_rolling): float32 [slices, 6], slice s at start + (end - start) * s / slices of the
    six numbers (x, y, z, yaw, pitch, roll) -- slice 0 fires at `start`, the slice after the last would fire at `end`, which is the
    next frame's start.  Computed in float64 and rounded to float32 once.  A plain interpolation of the six numbers: adequate for the
    small rotations of one sweep or one exposure, NOT a slerp -- for large rotations interpolate the rotations yourself."""
    a, b = np.asarray(start, np.float64), np.asarray(end, np.float64)
    if a.shape != (6,) or b.shape != (6,) or int(slices) != slices or slices < 1:
        raise ValueError("start and end must be (x, y, z, yaw, pitch, roll) and slices a positive integer, got %s, %s, %r" % (a.shape, b.shape, slices))
    s = np.arange(int(slices), dtype=np.float64)[:, None]
    return np.ascontiguousarray(a[None] + (b - a)[None] * s / float(slices), np.float32)


BROWN_CONRADY_ITERATIONS = 20


def brown_conrady_distort(xn, yn, dist):
    """the forward model (OpenCV's): normalised undistorted (xn, yn) -> normalised distorted coordinates"""
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    r2 = xn * xn + yn * yn
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return (xn * radial + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn),
            yn * radial + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn)


def brown_conrady(width, height, K, dist, with_mask=False):
    """A calibrated camera in the Brown-Conrady (OpenCV) model: K the 3x3 intrinsic matrix, dist = (k1, k2, p1, p2[, k3]).  Pixel
    (x, y) -- integer coordinates, as the reference's pinhole takes them -- goes through K^-1 to distorted normalised coordinates,
    which are undistorted by BROWN_CONRADY_ITERATIONS = 20 fixed-point iterations of OpenCV's undistortPoints scheme
    (x <- (xd - tangential(x)) / radial(x), started at xd), all in float64; the direction is (xn, 1, -yn), normalised.  A pixel is
    valid where the iteration has settled: distorting its result again lands within 1e-4 pixel of the pixel.  The others hold
    FALLBACK.  With dist all zero this is the plain pinhole K^-1 (x, y, 1), swizzled as raycast.cu:182 does and normalised."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Ki = np.linalg.inv(K)
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    p = np.einsum("ij,hwj->hwi", Ki, np.stack([x, y, np.ones_like(x)], -1))
    xd, yd = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    k1, k2, p1, p2 = [float(v) for v in dist[:4]]
    k3 = float(dist[4]) if len(dist) > 4 else 0.0
    xn, yn = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(BROWN_CONRADY_ITERATIONS):
            r2 = xn * xn + yn * yn
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            dx = 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
            dy = p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
            xn, yn = (xd - dx) / radial, (yd - dy) / radial
        bx, by = brown_conrady_distort(xn, yn, (k1, k2, p1, p2, k3))
        back = np.einsum("ij,hwj->hwi", K, np.stack([bx, by, np.ones_like(bx)], -1))
        err = np.hypot(back[..., 0] / back[..., 2] - x, back[..., 1] / back[..., 2] - y)
        valid = np.isfinite(err) & (err < 1e-4)
    d = np.stack([xn, np.ones_like(xn), -yn], -1)
    return _finish(np.where(valid[..., None], d, 0.0), valid, with_mask)
