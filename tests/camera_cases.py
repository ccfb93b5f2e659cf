"""TEST INFRASTRUCTURE: camera-model cases for camera_device.hpp's alva_undistort_dev / alva_project_dist_dev (through alva_undistort_points and
alva_project_dist) -- coefficient sets, a pixel table, a projection table and a numpy restatement of the undistortion loop that also
reports at which iteration a pixel leaves through `icdist < 0`.  test_camera_cases.py (CPU) asserts what the tables reach;
test_gpu_camera_cases.py runs them on the GPU against the oracle, bit for bit.

  OLD_DISTS   the four sets of test_distortion.py: icdist stays positive on every pixel of the table
  NEW_DISTS   three sets whose radial polynomial 1 + k1 r^2 + k2 r^4 turns negative inside the image: the early exit resets x, y to the
              undistorted-from pixel and stops.  A pixel beyond the polynomial's root leaves at iteration 0; a pixel inside it can be
              thrown beyond the root by its first update and leaves at iteration 1 or later, with other x, y left behind.
  pixels()    random pixels of test_distortion.py's range, rings around the principal point at radii on both sides of every root, the
              principal point and the corners
  points()    camera-frame points with Z = 0, Z < 0, Z tiny, infinite or NaN coordinates, X / Z beyond the float range, among ordinary ones"""
from __future__ import annotations

import functools

import numpy as np

K = (520.0, 515.0, 318.5, 241.25)
OLD_DISTS = ((0, 0, 0, 0), (-0.28, 0.07, 0.0002, -0.0003), (0.12, -0.05, 0.001, 0.002), (-0.9, 0.3, 0.01, 0.01))
NEW_DISTS = ((-3, 0, 0, 0), (-2.5, 0.4, 0.001, -0.002), (-6, 0, 0, 0))
DISTS = OLD_DISTS + NEW_DISTS
PROJ_DISTS = (OLD_DISTS[1], NEW_DISTS[1])
SIZES = (1, 255, 256, 257)          # 256-thread blocks
GOLDEN_PIXELS = slice(0, None, 4)   # the reference pin records every fourth pixel
GOLDEN_POINTS = slice(3, 403, 2)    # ... and 200 points, every special row among them


def dist_id(d):
    return ",".join(f"{v:g}" for v in d)


def restate_undistort(px, K, dist):
    """orc_undistort_points in numpy: (out [n,2] f32, exit_at [n]: the iteration whose icdist was negative, -1 where none was)"""
    fx, fy, cx, cy = (float(v) for v in K)
    k1, k2, p1, p2 = (float(v) for v in dist)
    px = np.asarray(px, np.float32)
    ifx, ify = 1. / fx, 1. / fy
    u, v = px[:, 0].astype(np.float64), px[:, 1].astype(np.float64)
    x, y = (u - cx) * ifx, (v - cy) * ify
    x0, y0 = x.copy(), y.copy()
    exit_at, live = np.full(len(px), -1), np.ones(len(px), bool)
    with np.errstate(all="ignore"):
        for j in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((0 * r2 + k2) * r2 + k1) * r2)
            out = live & (icdist < 0)
            exit_at[out] = j
            x[out], y[out] = x0[out], y0[out]
            live &= ~out
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + 0 * r2 + 0 * r2 * r2
            x, y = np.where(live, (x0 - dx) * icdist, x), np.where(live, (y0 - dy) * icdist, y)
        xx, yy, ww = fx * x + 0 * y + cx, 0 * x + fy * y + cy, 1. / (0 * x + 0 * y + 1)
        return np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], 1), exit_at


RING_RADII = np.round(np.arange(0.04, 1.0001, 0.04), 2)    # normalised radius; the roots of the new sets lie at 0.41, 0.58 and 0.65
RING_DIRS = 16


@functools.lru_cache(maxsize=None)
def pixels():
    """[n, 2] f32, read-only; the first RING rows are the rings (radius-major), then the fixed pixels, then the random ones"""
    rng = np.random.RandomState(77)
    ang = (np.arange(RING_DIRS) + 0.25) * (2 * np.pi / RING_DIRS)
    ring = np.array([[K[2] + K[0] * r * np.cos(a), K[3] + K[1] * r * np.sin(a)] for r in RING_RADII for a in ang])
    fixed = np.array([[K[2], K[3]], [0, 0], [639, 0], [0, 479], [639, 479], [-40, -40], [680, 520], [318, 241], [319, 242]])
    rand = rng.uniform(-40, [680, 520], (1500, 2))
    px = np.ascontiguousarray(np.concatenate([ring, fixed, rand]).astype(np.float32))
    px.setflags(write=False)
    return px


N_RING = len(RING_RADII) * RING_DIRS


def identity_rows():
    """the pixels that zero distortion must return unchanged: both coordinates at least 2^-20 in size, where half a float ulp (2^-45 and
    up) is above the 1e-13 that the trip through the normalised plane can be off by in double"""
    return (np.abs(pixels()) >= 2.0 ** -20).all(1)

# (X, Y, Z) rows that leave the ordinary range, by what they feed the projection
SPECIAL_POINTS = (
    ("Z=0", (0.3, -0.2, 0.0)), ("Z=0,X=0", (0.0, 0.1, 0.0)), ("Z=-0", (0.3, 0.2, -0.0)), ("Z=-2", (0.5, 0.25, -2.0)), ("Z=-2,X<0", (-0.5, -0.25, -2.0)),
    ("Z=1e-300", (0.1, 0.2, 1e-300)), ("Z=1e-300,X=0", (0.0, 0.0, 1e-300)), ("X=1e300", (1e300, 0.5, 2.0)), ("Y=-1e300", (0.5, -1e300, 2.0)),
    ("X=1e39", (1e39, 0.5, 1.0)), ("X=3e38", (3e38, 0.5, 1.0)), ("X=1e10", (1e10, 2e9, 1.0)), ("X=1e25", (1e25, 1.0, 1.0)),
    ("X=1e60,Z=1e30", (1e60, 1.0, 1e30)), ("X=NaN", (np.nan, 0.5, 2.0)), ("Y=NaN", (0.5, np.nan, 2.0)), ("Z=NaN", (0.5, 0.5, np.nan)),
    ("Z=+inf", (0.5, 0.5, np.inf)), ("Z=-inf", (0.5, 0.5, -np.inf)), ("X=inf", (np.inf, 0.5, 2.0)), ("X=inf,Z=inf", (np.inf, 0.5, np.inf)),
    ("X=1e-40", (1e-40, -1e-44, 1.0)), ("origin", (0.0, 0.0, 0.0)), ("axis", (0.0, 0.0, 3.0)),
)


@functools.lru_cache(maxsize=None)
def points():
    """[n, 3] f64, read-only: the special rows spread among ordinary points (every tenth row from row 3 on), then ordinary points only"""
    rng = np.random.RandomState(78)
    n = 2000
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 9, n)], 1)
    P[special_rows()] = np.array([p for _, p in SPECIAL_POINTS])
    P.setflags(write=False)
    return P


def special_rows():
    return 3 + 10 * np.arange(len(SPECIAL_POINTS))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """float32 arrays bit for bit, except that where b is NaN a must be NaN (any sign and payload)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))


@functools.lru_cache(maxsize=None)
def oracle_undistort(dist):
    from oracles import orc_undistort_points
    out = orc_undistort_points(pixels(), K, dist)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_project(dist):
    from oracles import orc_project_dist
    out = orc_project_dist(points(), K, dist)
    out.setflags(write=False)
    return out
