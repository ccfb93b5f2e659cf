"""The scene volume's shift (include/alvaar_hip.h: alva_mesh_shift S1-S4) and the session's follow rule (include/alvaar_system.h: V1-V4)
restated in numpy / plain Python, and the case table.  The reference has no scene mesh, so this file is what the stage and the rule are
pinned to (tests/test_mesh_shift_cases.py checks the restatement against a naive triple loop, its own properties and the extraction's
world invariance; tests/test_gpu_mesh_shift.py the kernel against it, byte for byte).

Nothing is resampled and the counts are integer sums, so the GPU is compared with `==`."""
from __future__ import annotations

import functools
import math

import numpy as np

import mesh_cases as Mc

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
W_VALUES = np.array([0, 1, 127, 128, 255], np.uint8)
FOLLOW_MAX_SHIFT = 1 << 24   # ALVA_MESH_FOLLOW_MAX_SHIFT
FOLLOW_BLOCKS = (1, 2, 4, 8, 16, 32)


# ---------------------------------------------------------------------------------------------------- alva_mesh_shift
def shift(q, w, c, s):
    """alva_mesh_shift with slices.  q int16, w uint8 [N,N,N] (index [k][j][i]), c uint8 [N,N,N,4] or None, s = (s_x, s_y, s_z), any
    Python ints.  Returns (q2, w2, c2 or None, info [8] int32)."""
    q, w = np.asarray(q, np.int16), np.asarray(w, np.uint8)
    N = q.shape[0]
    s = [int(v) for v in s]
    q2, w2 = np.zeros_like(q), np.zeros_like(w)
    c2 = None if c is None else np.zeros_like(c)
    info = np.zeros(8, np.int64)
    info[7] = N
    weighted = int((w > 0).sum())
    if all(-N < v < N for v in s):   # S3, before any index is formed
        # S1, S2: per axis the destination range [d0, d1) whose source d + s lies in [0, N)
        dst = tuple(slice(max(0, -v), min(N, N - v)) for v in reversed(s))   # arrays are [k][j][i]: z first
        src = tuple(slice(max(0, v), min(N, N + v)) for v in reversed(s))
        q2[dst], w2[dst] = q[src], w[src]
        if c is not None:
            c2[dst] = c[src]
            info[3] = int((c[src][..., 3] > 0).sum())
        info[0] = q[src].size
        info[1] = int((w[src] > 0).sum())
    info[2] = weighted - info[1]   # S4: what the shift lost
    return q2, w2, c2, info.astype(np.int32)


def shift_naive(q, w, c, s):
    """S1 - S4 as a triple loop over the destination, for small N"""
    N = q.shape[0]
    q2, w2 = np.zeros_like(q), np.zeros_like(w)
    c2 = None if c is None else np.zeros_like(c)
    copied = kept = colored = 0
    none = any(abs(int(v)) >= N for v in s)
    for k in range(N):
        for j in range(N):
            for i in range(N):
                if none:
                    continue
                si, sj, sk = i + int(s[0]), j + int(s[1]), k + int(s[2])
                if 0 <= si < N and 0 <= sj < N and 0 <= sk < N:
                    q2[k, j, i], w2[k, j, i] = q[sk, sj, si], w[sk, sj, si]
                    copied += 1
                    kept += int(w[sk, sj, si] > 0)
                    if c is not None:
                        c2[k, j, i] = c[sk, sj, si]
                        colored += int(c[sk, sj, si, 3] > 0)
    return q2, w2, c2, np.array([copied, kept, int((w > 0).sum()) - kept, colored, 0, 0, 0, N], np.int32)


def case_volume(N, seed):
    """a hashed volume: q over its full int16 range (-32768 too), w in {0, 1, 127, 128, 255}, every colour byte hashed with a colour
    weight that is zero in about a quarter of the voxels"""
    q, _ = Mc.hashed_volume(N, seed, q_lo=-32768, q_hi=32767)
    n = N * N * N
    w = W_VALUES[Mc.hashed(n, seed + 1) % 5].reshape(N, N, N)
    c = (Mc.hashed(4 * n, seed + 2) % 256).astype(np.uint8).reshape(N, N, N, 4)
    c[..., 3] = np.where((Mc.hashed(n, seed + 3) % 4 == 0).reshape(N, N, N), 0, c[..., 3])
    # the extremes, planted at the corners and in the middle (a hash of 64 values need not hit them)
    mid = n // 2 + N // 2
    q.reshape(-1)[[0, mid, n - 1]] = (-32768, 32767, -32768)
    w.reshape(-1)[[0, mid, n - 1]] = (255, 1, 128)
    c.reshape(-1, 4)[[0, mid, n - 1]] = ((255, 0, 255, 255), (0, 255, 0, 1), (1, 2, 3, 255))
    return q, w, c


def case_shifts(N):
    """the shifts of the table for one N: (name, s)"""
    out = [("zero", (0, 0, 0))]
    for a, ax in enumerate("xyz"):
        for sign in (1, -1):
            for m in (1, 8, 16):
                s = [0, 0, 0]
                s[a] = sign * m
                out.append((f"{ax}{sign * m:+d}", tuple(s)))
    out += [("mixed_3_-5_8", (3, -5, 8)), ("mixed_-8_16_0", (-8, 16, 0))]
    for a, ax in enumerate("xyz"):   # near-total: one plane survives, none, none
        for m, name in ((N - 1, "N-1"), (N, "N"), (N + 1, "N+1")):
            s = [0, 0, 0]
            s[a] = m if a != 1 else -m
            out.append((f"{ax}_{name}", tuple(s)))
    out += [("int_max_x", (INT_MAX, 0, 0)), ("int_min_y", (0, INT_MIN, 0)), ("extreme_all", (INT_MIN, INT_MAX, INT_MIN))]
    return out


CASE_N = (4, 8, 16, 32, 65, 81)


@functools.lru_cache(maxsize=None)
def volumes():
    return {N: case_volume(N, 100 + N) for N in CASE_N}


def cases():
    """(id, N, s) for every case of the table; each is run with and without colour"""
    return [(f"N{N}-{name}", N, s) for N in CASE_N for name, s in case_shifts(N)]


@functools.lru_cache(maxsize=None)
def expected(N, s):
    """the restatement's answer for a table case, computed once (read-only)"""
    q, w, c = volumes()[N]
    out = shift(q, w, c, s)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- the follow rule
# The session test (tests/test_gpu_mesh_follow_system.py) runs the stream of tests/test_gpu_mesh_system.py -- view 3 k at frame k, an
# update on every fifth frame -- with this extent and block.  At rel_extent 1 the cube's side is the plane's depth, about 4 units of
# the stream, a voxel 1/8; the camera's x swings from about +0.85 to -0.9, about 14 voxels, so a block of 2 voxels shifts many times
# (tests/test_mesh_shift_cases.py counts them on synth.plane_camera_pose)
STREAM_EXTENT, STREAM_BLOCK, STREAM_RES, STREAM_SPEED, STREAM_EVERY, STREAM_TRACKED = 1.0, 2, 32, 3, 5, 110


def stream_shifts(k_place, plane_z=4.0):
    """the rule on the stream's analytic poses, the volume placed at frame k_place -> the list of (frame, shift) that are not zero"""
    from alvaar_amd import synth
    R, t = synth.plane_camera_pose(STREAM_SPEED * k_place)
    m0 = plane_z - t[2]
    side = STREAM_EXTENT * m0
    voxel = side / STREAM_RES
    origin0 = np.array(follow_target(t, R, m0)) - side / 2
    offset, out = np.zeros(3, np.int64), []
    for k in range(k_place + STREAM_EVERY, STREAM_TRACKED, STREAM_EVERY):
        R, t = synth.plane_camera_pose(STREAM_SPEED * k)
        s = follow_shift(follow_target(t, R, m0), follow_origin(origin0, offset, voxel), side, voxel, STREAM_BLOCK)
        if any(s):
            offset += np.array(s)
            out.append((k, s))
    return out


def follow_shift(centre, origin, side, voxel, block):
    """V2, V3: the shift (s_x, s_y, s_z) in voxels that brings the volume's centre within a block of `centre`"""
    s = []
    lim = float(FOLLOW_MAX_SHIFT // block)
    for i in range(3):
        d = (np.float64(centre[i]) - (np.float64(origin[i]) + np.float64(side) / 2)) / np.float64(voxel)   # V2
        b = float(np.trunc(d / np.float64(block))) if math.isfinite(d) else 0.0   # V3
        b = min(max(b, -lim), lim)
        s.append(block * int(b))
    return tuple(s)


def follow_target(t_wc, R_wc, m0):
    """V1: the placement's own expression, with the placement's m0"""
    R = np.asarray(R_wc, np.float64).reshape(3, 3)
    return tuple(np.float64(t_wc[i]) + np.float64(m0) * R[i, 2] for i in range(3))


def follow_origin(origin0, offset, voxel):
    """origin0 + (double) offset voxel, afresh from the integers"""
    return np.array([np.float64(origin0[i]) + np.float64(int(offset[i])) * np.float64(voxel) for i in range(3)], np.float64)
