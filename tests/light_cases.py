"""The light estimation stages' definitions (include/alvaar_hip.h: alva_light_bin B1-B5, alva_light_fuse F1-F3, alva_light_estimate E1-E5)
restated in numpy, operation for operation, and the analytic environments the tests run them on.  The reference has no light estimation,
so this file is what the three stages are pinned to (tests/test_light_cases.py checks the restatement against the sRGB curve, an analytic
projection and the blend's properties; tests/test_gpu_light.py the kernels against it, bit for bit).

Sums whose order the definition leaves open are integer sums; the geometry and the projection are float64 in the written order
(elementwise numpy does not contract a * b + c), so the GPU is compared with `==`."""
from __future__ import annotations

import functools
import math
import re
from pathlib import Path

import numpy as np

import depth_cases as Dc

F32 = np.float32
N, CELLS = 8, 384
ACC_WORDS, STATE_BYTES = 4 * CELLS + 8, 13 * CELLS + 32   # ALVA_LIGHT_ACC_WORDS, ALVA_LIGHT_STATE_BYTES
FRAME = 4 * CELLS                                        # the frame's words behind the cells'
STEP, MIN_PIXELS, W_NEW, W_MAX = 4, 64, 32, 224          # the system's constants (include/alvaar_system.h)
LUT_FILE = Path(__file__).resolve().parent.parent / "alvaar_amd" / "csrc" / "light_lut.inc"


@functools.lru_cache(maxsize=None)
def lut():
    """B1: the committed table, parsed from the file the kernel includes"""
    text = "\n".join(line for line in LUT_FILE.read_text().splitlines() if not line.lstrip().startswith("//"))
    vals = [int(v) for v in re.findall(r"\d+", text)]
    assert len(vals) == 256
    return np.array(vals, np.uint16)


def srgb_to_linear(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb8(v):
    """the 8-bit pixel value of a linear radiance in 0..1"""
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0)
    s = np.where(v <= 0.0031308, 12.92 * v, 1.055 * v ** (1.0 / 2.4) - 0.055)
    return np.clip(np.rint(255.0 * s), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- alva_light_bin
def cell_of(d0, d1, d2):
    """B4: the cell of every direction (int64, -1 for none)"""
    d = [np.asarray(v, np.float64) for v in (d0, d1, d2)]
    with np.errstate(all="ignore"):
        finite = np.isfinite(d[0]) & np.isfinite(d[1]) & np.isfinite(d[2])
        a0, a1, a2 = np.abs(d[0]), np.abs(d[1]), np.abs(d[2])
        axis = np.zeros(d[0].shape, np.int64)
        m = a0.copy()
        axis = np.where(a1 > m, 1, axis)
        m = np.where(a1 > m, a1, m)
        axis = np.where(a2 > m, 2, axis)
        m = np.where(a2 > m, a2, m)
        ok = finite & (m > 0.0)
        major = np.select([axis == 0, axis == 1], [d[0], d[1]], d[2])
        face = 2 * axis + (major < 0.0)
        a = np.where(axis == 0, d[1], d[0]) / m
        b = np.where(axis == 2, d[1], d[2]) / m
        fi = np.floor((a + 1.0) * 4.0)
        fj = np.floor((b + 1.0) * 4.0)
        i = np.minimum(N - 1, np.where(ok, fi, 0).astype(np.int64))
        j = np.minimum(N - 1, np.where(ok, fj, 0).astype(np.int64))
    return np.where(ok, (face * N + j) * N + i, -1)


def block_cells(calib8, R_wc9, step, gw, gh):
    """B3, B4: the cell of every block [gh,gw] and its direction dw [3][gh,gw]"""
    fx, fy, cx, cy = (np.float64(c) for c in calib8[:4])
    gy, gx = np.mgrid[0:gh, 0:gw]
    u = gx * step + step // 2
    v = gy * step + step // 2
    uu, vv = Dc.undistort(calib8, u.reshape(-1).astype(F32), v.reshape(-1).astype(F32))
    x, y = (uu.astype(np.float64) - cx) / fx, (vv.astype(np.float64) - cy) / fy
    R = np.asarray(R_wc9, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        dw = [(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * 1.0 for r in range(3)]
    return cell_of(*dw).reshape(gh, gw), [c.reshape(gh, gw) for c in dw]


def bin_frame(rgba, calib8, R_wc9, step, acc=None):
    """alva_light_bin: rgba [h,w,4] uint8 -> the accumulators uint64 [ACC_WORDS] (acc, when given, is added to and returned)"""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    acc = np.zeros(ACC_WORDS, np.uint64) if acc is None else acc
    gw, gh = w // step, h // step
    if gw == 0 or gh == 0:
        return acc
    px = rgba[:gh * step, :gw * step, :3]
    lin = lut()[px].astype(np.int64)                                                     # B1
    S = lin.reshape(gh, step, gw, step, 3).sum(axis=(1, 3))                              # B2 [gh,gw,3]
    sat = (px >= 250).any(axis=2).reshape(gh, step, gw, step).sum(axis=(1, 3))
    fr = [S[..., 0].sum(), S[..., 1].sum(), S[..., 2].sum(), gw * gh * step * step, sat.sum(), gw * gh]
    acc[FRAME:FRAME + 6] += np.array(fr, np.uint64)
    if R_wc9 is not None:
        cell, _ = block_cells(calib8, R_wc9, step, gw, gh)
        ok = cell >= 0
        add = np.zeros((CELLS, 4), np.int64)
        for k in range(3):
            np.add.at(add[:, k], cell[ok], S[..., k][ok])
        np.add.at(add[:, 3], cell[ok], step * step)
        acc[:FRAME] += add.reshape(-1).astype(np.uint64)                                 # B5
    return acc


# ---------------------------------------------------------------------------------------------------- the state
def empty_state():
    return dict(E=np.zeros((CELLS, 3), np.uint32), W=np.zeros(CELLS, np.uint8), latch=np.zeros(8, np.uint32))


def pack_state(st):
    b = np.concatenate([st["E"].astype("<u4").reshape(-1).view(np.uint8), st["W"].astype(np.uint8), st["latch"].astype("<u4").view(np.uint8)])
    assert b.size == STATE_BYTES
    return b


def unpack_state(b):
    b = np.ascontiguousarray(np.asarray(b, np.uint8).reshape(-1)[:STATE_BYTES])
    return dict(E=b[:12 * CELLS].view("<u4").reshape(CELLS, 3).copy(), W=b[12 * CELLS:13 * CELLS].copy(), latch=b[13 * CELLS:].view("<u4").copy())


# ---------------------------------------------------------------------------------------------------- alva_light_fuse
def fuse(acc, state, min_pixels=MIN_PIXELS, w_new=W_NEW, w_max=W_MAX):
    """alva_light_fuse: -> the new state (a fresh dict); acc is zeroed in place, as the kernel leaves it"""
    a = np.asarray(acc, np.uint64)[:FRAME].reshape(CELLS, 4).astype(object)   # Python integers: 64-bit products without wrap
    E, W, latch = state["E"].copy(), state["W"].copy(), state["latch"].copy()
    observed = touched = 0
    for c in range(CELLS):
        n = int(a[c, 3])
        touched += n > 0
        if n < min_pixels:                                                     # F1
            continue
        observed += 1
        w = int(W[c])
        for k in range(3):                                                     # F2
            m = int(a[c, k]) // n
            E[c, k] = (m if w == 0 else (int(E[c, k]) * w + m * w_new) // (w + w_new)) & 0xFFFFFFFF
        W[c] = w_new if w == 0 else min(w_max, w + w_new)
    f = [int(v) for v in np.asarray(acc, np.uint64)[FRAME:FRAME + 8]]
    if f[3] > 0:                                                               # F3
        latch[0], latch[1], latch[2] = f[0] // f[3], f[1] // f[3], f[2] // f[3]
        latch[3], latch[4], latch[5] = f[4], f[5], touched
        latch[7] += 1
    if observed:
        latch[6] += 1
    acc[:] = 0
    return dict(E=E, W=W, latch=latch)


# ---------------------------------------------------------------------------------------------------- alva_light_estimate
Y_LIT = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)


def sh_basis(x, y, z):
    """the nine basis polynomials of E2 at a unit direction (works on arrays)"""
    c0, c1, c2, c3, c4 = Y_LIT
    return [c0 + 0.0 * x, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3.0 * (z * z) - 1.0), c2 * (x * z), c4 * (x * x - y * y)]


@functools.lru_cache(maxsize=None)
def basis_table():
    """E2: [9, CELLS] float64, in Python floats (IEEE double, one operation at a time) in the written order"""
    pi = 3.141592653589793
    dirs, om, total = [], [], 0.0
    for cell in range(CELLS):
        face, j, i = cell // (N * N), (cell // N) % N, cell % N
        a, b = (2 * i + 1) / 8.0 - 1.0, (2 * j + 1) / 8.0 - 1.0
        r2 = (1.0 + a * a) + b * b
        r = math.sqrt(r2)
        axis = face >> 1
        d = [0.0, 0.0, 0.0]
        d[axis] = -1.0 if face & 1 else 1.0
        d[1 if axis == 0 else 0] = a
        d[1 if axis == 2 else 2] = b
        dirs.append([v / r for v in d])
        om.append(1.0 / (r2 * r))
        total += om[-1]
    scale = (4.0 * pi) / total
    T = np.zeros((9, CELLS))
    c0, c1, c2, c3, c4 = Y_LIT
    for cell in range(CELLS):
        w = om[cell] * scale
        x, y, z = dirs[cell]
        col = [w * c0, w * (c1 * y), w * (c1 * z), w * (c1 * x), w * (c2 * (x * y)), w * (c2 * (y * z)), w * (c3 * (3.0 * (z * z) - 1.0)),
               w * (c2 * (x * z)), w * (c4 * (x * x - y * y))]
        T[:, cell] = col
    return T


@functools.lru_cache(maxsize=None)
def cell_dirs():
    """the unit direction of every cell's centre [CELLS,3] (for the tests; the table holds the same directions)"""
    out = np.zeros((CELLS, 3))
    for cell in range(CELLS):
        face, j, i = cell // (N * N), (cell // N) % N, cell % N
        a, b = (2 * i + 1) / 8.0 - 1.0, (2 * j + 1) / 8.0 - 1.0
        axis = face >> 1
        d = np.zeros(3)
        d[axis] = -1.0 if face & 1 else 1.0
        d[1 if axis == 0 else 0] = a
        d[1 if axis == 2 else 2] = b
        out[cell] = d / np.linalg.norm(d)
    return out


def estimate(state):
    """alva_light_estimate -> (sh [9,3] float32, primary_dir [3], primary_rgb [3], ambient [4] float32, info [8] int32); also returns the
    doubles L [9,3] as a sixth value for the tests"""
    E, W, latch = state["E"], state["W"], [int(v) for v in state["latch"]]
    has = W > 0
    K = int(has.sum())
    A = [int(E[has, c].astype(np.uint64).sum()) // K for c in range(3)] if K else latch[:3]          # E1
    filled = np.where(has[:, None], E.astype(np.int64), np.array(A, np.int64)[None, :])
    v = filled.astype(np.float64) / 65535.0
    T = basis_table()
    x = np.zeros((64, 27))                                                                           # E3
    for j in range(CELLS // 64):
        cells = np.arange(64) + 64 * j
        for k in range(9):
            for c in range(3):
                x[:, 3 * k + c] += T[k, cells] * v[cells, c]
    for s in (32, 16, 8, 4, 2, 1):
        x[:s] += x[s:2 * s]
    L = x[0].reshape(9, 3).copy()
    code = 0 if K else (1 if latch[7] else 5)
    if not K:
        L[1:] = 0.0
    lum = [(0.2126 * L[k, 0] + 0.7152 * L[k, 1]) + 0.0722 * L[k, 2] for k in range(4)]                # E4
    g = (lum[3], lum[1], lum[2])
    gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    thr = 1e-3 * lum[0]
    valid = bool(K and gg > thr * thr)
    pd, pc = np.zeros(3, F32), np.zeros(3, F32)
    if valid:
        nrm = math.sqrt(gg)
        d = [g[0] / nrm, g[1] / nrm, g[2] / nrm]
        pd = np.array(d, np.float64).astype(F32)
        pc = np.array([max(0.0, ((L[3, c] * d[0] + L[1, c] * d[1]) + L[2, c] * d[2]) / 0.488603) for c in range(3)], np.float64).astype(F32)
    MR, MG, MB = latch[:3]                                                                           # E5
    amb = np.array([((13933 * MR + 46871 * MG + 4732 * MB) >> 16) / 65535.0, MR / MG if MG else 1.0, 1.0, MB / MG if MG else 1.0],
                   np.float64).astype(F32)
    info = np.array([code, K, latch[5], latch[4], latch[3], latch[6], int(valid), 0], np.int32)
    return L.astype(F32), pd, pc, amb, info, L


# ---------------------------------------------------------------------------------------------------- analytic environments
def rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def sphere_rotations():
    """camera-to-world rotations whose views (90 x 74 degrees) cover the sphere: eight yaws at three pitches, then up and down"""
    out = [rot_y(yaw) @ rot_x(pitch) for pitch in (-50, 0, 50) for yaw in range(0, 360, 45)]
    return out + [rot_x(90), rot_x(-90), rot_y(90) @ rot_x(90), rot_y(90) @ rot_x(-90)]


ENV_W, ENV_H, ENV_F = 128, 96, 64.0
ENV_CALIB = (ENV_F, ENV_F, ENV_W / 2, ENV_H / 2, 0.0, 0.0, 0.0, 0.0)
ENV_A, ENV_B, ENV_P = np.array([0.10, 0.12, 0.15]), np.array([0.80, 0.70, 0.50]), 4


def radiance(d, light):
    """a + b max(0, d . l)^p per channel, d [...,3] unit"""
    t = np.maximum(0.0, d @ np.asarray(light, np.float64))
    return ENV_A + ENV_B * (t ** ENV_P)[..., None]


def render_env(R_wc, light, width=ENV_W, height=ENV_H, f=ENV_F):
    """the frame a distortion-free camera with rotation R_wc sees of the environment: [h,w,4] uint8, sRGB-encoded"""
    v, u = np.mgrid[0:height, 0:width]
    dc = np.stack([(u - width / 2) / f, (v - height / 2) / f, np.ones(u.shape)], axis=-1)
    dw = dc @ np.asarray(R_wc, np.float64).T
    dw /= np.linalg.norm(dw, axis=-1, keepdims=True)
    rgba = np.full((height, width, 4), 255, np.uint8)
    rgba[..., :3] = linear_to_srgb8(radiance(dw, light))
    return rgba


def analytic_sh(light):
    """the projection of a + b max(0, d . l)^p on the nine basis functions [9,3] (Funk-Hecke: lambda_l Y_lm(l), lambda_l = 2 pi times the
    integral over 0..1 of t^p P_l(t))"""
    l = np.asarray(light, np.float64)
    p = ENV_P
    lam = [2 * math.pi / (p + 1), 2 * math.pi / (p + 2), math.pi * (3.0 / (p + 3) - 1.0 / (p + 1))]
    Y = np.array(sh_basis(*l), np.float64)
    band = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
    out = np.array([lam[band[k]] * Y[k] for k in range(9)])[:, None] * ENV_B[None, :]
    out[0] += ENV_A * 4 * math.pi * Y_LIT[0]
    return out


def run_session(frames_R, light, fuse_kw=None):
    """every (frame, rotation) binned and fused in turn -> the state"""
    st = empty_state()
    for R in frames_R:
        acc = bin_frame(render_env(R, light), ENV_CALIB, R.reshape(-1), STEP)
        st = fuse(acc, st, **(fuse_kw or {}))
    return st


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


LIGHTS = {"oblique": unit([0.3, -0.8, 0.52]), "face_centre": unit([0.0, 0.0, 1.0]), "cube_edge": unit([1.0, 1.0, 0.0])}
