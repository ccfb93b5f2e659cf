"""The volume raycast's definition (include/alvaar_hip.h: alva_mesh_raycast / alva_mesh_raycast_pixels, R0-R8) restated in numpy,
operation for operation, and the case table.  The reference has no raycast, so this file is what the two stages are pinned to
(tests/test_raycast_cases.py checks the restatement against analytic surfaces; tests/test_gpu_mesh_raycast.py the kernel against it, bit
for bit).

As in tests/mesh_cases.py the geometry is float64 in the definition's operation order (elementwise numpy does not contract a * b + c)
and everything from R3's fractions on is an integer, so the GPU is compared with `==`.  Vectorised over the rays, a loop over n."""
from __future__ import annotations

import functools

import numpy as np

import depth_cases as Dc
import mesh_cases as Mc

F32 = np.float32
MIN_COS = 0.0872   # the hit test's grazing gate


def _clamp_int(v, lo, hi):
    """a double clamped to lo..hi and converted; a NaN gives lo (the clamp comes first, as in the kernel)"""
    return np.where(v >= float(hi), float(hi), np.where(v >= float(lo), v, float(lo))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- R0 - R6
def march(q, w, origin3, voxel, min_weight, O, D, t_near=0.0, t_far=np.inf):
    """R0 - R6 for rays O, D [n,3] float64.  Returns a dict: t float32 [n], point, normal float32 [n,3], code uint8 [n], samples int [n],
    and for R7 and the tests nd float64 [n,3] (R6's quotient before the rounding), has_n bool [n], census (how often each branch of R4
    was taken, over all rays)."""
    q = np.asarray(q, np.int16)
    N = q.shape[0]
    qf = q.reshape(-1).astype(np.int64)
    wf = np.asarray(w, np.uint8).reshape(-1).astype(np.int64)
    o = np.asarray(origin3, np.float64).reshape(-1)
    voxel = np.float64(voxel)
    O, D = np.asarray(O, np.float64).reshape(-1, 3), np.asarray(D, np.float64).reshape(-1, 3)
    n_rays = len(O)
    census = dict(invalid=0, first=0, step=0, hit=0, behind=0, exhausted=0, hit_F0=0, prev_F0=0, normal0=0)
    with np.errstate(all="ignore"):
        # R0
        aD = np.abs(D)
        m01 = np.where(aD[:, 0] > aD[:, 1], aD[:, 0], aD[:, 1])
        dmax = np.where(m01 > aD[:, 2], m01, aD[:, 2])
        code4 = ~(np.isfinite(O).all(1) & np.isfinite(D).all(1)) | (dmax == 0.0)
        O = np.where(code4[:, None], 0.0, O)
        D = np.where(code4[:, None], np.array([1.0, 0.0, 0.0]), D)
        dmax = np.where(code4, 1.0, dmax)
        # R1
        t0, t1 = np.full(n_rays, np.float64(t_near)), np.full(n_rays, np.float64(t_far))
        code1 = np.zeros(n_rays, bool)
        for a in range(3):
            lo, hi = o[a] + 0.5 * voxel, o[a] + (np.float64(N) - 0.5) * voxel
            zero = D[:, a] == 0.0
            code1 |= zero & ~((lo <= O[:, a]) & (O[:, a] <= hi))
            Da = np.where(zero, 1.0, D[:, a])
            ta, tb = (lo - O[:, a]) / Da, (hi - O[:, a]) / Da
            tmin, tmax = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            t0 = np.where(zero, t0, np.where(t0 > tmin, t0, tmin))
            t1 = np.where(zero, t1, np.where(t1 < tmax, t1, tmax))
        code1 |= ~(t0 <= t1)
        # R2
        dt = (0.5 * voxel) / dmax
        code = np.where(code4, 4, np.where(code1, 1, 2)).astype(np.int64)
        live = ~(code4 | code1)
        have_prev = np.zeros(n_rays, bool)
        Fp = np.zeros(n_rays, np.int64)
        samples = np.zeros(n_rays, np.int64)
        t_hit = np.zeros(n_rays)
        g_hit = np.zeros((n_rays, 3), np.int64)
        for n in range(2 * N + 2):
            tn = t0 + np.float64(n) * dt
            gone = live & ~(tn <= t1)
            census["exhausted"] += int(gone.sum())
            live = live & (tn <= t1)
            if not live.any():
                break
            samples = np.where(live, n + 1, samples)
            # R3
            ic, f = [], []
            for a in range(3):
                P = O[:, a] + tn * D[:, a]
                g = (P - o[a]) / voxel - 0.5
                i = _clamp_int(np.floor(g), 0, N - 2)
                ic.append(i)
                f.append(_clamp_int(np.rint((g - i.astype(np.float64)) * 256.0), 0, 256))
            base = (ic[2] * N + ic[1]) * N + ic[0]
            corner = [base + (c & 1) + ((c >> 1) & 1) * N + (c >> 2) * N * N for c in range(8)]
            valid = functools.reduce(np.logical_and, [wf[c] >= min_weight for c in corner])
            qc = [qf[c] for c in corner]
            F = np.zeros(n_rays, np.int64)
            for c in range(8):
                wt = [f[a] if (c >> a) & 1 else 256 - f[a] for a in range(3)]
                F += qc[c] * wt[0] * wt[1] * wt[2]
            # R4
            seen = live & valid
            hit = seen & have_prev & (Fp > 0) & (F <= 0)
            behind = seen & have_prev & (Fp <= 0) & (F > 0)
            other = seen & ~hit & ~behind
            census["invalid"] += int((live & ~valid).sum())
            census["first"] += int((other & ~have_prev).sum())
            census["step"] += int((other & have_prev).sum())
            census["hit"] += int(hit.sum())
            census["behind"] += int(behind.sum())
            census["hit_F0"] += int((hit & (F == 0)).sum())
            census["prev_F0"] += int((seen & have_prev & (Fp == 0)).sum())
            # R5
            tp = t0 + np.float64(n - 1) * dt
            den = np.where(hit, Fp - F, 1)
            th = tp + dt * (Fp.astype(np.float64) / den.astype(np.float64))
            t_hit = np.where(hit, th, t_hit)
            # R6 (X4 on the hit sample's cell)
            for a in range(3):
                ga = sum(qc[c] if (c >> a) & 1 else -qc[c] for c in range(8))
                g_hit[:, a] = np.where(hit, ga, g_hit[:, a])
            code = np.where(hit, 0, np.where(behind, 3, code))
            have_prev = np.where(live & ~valid, False, np.where(other, True, have_prev))
            Fp = np.where(other, F, Fp)
            live = live & ~hit & ~behind
        census["exhausted"] += int(live.sum())   # (never for finite input: the loop's bound did not bind)
        is_hit = code == 0
        L2 = (g_hit[:, 0] * g_hit[:, 0] + g_hit[:, 1] * g_hit[:, 1]) + g_hit[:, 2] * g_hit[:, 2]
        has_n = is_hit & (L2 != 0)
        census["normal0"] = int((is_hit & (L2 == 0)).sum())
        length = np.sqrt(np.where(has_n, L2, 1).astype(np.float64))
        nd = np.where(has_n[:, None], g_hit.astype(np.float64) / length[:, None], 0.0)
        point = np.where(is_hit[:, None], (O + t_hit[:, None] * D).astype(F32), F32(0))
        t = np.where(is_hit, t_hit.astype(F32), F32(0))
    return dict(t=t.astype(F32), point=point.astype(F32), normal=nd.astype(F32), code=code.astype(np.uint8), samples=samples, nd=nd, has_n=has_n,
                census=census, D=D)


def info8(res, N):
    """R8"""
    c = res["code"]
    return np.array([len(c)] + [int((c == k).sum()) for k in range(5)] + [int(res["samples"].max()), N], np.int32)


# ---------------------------------------------------------------------------------------------------- R7
def poses(res, T_wc12):
    """R7 -> (pose float32 [n,16], pose_ok uint8 [n])"""
    R = np.asarray(T_wc12, np.float64).reshape(-1)[:9].reshape(3, 3)
    y, D, p = res["nd"], res["D"], res["point"]
    n = len(y)
    with np.errstate(all="ignore"):
        nD = (y[:, 0] * D[:, 0] + y[:, 1] * D[:, 1]) + y[:, 2] * D[:, 2]
        Dl = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        ok = res["has_n"] & (np.abs(nD) / Dl >= MIN_COS)
        xs, xls = [], []
        for col in range(2):
            a = R[:, col]
            an = (a[0] * y[:, 0] + a[1] * y[:, 1]) + a[2] * y[:, 2]
            xc = a[None, :] - an[:, None] * y
            xs.append(xc)
            xls.append(np.sqrt((xc[:, 0] * xc[:, 0] + xc[:, 1] * xc[:, 1]) + xc[:, 2] * xc[:, 2]))
        first = xls[0] >= 1e-6
        x, xl = np.where(first[:, None], xs[0], xs[1]), np.where(first, xls[0], xls[1])
        ok &= xl >= 1e-6
        fallback = ok & ~first
        x = x / np.where(ok, xl, 1.0)[:, None]
        z = np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], 1)
    out = np.zeros((n, 16), F32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11], out[:, 12:15], out[:, 15] = x.astype(F32), y.astype(F32), z.astype(F32), p, F32(1)
    out[~ok] = 0
    return out, ok.astype(np.uint8), fallback


# ---------------------------------------------------------------------------------------------------- the two stages
def grid_pixels(width, height, step):
    gw, gh = width // step, height // step
    u = np.tile(np.arange(gw) * step + step // 2, gh)
    v = np.repeat(np.arange(gh) * step + step // 2, gw)
    return np.stack([u, v], 1).astype(F32)


def pixel_rays(T_wc12, calib8, uv):
    """step 3 of alva_depth_sweep -> (O, D) float64 [n,3]"""
    T = np.asarray(T_wc12, np.float64).reshape(-1)
    R, t = T[:9].reshape(3, 3), T[9:]
    uv = np.asarray(uv, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        uu, vv = Dc.undistort(calib8, uv[:, 0], uv[:, 1])
        x = (uu.astype(np.float64) - calib8[2]) / calib8[0]
        y = (vv.astype(np.float64) - calib8[3]) / calib8[1]
        D = np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * 1.0 for r in range(3)], 1)
    return np.tile(t, (len(uv), 1)), D


def raycast(q, w, origin3, voxel, min_weight, rays6, t_near=0.0, t_far=np.inf):
    """alva_mesh_raycast"""
    rays6 = np.asarray(rays6, np.float64).reshape(-1, 6)
    res = march(q, w, origin3, voxel, min_weight, rays6[:, :3], rays6[:, 3:], t_near, t_far)
    res["info"] = info8(res, np.asarray(q).shape[0])
    return res


def raycast_pixels(q, w, origin3, voxel, min_weight, T_wc12, calib8, width, height, step, uv=None, t_near=0.0, t_far=np.inf):
    """alva_mesh_raycast_pixels: uv None = the grid, row-major [gh gw]; the result also holds pose [n,16], pose_ok [n], rays6 [n,6] (what
    alva_mesh_raycast would be fed) and fallback [n] (R7 took R_wc's second column)"""
    px = grid_pixels(width, height, step) if uv is None else np.asarray(uv, F32).reshape(-1, 2)
    O, D = pixel_rays(T_wc12, calib8, px)
    res = march(q, w, origin3, voxel, min_weight, O, D, t_near, t_far)
    res["info"] = info8(res, np.asarray(q).shape[0])
    res["pose"], res["pose_ok"], res["fallback"] = poses(res, T_wc12)
    res["rays6"] = np.concatenate([O, D], 1)
    return res


def T_wc_of(T_cw12):
    """the inverse of mesh_cases.look_at's T_cw12: R_wc row-major, then t_wc"""
    T = np.asarray(T_cw12, np.float64)
    R, t = T[:9].reshape(3, 3), T[9:]
    return np.concatenate([R.T.reshape(-1), -R.T @ t])


# ---------------------------------------------------------------------------------------------------- the volumes
def wall_dist(z_wall):
    """the half space z >= z_wall, seen from below"""
    return lambda x, y, z: z_wall - z + 0 * x


@functools.lru_cache(maxsize=None)
def volumes():
    V = {}
    V["wall8"] = Mc.sampled(8, wall_dist(0.3))
    V["wall32"] = Mc.sampled(32, wall_dist(0.3))
    for N in (16, 32):
        V[f"sphere{N}"] = Mc.sampled(N, Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R))
    V["box16"] = Mc.sampled(16, Mc.box_dist((-0.52, -0.4, -0.33), (0.47, 0.55, 0.41)))
    V["sphere5"] = Mc.sampled(5, Mc.sphere_dist((0.0, 0.0, 0.0), 0.5))
    # a wall whose slab k = 2 was never seen: the surface lies behind the gap
    q, w, o, vx = Mc.sampled(8, wall_dist(0.3))
    w = w.copy()
    w[2] = 0
    V["gap_before"] = (q, w, o, vx)
    # a wall whose slabs k = 4, 5 -- the ones the surface lies between -- were never seen: free space, the gap, the solid
    w = Mc.sampled(8, wall_dist(0.3))[1].copy()
    w[4:6] = 0
    V["gap_across"] = (q, w, o, vx)
    # q = 0 exactly on the voxel centres of k = 4, the solid above: every coordinate a dyadic rational
    q = np.broadcast_to(((4 - np.arange(8)) * 1000).astype(np.int16)[:, None, None], (8, 8, 8)).copy()
    V["zero_plane"] = (q, np.full((8, 8, 8), 255, np.uint8), np.array([-1.0, -1.0, -1.0]), 0.25)
    V["fresh32"] = (*Mc.empty_volume(32), np.array([-1.0, -1.0, -1.0]), 2.0 / 32)
    V["hashed16"] = (*Mc.hashed_volume(16, 41, -3000, 3000, 4), np.array([-1.0, -1.0, -1.0]), 0.125)
    V["hashed16w"] = (*Mc.hashed_volume(16, 43, -3000, 3000, 255), np.array([-1.0, -1.0, -1.0]), 0.125)
    # a cell whose gradient is zero: + on the corners of even parity, - on the others, of the cell (1, 1, 1) of an N = 4 volume
    q = np.full((4, 4, 4), 1000, np.int16)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        q[1 + dz, 1 + dy, 1 + dx] = 1000 if (dx + dy + dz) % 2 == 0 else -3000
    V["zero_gradient"] = (q, np.full((4, 4, 4), 255, np.uint8), np.array([-0.5, -0.5, -0.5]), 0.25)
    return V


def hashed_rays(n, seed, reach=1.6):
    """n rays from hashed origins in [-reach, reach]^3 towards hashed points of [-0.8, 0.8]^3, of hashed lengths"""
    h = Mc.hashed(7 * n, seed).reshape(n, 7) % 4096
    O = (h[:, :3] / 4095.0 * 2 - 1) * reach
    target = (h[:, 3:6] / 4095.0 * 2 - 1) * 0.8
    return np.concatenate([O, (target - O) * (0.25 + h[:, 6:7] / 1024.0)], 1)


# ---------------------------------------------------------------------------------------------------- the case table
def _wcase(name, vol, rays6, min_weight=1, t_near=0.0, t_far=np.inf, want=None):
    q, w, o, vx = volumes()[vol]
    return dict(name=name, kind="world", q=q, w=w, origin3=o, voxel=vx, min_weight=min_weight, rays6=np.asarray(rays6, np.float64).reshape(-1, 6),
                t_near=t_near, t_far=t_far, want=want)


def _pcase(name, vol, T_wc12, gw, gh, step=4, uv=None, dist=(0.0, 0.0, 0.0, 0.0), min_weight=1, t_near=0.0, t_far=np.inf):
    q, w, o, vx = volumes()[vol]
    width, height = gw * step, gh * step
    return dict(name=name, kind="pixels", q=q, w=w, origin3=o, voxel=vx, min_weight=min_weight, T_wc12=np.asarray(T_wc12, np.float64),
                calib8=Mc.calib_for(width, height, dist), width=width, height=height, step=step,
                uv=None if uv is None else np.asarray(uv, F32).reshape(-1, 2), t_near=t_near, t_far=t_far)


NAN, INF = float("nan"), float("inf")
# named single rays on the N = 8 wall (voxel 0.25, voxel centres -0.875 .. 0.875, the surface at z = 0.3) with the code each must get
WALL_RAYS = [
    ("misses_parallel_outside_slab", (3.0, 3.0, -3.0, 0.0, 0.0, 1.0), 1),
    ("misses_oblique", (3.0, 0.0, -3.0, 0.1, 0.1, 1.0), 1),
    ("parallel_inside_slab", (0.1, 0.2, -2.0, 0.0, 0.0, 1.0), 0),
    ("parallel_on_lo", (-0.875, 0.0, -2.0, 0.0, 0.0, 1.0), 0),
    ("parallel_on_hi", (0.0, 0.875, -2.0, 0.0, 0.0, 2.0), 0),
    ("parallel_just_outside_lo", (-0.8750000000000001, 0.0, -2.0, 0.0, 0.0, 1.0), 1),
    ("origin_inside_free", (0.0, 0.0, -0.5, 0.0, 0.0, 1.0), 0),
    ("origin_inside_free_oblique", (0.3, -0.2, -0.6, -0.2, 0.1, 0.7), 0),
    ("origin_behind_surface", (0.0, 0.0, 0.8, 0.0, 0.0, -1.0), 3),
    ("origin_behind_surface_oblique", (0.1, 0.1, 0.7, 0.3, -0.2, -1.0), 3),
    ("stays_in_free_space", (-2.0, 0.0, -0.5, 1.0, 0.0, 0.0), 2),
    ("stays_in_the_solid", (-2.0, 0.0, 0.6, 1.0, 0.0, 0.0), 2),
    ("leaves_through_a_corner", (0.0, 0.0, 0.0, 1.0, 1.0, -1.0), 2),
    ("long_direction", (0.0, 0.0, -2.0, 0.0, 0.0, 1e6), 0),
    ("short_direction", (0.0, 0.0, -2.0, 0.0, 0.0, 1e-6), 0),
    ("nan_origin", (NAN, 0.0, -2.0, 0.0, 0.0, 1.0), 4),
    ("inf_origin", (0.0, -INF, -2.0, 0.0, 0.0, 1.0), 4),
    ("nan_direction", (0.0, 0.0, -2.0, 0.0, NAN, 1.0), 4),
    ("inf_direction", (0.0, 0.0, -2.0, 0.0, 0.0, INF), 4),
    ("zero_direction", (0.0, 0.0, -2.0, 0.0, 0.0, 0.0), 4),
    ("negative_zero_direction", (0.0, 0.0, -2.0, -0.0, 0.0, -0.0), 4),
    ("denormal_direction", (0.0, 0.0, -2.0, 0.0, 0.0, 5e-324), 2),
]


def _camera(eye, target, up=(0.0, -1.0, 0.0)):
    return T_wc_of(Mc.look_at(eye, target, up))


@functools.lru_cache(maxsize=None)
def cases():
    wall = np.array([r[1] for r in WALL_RAYS])
    want = np.array([r[2] for r in WALL_RAYS])
    along_z = (0.0, 0.0, -2.0, 0.0, 0.0, 1.0)   # meets the wall at t = 2.3
    out = [
        _wcase("wall_named_rays", "wall8", wall, want=want),
        _wcase("gap_then_hit", "gap_before", [along_z, (0.3, -0.4, -2.0, 0.05, 0.1, 1.0)], want=[0, 0]),
        _wcase("no_crossing_across_a_gap", "gap_across", [along_z, (0.3, -0.4, -2.0, 0.05, 0.1, 1.0)], want=[2, 2]),
        _wcase("t_near_beyond_the_surface", "wall8", [along_z], t_near=2.5, want=[2]),
        _wcase("t_far_short_of_the_surface", "wall8", [along_z], t_far=1.5, want=[2]),
        _wcase("t_near_equals_t_far_inside", "wall8", [along_z], t_near=1.5, t_far=1.5, want=[2]),
        _wcase("t_near_equals_t_far_on_the_surface", "wall8", [along_z], t_near=2.3, t_far=2.3, want=[2]),
        _wcase("t_near_equals_t_far_outside", "wall8", [along_z], t_near=0.5, t_far=0.5, want=[1]),
        _wcase("t_near_negative", "wall8", [(0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.5, 0.0, 0.0, 1.0)], t_near=-3.0, want=[0, 0]),
        # F == 0 exactly: as the current sample (a hit on the sample itself), as prev (then the solid is left: code 3)
        _wcase("F_zero_current", "zero_plane", [(0.125, 0.125, -2.0, 0.0, 0.0, 1.0)], want=[0]),
        _wcase("F_zero_prev", "zero_plane", [(0.125, 0.125, 2.0, 0.0, 0.0, -1.0)], want=[3]),
        _wcase("zero_gradient_world", "zero_gradient", [(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)], want=[0]),
        # the long diagonal at N = 32: 2 (N - 1) + 1 = 63 samples of the 2 N + 2 = 66 the bound allows; the volume is fresh (all zero)
        _wcase("fresh_volume_long_diagonal", "fresh32", [(-2.0, -2.0, -2.0, 1.0, 1.0, 1.0), (2.0, -2.0, 2.0, -1.0, 1.0, -1.0), along_z], want=[2, 2, 2]),
        _wcase("sphere32_long_diagonal", "sphere32", [(-2.0, -2.0, -2.0, 1.0, 1.0, 1.0), (2.0, 2.0, 2.0, -0.5, -0.5, -0.5)], want=[0, 0]),
        _wcase("min_weight_255_all_seen", "sphere16", hashed_rays(64, 3), min_weight=255),
        _wcase("min_weight_255_hashed", "hashed16w", hashed_rays(65, 4), min_weight=255),
        _wcase("min_weight_128_hashed", "hashed16w", hashed_rays(65, 5, reach=0.8), min_weight=128),
        _wcase("n4", "zero_gradient", hashed_rays(63, 6, reach=0.9)),
        _wcase("n5", "sphere5", hashed_rays(65, 7)),
        _wcase("box16", "box16", hashed_rays(257, 8)),
    ]
    for n in (1, 63, 64, 65, 257):
        out.append(_wcase(f"hashed_volume_{n}_rays", "hashed16", hashed_rays(n, 10 + n, reach=1.0)))
        out.append(_wcase(f"sphere16_{n}_rays", "sphere16", hashed_rays(n, 20 + n)))
    # pixels: grids (8 x 8 one whole tile, the others partial tiles) and lists
    eye = (1.4, -0.9, -1.9)
    for gw, gh in ((8, 8), (10, 7), (9, 1), (1, 9)):
        out.append(_pcase(f"grid_{gw}x{gh}", "sphere16", _camera(eye, Mc.SPHERE_C), gw, gh))
    out.append(_pcase("grid_24x18_step1", "sphere32", _camera((-0.3, 0.2, -2.4), Mc.SPHERE_C), 24, 18, step=1))
    out.append(_pcase("grid_step8_inside_the_volume", "box16", _camera((-0.9, -0.9, -0.9), (0.0, 0.1, 0.0)), 17, 9, step=8))
    out.append(_pcase("distortion", "sphere16", _camera(eye, Mc.SPHERE_C), 20, 15, dist=(-0.28, 0.07, 0.0011, -0.0007)))
    out.append(_pcase("grid_hashed_volume", "hashed16", _camera((0.2, 0.1, -0.3), (0.0, 0.0, 0.9)), 19, 13))
    # grazing: the wall seen from close above it, the optical axis under 5 degrees from the surface; the rows below meet it more steeply
    out.append(_pcase("grazing", "wall32", _camera((-0.8, 0.0, 0.25), (0.2, 0.0, 0.31), up=(0.0, 0.0, -1.0)), 16, 12))
    # the camera's x axis along the wall's normal (0, 0, -1): R7 falls back to R_wc's second column
    T_side = [0, 0, -1, 0, 1, 0, 1, 0, 0, 0.8, 0.0, -0.3]
    side = _pcase("pose_fallback_axis", "wall32", T_side, 16, 12)
    c = side["calib8"]
    side["uv"] = np.array([[c[2] + c[0] * 0.5, c[3]], [c[2] + c[0] * 0.4, c[3] + 7.0], [c[2] - 3.0, c[3]]], F32)
    out.append(side)
    zg = _pcase("zero_gradient_pose", "zero_gradient", _camera((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), 8, 8)
    zg["uv"] = np.array([[zg["calib8"][2], zg["calib8"][3]]], F32)
    out.append(zg)
    # taps: off the image, non-finite, 65 of them
    taps = _pcase("taps", "sphere16", _camera(eye, Mc.SPHERE_C), 16, 12)
    h = Mc.hashed(130, 9).reshape(65, 2) % 1024
    uv = (h / 1023.0 * np.array([80.0, 64.0]) - 8.0).astype(F32)
    uv[3] = (NAN, 5.0)
    uv[4] = (5.0, INF)
    uv[5] = (-1e30, 1e30)
    taps["uv"] = uv
    out.append(taps)
    out.append(_pcase("pixels_t_far", "sphere16", _camera(eye, Mc.SPHERE_C), 10, 7, t_near=1.0, t_far=2.2))
    return out


def run(case):
    """the restatement on a case"""
    vol = (case["q"], case["w"], case["origin3"], case["voxel"], case["min_weight"])
    if case["kind"] == "world":
        return raycast(*vol, case["rays6"], case["t_near"], case["t_far"])
    return raycast_pixels(*vol, case["T_wc12"], case["calib8"], case["width"], case["height"], case["step"], case["uv"], case["t_near"], case["t_far"])


@functools.lru_cache(maxsize=None)
def expected():
    """the restatement on every case, computed once: name -> result (read only)"""
    return {c["name"]: run(c) for c in cases()}


# ---------------------------------------------------------------------------------------------------- the analytic scenes
SPHERE_VIEWS = [((2.5, 0.0, 0.0), (0.0, -1.0, 0.0)), ((-2.5, 0.0, 0.0), (0.0, -1.0, 0.0)), ((0.0, 2.5, 0.0), (0.0, 0.0, 1.0)),
                ((0.0, -2.5, 0.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 2.5), (0.0, -1.0, 0.0)), ((0.0, 0.0, -2.5), (0.0, -1.0, 0.0)),
                ((1.6, -1.1, -1.5), (0.0, -1.0, 0.0)), ((-1.2, 1.5, 1.4), (0.0, -1.0, 0.0))]
SPHERE_GW, SPHERE_GH, SPHERE_STEP = 24, 18, 4


def sphere_view(k):
    """view k of the analytic sphere at N = 32 -> (the restatement's result, per ray the distance of the line from the sphere's centre)"""
    q, w, o, vx = volumes()["sphere32"]
    eye, up = SPHERE_VIEWS[k]
    width, height = SPHERE_GW * SPHERE_STEP, SPHERE_GH * SPHERE_STEP
    res = raycast_pixels(q, w, o, vx, 1, _camera(eye, Mc.SPHERE_C, up), Mc.calib_for(width, height), width, height, SPHERE_STEP)
    O, D = res["rays6"][:, :3], res["rays6"][:, 3:]
    d = D / np.linalg.norm(D, axis=1)[:, None]
    oc = np.asarray(Mc.SPHERE_C) - O
    along = (oc * d).sum(1)
    miss = np.sqrt(np.maximum((oc * oc).sum(1) - along * along, 0.0))
    return res, np.where(along > 0, miss, np.inf)


E2E_NINTH = (0.45, -0.35, -2.35)   # between the arc's poses, off its plane


def e2e_depth():
    """mesh_cases.e2e_run's volume seen from a ninth pose -> (the restatement's result, the analytic depth [gh,gw], T_cw12)"""
    r = Mc.e2e_run()
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib = Mc.calib_for(width, height)
    T_cw = Mc.look_at(E2E_NINTH, (0.0, 0.0, 0.3))
    res = raycast_pixels(r["q"], r["w"], r["origin3"], r["voxel"], 2, T_wc_of(T_cw), calib, width, height, Mc.E2E_STEP)
    return res, Mc.render(Mc.e2e_scene(), T_cw, calib, width, height, Mc.E2E_STEP), T_cw
