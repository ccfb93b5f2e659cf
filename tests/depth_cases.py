"""The depth sweep's definition (include/alvaar_hip.h, alva_depth_sweep) restated in numpy, step for step, the scenes the tests run it
on and the case table.  The reference has no depth from motion, so this file is what alva_depth_sweep is pinned to
(tests/test_depth_cases.py checks the restatement itself, tests/test_gpu_depth_sweep.py the kernel against it, bit for bit).

The geometry is float64 / float32 exactly where the definition says so, in its operation order (elementwise numpy does not contract
a * b + c into an FMA; nothing below goes through a BLAS product); the costs are integers.  There is no sum whose order could differ,
so the GPU is compared with `==`, not with a tolerance."""
from __future__ import annotations

import functools

import numpy as np

from alvaar_amd import synth

F32 = np.float32


# ---------------------------------------------------------------------------------------------------- the camera model
def undistort(calib8, u, v):
    """alva_undistort_dev on arrays: float32 in, float32 out"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (np.float64(c) for c in calib8)
    ifx, ify = 1.0 / fx, 1.0 / fy
    u, v = np.asarray(u, F32).astype(np.float64), np.asarray(v, F32).astype(np.float64)
    x = (u - cx) * ifx
    y = (v - cy) * ify
    x0, y0 = x, y
    done = np.zeros(x.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((0 * r2 + k2) * r2 + k1) * r2)
        brk = ~done & (icdist < 0)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + 0 * r2 + 0 * r2 * r2
        xn = np.where(brk, (u - cx) * ifx, (x0 - dx) * icdist)
        yn = np.where(brk, (v - cy) * ify, (y0 - dy) * icdist)
        x, y = np.where(done, x, xn), np.where(done, y, yn)
        done = done | brk
    xx, yy, ww = fx * x + 0 * y + cx, 0 * x + fy * y + cy, 1.0 / (0 * x + 0 * y + 1)
    return (xx * ww).astype(F32), (yy * ww).astype(F32)


def project_dist(calib8, X, Y, Z):
    """alva_project_dist_dev on arrays: float64 in, float32 out"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (np.float64(c) for c in calib8)
    iz = 1.0 / Z
    x, y = (X * iz).astype(F32).astype(np.float64), (Y * iz).astype(F32).astype(np.float64)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
    cdist = 1 + k1 * r2 + k2 * r4 + 0 * r6
    icdist2 = 1.0 / (1 + 0 * r2 + 0 * r4 + 0 * r6)
    xd0 = x * cdist * icdist2 + p1 * a1 + p2 * a2 + 0 * r2 + 0 * r4
    yd0 = y * cdist * icdist2 + p1 * a3 + p2 * a1 + 0 * r2 + 0 * r4
    return (xd0 * fx + cx).astype(F32), (yd0 * fy + cy).astype(F32)


# ---------------------------------------------------------------------------------------------------- the restatement
def sweep(cur, ref, calib8, T_rc12, rho_min, rho_max, step=4, num_hyp=64, patch_radius=2, min_texture=4, min_conf=96, width=None):
    """alva_depth_sweep.  cur / ref: [h, w'] uint8 (w' >= width: what lies past `width` is padding).  Returns a dict: depth [gh,gw]
    float32, conf, code [gh,gw] uint8, info [8] int32, best [gh,gw,4] int32 = {kb, best, second, T}, and off [gh,gw] float64 (the
    refinement's offset, for the tests)."""
    cur, ref = np.asarray(cur), np.asarray(ref)
    assert cur.dtype == np.uint8 and ref.dtype == np.uint8 and cur.shape == ref.shape
    h, w = cur.shape[0], cur.shape[1] if width is None else width
    D, r = int(num_hyp), int(patch_radius)
    N = (2 * r + 1) ** 2
    Tm = np.asarray(T_rc12, np.float64).reshape(-1)
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    fx, fy, cx, cy = (np.float64(c) for c in calib8[:4])
    rho_min, rho_max = np.float64(rho_min), np.float64(rho_max)
    gw, gh = w // step, h // step
    G = gw * gh
    u = np.tile(np.arange(gw) * step + step // 2, gh)
    v = np.repeat(np.arange(gh) * step + step // 2, gw)
    depth, conf, code = np.zeros(G, F32), np.zeros(G, np.uint8), np.zeros(G, np.uint8)
    best4 = np.full((G, 4), -1, np.int32)
    off_all = np.zeros(G)
    # 1 patch
    inside = (u - r >= 0) & (u + r <= w - 1) & (v - r >= 0) & (v + r <= h - 1)
    code[~inside] = 1
    best4[~inside, 3] = 0
    gi = np.nonzero(inside)[0]
    dy, dx = (a.ravel() for a in np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij"))   # dy outer, dx inner
    px, py = u[gi, None] + dx[None, :], v[gi, None] + dy[None, :]
    c = cur[py, px].astype(np.int64)
    cdev = N * c - c.sum(1, keepdims=True)
    # 2 texture
    T = np.abs(cdev).sum(1)
    best4[gi, 3] = T
    flat = T < min_texture * N * N
    code[gi[flat]] = 2
    act = ~flat
    gi, px, py, cdev = gi[act], px[act], py[act], cdev[act]
    A = len(gi)
    if A:
        # 3 rays
        uu, vv = undistort(calib8, px.astype(F32), py.astype(F32))
        x, y = (uu.astype(np.float64) - cx) / fx, (vv.astype(np.float64) - cy) / fy
        q = [(R[i, 0] * x + R[i, 1] * y) + R[i, 2] * 1.0 for i in range(3)]
        # 4 hypotheses
        cost = np.full((D, A), -1, np.int64)
        wmax, hmax = F32(w - 1), F32(h - 1)
        refi = ref.astype(np.int64)
        for k in range(D):
            rho = rho_min + ((rho_max - rho_min) * np.float64(k)) / np.float64(D - 1)
            Px, Py, Pz = q[0] + rho * t[0], q[1] + rho * t[1], q[2] + rho * t[2]
            with np.errstate(all="ignore"):
                up, vp = project_dist(calib8, Px, Py, Pz)
                fu, fv = np.floor(up), np.floor(vp)
                ok = (Pz > 1e-9) & (F32(0) <= fu) & (fu + F32(1) <= wmax) & (F32(0) <= fv) & (fv + F32(1) <= hmax)
                valid = ok.all(1)
                a = np.rint((up - fu) * F32(32)).astype(np.float64)
                b = np.rint((vp - fv) * F32(32)).astype(np.float64)
            okv = ok & valid[:, None]
            iu, iv = np.where(okv, fu, 0).astype(np.int64), np.where(okv, fv, 0).astype(np.int64)
            a, b = np.where(okv, a, 0).astype(np.int64), np.where(okv, b, 0).astype(np.int64)
            s = (refi[iv, iu] * (32 - a) * (32 - b) + refi[iv, iu + 1] * a * (32 - b) + refi[iv + 1, iu] * (32 - a) * b
                 + refi[iv + 1, iu + 1] * a * b + 512) >> 10
            ck = np.abs(cdev - (N * s - s.sum(1, keepdims=True))).sum(1)
            cost[k] = np.where(valid, ck, -1)
        # 5 winner
        BIG = np.int64(1) << 40
        cv = np.where(cost >= 0, cost, BIG)
        kb = cv.argmin(0)   # the first of equal minima: the lowest k
        best = cv[kb, np.arange(A)]
        none = best >= BIG
        ks = np.arange(D)[:, None]
        far = np.where(np.abs(ks - kb[None, :]) >= 2, cv, BIG).min(0)
        has2 = far < BIG
        second = np.where(has2, far, -1)
        cf = np.where(has2, 255 - (255 * best) // np.maximum(far, 1), 0)
        # 6 refinement
        inner = (kb > 0) & (kb < D - 1)
        cm = cost[np.clip(kb - 1, 0, D - 1), np.arange(A)]
        cp = cost[np.clip(kb + 1, 0, D - 1), np.arange(A)]
        den = cm - 2 * best + cp
        use = inner & (cm >= 0) & (cp >= 0) & (den > 0) & ~none
        off = np.where(use, (cm - cp).astype(np.float64) / np.where(use, 2 * den, 1).astype(np.float64), 0.0)
        rho = rho_min + ((rho_max - rho_min) * (kb.astype(np.float64) + off)) / np.float64(D - 1)
        dep = (1.0 / rho).astype(F32)
        # 7 codes
        cd = np.where(none, 3, np.where((kb == 0) | (kb == D - 1), 5, np.where(cf < min_conf, 4, 0)))
        code[gi] = cd
        depth[gi] = np.where(cd == 0, dep, F32(0))
        conf[gi] = np.where(none, 0, cf)
        best4[gi, 0] = np.where(none, -1, kb)
        best4[gi, 1] = np.where(none, -1, best)
        best4[gi, 2] = np.where(none, -1, second)
        off_all[gi] = np.where(none, 0.0, off)
    info = np.array([int((code == k).sum()) for k in range(6)] + [gw, gh], np.int32)
    return dict(depth=depth.reshape(gh, gw), conf=conf.reshape(gh, gw), code=code.reshape(gh, gw), info=info, best=best4.reshape(gh, gw, 4),
                off=off_all.reshape(gh, gw))


# ---------------------------------------------------------------------------------------------------- scenes
W, H, F = 256, 192, 232.0
FAR_Z, NEAR_Z, NEAR_X = 4.0, 2.6, 0.3
RHO_RANGE = (1.0 / 8.0, 1.0 / 1.5)
K_DIST4 = (-0.1, 0.02, 1e-3, 1e-3)
DENSE_PAIRS = ((40, 10), (40, 25), (90, 60))   # (current, reference) frames of synth.plane_camera_pose


def calib_of(w=W, h=H, f=F, dist=(0.0, 0.0, 0.0, 0.0)):
    return (f, f, w * 0.5, h * 0.5) + tuple(dist)


@functools.lru_cache(maxsize=None)
def dense_canvas(w=W, h=H, seed=3, margin=400):
    """gray 96 with area / 12 squares of side 3 .. 12 and a random gray: texture nearly everywhere"""
    rng = np.random.RandomState(seed)
    ch, cw = h + margin, w + margin
    canvas = np.full((ch, cw), 96, np.uint8)
    n = (ch * cw) // 12
    xs, ys, sides, grays = rng.randint(0, cw, n), rng.randint(0, ch, n), rng.randint(3, 13, n), rng.randint(0, 256, n)
    for x, y, s, g in zip(xs, ys, sides, grays):
        canvas[y:y + s, x:x + s] = g
    canvas.setflags(write=False)
    return canvas


def T_rc(k_cur, k_ref):
    """R_rc row-major then t_rc, X_ref = R_rc X_cur + t_rc, from the two frames' Twc"""
    Rc, tc = synth.plane_camera_pose(k_cur)
    Rr, tr = synth.plane_camera_pose(k_ref)
    return np.concatenate([(Rr.T @ Rc).ravel(), Rr.T @ (tc - tr)])


def pixel_rays(w, h, calib8):
    """camera-frame rays (x, y, 1) of every raw pixel: K^-1 of the undistorted pixel"""
    ys, xs = np.mgrid[0:h, 0:w]
    uu, vv = undistort(calib8, xs.astype(F32), ys.astype(F32))
    return np.stack([(uu.astype(np.float64) - calib8[2]) / calib8[0], (vv.astype(np.float64) - calib8[3]) / calib8[1], np.ones((h, w))], -1)


def render_rays(canvas, rays, f, R_wc, t_wc, plane_z):
    """synth.render_plane's inverse mapping for given camera-frame rays [h,w,3] (for the pinhole rays it is synth.render_plane, which
    tests/test_depth_cases.py asserts).  Returns (image u8, lam = the camera-space depth of the plane along each ray, world X)."""
    ch, cw = canvas.shape
    d = rays @ R_wc.T
    lam = (plane_z - t_wc[2]) / d[..., 2]
    X = t_wc[0] + lam * d[..., 0]
    Y = t_wc[1] + lam * d[..., 1]
    s = f / plane_z
    u = cw * 0.5 + s * X
    v = ch * 0.5 + s * Y
    u0 = np.clip(np.floor(u).astype(np.int64), 0, cw - 2)
    v0 = np.clip(np.floor(v).astype(np.int64), 0, ch - 2)
    a = np.clip(u - u0, 0.0, 1.0)
    b = np.clip(v - v0, 0.0, 1.0)
    c = canvas.astype(np.float64)
    out = (c[v0, u0] * (1 - a) * (1 - b) + c[v0, u0 + 1] * a * (1 - b) + c[v0 + 1, u0] * (1 - a) * b + c[v0 + 1, u0 + 1] * a * b)
    out[(lam <= 0) | (u < 0) | (v < 0) | (u > cw - 1) | (v > ch - 1)] = 0
    return np.clip(np.rint(out), 0, 255).astype(np.uint8), lam, X


@functools.lru_cache(maxsize=None)
def two_depth_frame(k, w=W, h=H, f=F, dist=(0.0, 0.0, 0.0, 0.0)):
    """frame k of the dense two-depth scene: the plane z = 4, and in front of it the plane z = 2.6 where world X > 0.3.  Returns
    (image u8 [h,w], the analytic depth [h,w], near mask [h,w])"""
    canvas = dense_canvas(w, h)
    R, t = synth.plane_camera_pose(k)
    rays = pixel_rays(w, h, calib_of(w, h, f, dist))
    if not any(dist):
        far, near = (synth.render_plane(canvas, w, h, f, R, t, z) for z in (FAR_Z, NEAR_Z))
        _, lam_f, _ = render_rays(canvas, rays, f, R, t, FAR_Z)
        _, lam_n, X_n = render_rays(canvas, rays, f, R, t, NEAR_Z)
    else:
        far, lam_f, _ = render_rays(canvas, rays, f, R, t, FAR_Z)
        near, lam_n, X_n = render_rays(canvas, rays, f, R, t, NEAR_Z)
    mask = (lam_n > 0) & (X_n > NEAR_X)
    img = np.where(mask, near, far)
    img.setflags(write=False)
    return img, np.where(mask, lam_n, lam_f), mask


@functools.lru_cache(maxsize=None)
def sparse_frame(k, w=W, h=H, f=F):
    """frame k of the tracking tests' plane: synth.texture_canvas, mostly black"""
    R, t = synth.plane_camera_pose(k)
    img = synth.render_plane(synth.texture_canvas(w, h, 5), w, h, f, R, t)
    img.setflags(write=False)
    return img


def grid_truth(truth, step):
    """the analytic depth at the grid's centres"""
    h, w = truth.shape
    return truth[step // 2:(h // step) * step:step, step // 2:(w // step) * step:step]


# ---------------------------------------------------------------------------------------------------- the case table
# Measured with this restatement (dense scene, step 4, D 48, min_texture 4, min_conf 96): name -> (share of the grid with code 0, share
# of those within 3 % of the analytic depth, median relative error).  tests/test_depth_cases.py bounds the last two by these values
# loosened by a quarter of their distance to the trivial bound: the texture is random and the pairs differ.  The trivial bounds are a
# share of 0 and a median error of 0.03 (with more than half the answers within 3 %, which the share's floor already demands, the
# median cannot be larger).
DENSE_MEASURED = {
    "dense_40_10_r2": (0.6260, 0.9756, 0.00371),
    "dense_40_10_r3": (0.7018, 0.9903, 0.00326),
    "dense_40_25_r2": (0.7012, 0.9800, 0.00427),
    "dense_40_25_r3": (0.7676, 0.9835, 0.00354),
    "dense_90_60_r2": (0.7051, 0.9834, 0.00424),
    "dense_90_60_r3": (0.7526, 0.9857, 0.00347),
    "distorted_40_10": (0.6413, 0.9726, 0.00377),
}


def quality_bounds(name):
    """(the floor of the within-3 % share, the ceiling of the median relative error) of a dense case"""
    _, within3, median = DENSE_MEASURED[name]
    return within3 - 0.25 * (within3 - 0.0), median + 0.25 * (0.03 - median)


def _case(cur, ref, calib8, T, rho=RHO_RANGE, width=None, pad=0, **kw):
    return dict(cur=cur, ref=ref, calib8=tuple(calib8), T=np.asarray(T, np.float64), rho=rho, width=width, pad=pad, kw=kw)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(cur, ref [h,w] u8, calib8, T [12], rho (min, max), width (or None), pad (extra bytes per row on the device), kw for
    sweep / Context.depth_sweep).  Sizes: 256 x 192 for the scenes, 64 x 64 for the edges."""
    out = {}
    cal = calib_of()
    for kc, kr in DENSE_PAIRS:
        for r in (2, 3):
            out["dense_%d_%d_r%d" % (kc, kr, r)] = _case(two_depth_frame(kc)[0], two_depth_frame(kr)[0], cal, T_rc(kc, kr), step=4, num_hyp=48,
                                                           patch_radius=r, min_texture=4, min_conf=96)
    out["sparse_40_10"] = _case(sparse_frame(40), sparse_frame(10), cal, T_rc(40, 10), step=4, num_hyp=48, patch_radius=2, min_texture=4,
                                min_conf=96)
    out["distorted_40_10"] = _case(two_depth_frame(40, dist=K_DIST4)[0], two_depth_frame(10, dist=K_DIST4)[0], calib_of(dist=K_DIST4),
                                   T_rc(40, 10), step=4, num_hyp=48, patch_radius=2, min_texture=4, min_conf=96)
    # ---- 64 x 64: the codes and the size edges
    w = h = 64
    f = 58.0
    cal = calib_of(w, h, f)
    cur, ref = two_depth_frame(40, w, h, f)[0], two_depth_frame(10, w, h, f)[0]
    T = T_rc(40, 10)
    base = dict(step=4, num_hyp=16, patch_radius=2, min_texture=4, min_conf=96)
    out["code1_border_rows"] = _case(cur, ref, cal, T, **dict(base, step=2, patch_radius=4))
    out["code2_flat_image"] = _case(np.full((h, w), 77, np.uint8), ref, cal, T, **base)
    away = np.concatenate([np.diag([-1.0, 1.0, -1.0]).ravel(), [0.0, 0.0, 0.0]])   # the reference camera looks the other way
    out["code3_looking_away"] = _case(cur, ref, cal, away, **base)
    out["code5_range_excludes"] = _case(cur, ref, cal, T, rho=(1.0 / 1.4, 1.0 / 1.0), **base)
    out["code4_min_conf_255"] = _case(cur, ref, cal, T, **dict(base, min_conf=255))
    out["tie_lowest_k"] = _case(np.full((h, w), 77, np.uint8), np.full((h, w), 200, np.uint8), cal, T, **dict(base, min_texture=0))
    out["step1"] = _case(cur, ref, cal, T, **dict(base, step=1))
    out["step16"] = _case(cur, ref, cal, T, **dict(base, step=16))
    out["d8"] = _case(cur, ref, cal, T, **dict(base, num_hyp=8))
    out["d256"] = _case(cur, ref, cal, T, **dict(base, num_hyp=256))
    out["d65"] = _case(cur, ref, cal, T, **dict(base, num_hyp=65))     # a second pass of one lane
    out["r1"] = _case(cur, ref, cal, T, **dict(base, patch_radius=1))
    out["r4"] = _case(cur, ref, cal, T, **dict(base, patch_radius=4))  # N = 81: more patch pixels than lanes
    out["width60_step8"] = _case(cur, ref, cal, T, width=60, **dict(base, step=8))   # 60 / 8 truncates to 7; columns 60 .. 63 are padding
    out["pitch_80"] = _case(cur, ref, cal, T, pad=16, **base)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c = cases()[name]
    return sweep(c["cur"], c["ref"], c["calib8"], c["T"], c["rho"][0], c["rho"][1], width=c["width"], **c["kw"])
