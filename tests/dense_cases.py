"""The dense depth stages' definitions (include/alvaar_hip.h: alva_depth_fuse F1-F5, alva_depth_fill P1-P4) restated in numpy, operation
for operation, the analytic scenes the tests run them on and the two case tables.  The reference has no dense depth, so this file is
what the two stages are pinned to (tests/test_dense_cases.py checks the restatement against geometry, analytic depth and brute-force
fills; tests/test_gpu_depth_dense.py the kernels against it, bit for bit).

As in tests/depth_cases.py the geometry is float64 / float32 exactly where the definition says so, in its operation order (elementwise
numpy does not contract a * b + c), and every sum of more than two terms is an integer sum, so the GPU is compared with `==`."""
from __future__ import annotations

import functools

import numpy as np

import depth_cases as Dc

F32 = np.float32
Q_MAX = (1 << 20) - 1
FLT_MAX = np.finfo(np.float32).max
DECAY, W_MAX, REL_TOL = 230, 128, 0.05   # the system call's constants (include/alvaar_system.h)


def hashed(n, seed):
    """n hashed 32-bit values (a fixed integer mix of the index: the same on every machine)"""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    for _ in range(2):
        x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
        x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return (x ^ (x >> np.uint64(16))).astype(np.int64)


def hashed_unit(n, seed):
    """n hashed values in [0, 1)"""
    return hashed(n, seed).astype(np.float64) / 4294967296.0


# ---------------------------------------------------------------------------------------------------- alva_depth_fuse
def warp(prev_rho, prev_w, T_cp12, calib8, width, height, step):
    """F1: the key of every cell (uint64 [gh gw], 0 = no source) and, for the tests, per source its target cell (or -1) and rho'"""
    gw, gh = width // step, height // step
    G = gw * gh
    rho_f = np.asarray(prev_rho, F32).reshape(-1)[:G]
    w = np.asarray(prev_w, np.uint8).reshape(-1)[:G]
    Tm = np.asarray(T_cp12, np.float64).reshape(-1)
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    fx, fy, cx, cy = (np.float64(c) for c in calib8[:4])
    keys = np.zeros(G, np.uint64)
    target, rho_new = np.full(G, -1, np.int64), np.zeros(G, F32)
    src = np.nonzero((w > 0) & (rho_f > F32(0)))[0]
    if len(src):
        u = (src % gw) * step + step // 2
        v = (src // gw) * step + step // 2
        uu, vv = Dc.undistort(calib8, u.astype(F32), v.astype(F32))
        x, y = (uu.astype(np.float64) - cx) / fx, (vv.astype(np.float64) - cy) / fy
        rho = rho_f[src].astype(np.float64)
        P = [((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * 1.0) + rho * t[i] for i in range(3)]
        with np.errstate(all="ignore"):
            ok = P[2] > 1e-9
            up, vp = Dc.project_dist(calib8, P[0], P[1], P[2])
            fu, fv = np.floor(up + F32(0.5)), np.floor(vp + F32(0.5))
            assert fu.dtype == F32
            ok &= (F32(0) <= fu) & (fu < F32(gw * step)) & (F32(0) <= fv) & (fv < F32(gh * step))
            rn = (rho / P[2]).astype(F32)
            ok &= (rn > F32(0)) & (rn <= FLT_MAX)
        i, rn = src[ok], rn[ok]
        j = (fv[ok].astype(np.int64) // step) * gw + fu[ok].astype(np.int64) // step
        key = (rn.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i.astype(np.uint64))
        np.maximum.at(keys, j, key)
        target[i], rho_new[i] = j, rn
    return keys, target, rho_new


def fuse(prev, T_cp12, calib8, width, height, step, meas, decay=DECAY, w_max=W_MAX, rel_tol=REL_TOL):
    """alva_depth_fuse.  prev = (rho, w) or None, meas = (depth, conf, code) or None, each [gh,gw].  Returns a dict: rho float32, w uint8,
    src uint8 [gh,gw], info [8] int32, and for the tests source [gh,gw] (the winning source index, -1 without one)."""
    gw, gh = width // step, height // step
    G = gw * gh
    # F1, F2
    rho_c, w_c, source = np.zeros(G, F32), np.zeros(G, np.int64), np.full(G, -1, np.int64)
    if prev is not None:
        keys, _, _ = warp(prev[0], prev[1], T_cp12, calib8, width, height, step)
        has = keys != 0
        idx = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
        idx = np.where(has, idx, 0)
        w_c = np.where(has, (np.asarray(prev[1], np.uint8).reshape(-1)[idx].astype(np.int64) * int(decay)) >> 8, 0)
        rho_c = np.where(has, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
        source = np.where(has, idx, -1)
    # F3
    rho_m, w_m = np.zeros(G, F32), np.zeros(G, np.int64)
    if meas is not None:
        depth = np.asarray(meas[0], F32).reshape(-1)[:G]
        conf = np.asarray(meas[1], np.uint8).reshape(-1)[:G].astype(np.int64)
        code = np.asarray(meas[2], np.uint8).reshape(-1)[:G]
        m = (code == 0) & (depth > F32(0))
        with np.errstate(all="ignore"):
            rho_m = np.where(m, (1.0 / depth.astype(np.float64)).astype(F32), F32(0)).astype(F32)
        w_m = np.where(m, np.maximum(1, conf >> 3), 0)
    # F4
    a, b = rho_c.astype(np.float64), rho_m.astype(np.float64)
    both = (w_c > 0) & (w_m > 0)
    with np.errstate(all="ignore"):
        agree = np.abs(a - b) <= np.float64(rel_tol) * np.maximum(a, b)
        mean = ((w_c.astype(np.float64) * a + w_m.astype(np.float64) * b) / np.maximum(w_c + w_m, 1).astype(np.float64)).astype(F32)
    src = np.select([(w_c == 0) & (w_m == 0), w_c == 0, w_m == 0, both & agree, both & (w_m >= w_c)], [0, 1, 2, 3, 4], 5)
    rho = np.select([src == 0, src == 1, src == 2, src == 3, src == 4], [F32(0), rho_m, rho_c, mean, rho_m], rho_c).astype(F32)
    w = np.select([src == 0, src == 1, src == 2, src == 3, src == 4], [0, w_m, w_c, np.minimum(int(w_max), w_c + w_m), w_m], w_c - w_m)
    # F5
    info = np.array([int((src == k).sum()) for k in range(6)] + [gw, gh], np.int32)
    return dict(rho=rho.reshape(gh, gw), w=w.astype(np.uint8).reshape(gh, gw), src=src.astype(np.uint8).reshape(gh, gw), info=info,
                source=source.reshape(gh, gw))


# ---------------------------------------------------------------------------------------------------- alva_depth_fill
def E_weight(d):
    return np.maximum(1, 64 >> np.minimum(d >> 3, 6))


def quantise(rho, w, rho_ref):
    """P1's q and W"""
    with np.errstate(all="ignore"):
        r = np.rint((np.asarray(rho, F32).astype(np.float64) / np.float64(rho_ref)) * 65536.0)
        q = np.where(r >= Q_MAX, Q_MAX, np.where(r >= 0, r, 0)).astype(np.int64)
    W = np.asarray(w, np.uint8).astype(np.int64)
    return np.where(W > 0, q, 0), W


def fill(rho, w, gray, step, rho_ref, max_level, width=None, edge_aware=True):
    """alva_depth_fill.  rho float32 / w uint8 [gh,gw], gray [h,w'] uint8 (w' >= width).  edge_aware=False is the plain push-pull with E = 1
    (not a mode of the stage: the tests' comparison).  Returns a dict: depth float32, level uint8 [gh,gw], info [4] int32, q [gh,gw]."""
    gray = np.asarray(gray)
    h, wd = gray.shape[0], gray.shape[1] if width is None else width
    gw, gh = wd // step, h // step
    rho = np.asarray(rho, F32).reshape(-1)[:gw * gh].reshape(gh, gw)
    w = np.asarray(w, np.uint8).reshape(-1)[:gw * gh].reshape(gh, gw)
    L = int(max_level)
    # P1
    q0, W0 = quantise(rho, w, rho_ref)
    G0 = gray[step // 2:gh * step:step, step // 2:gw * step:step][:gh, :gw].astype(np.int64)
    qs, Ws, Gs = [q0], [W0], [G0]
    # P2
    for _ in range(L):
        q, W, G = qs[-1], Ws[-1], Gs[-1]
        hl, wl = q.shape
        hc, wc = (hl + 1) // 2, (wl + 1) // 2

        def blocks(a):
            p = np.zeros((2 * hc, 2 * wc), np.int64)
            p[:hl, :wl] = a
            return p.reshape(hc, 2, wc, 2).sum((1, 3))
        Wsum, n = blocks(W), blocks(np.ones((hl, wl), np.int64))
        qs.append(np.where(Wsum > 0, (blocks(W * q) + Wsum // 2) // np.maximum(Wsum, 1), 0))
        Ws.append(np.minimum(255, Wsum))
        Gs.append((blocks(G) + n // 2) // n)
    # P3
    has, val, ev = Ws[L] > 0, qs[L].copy(), np.full(qs[L].shape, L, np.int64)
    for l in range(L - 1, -1, -1):
        hl, wl = qs[l].shape
        hp, wp = qs[l + 1].shape
        Y, X = np.mgrid[0:hl, 0:wl]
        S, acc, evmin = np.zeros((hl, wl), np.int64), np.zeros((hl, wl), np.int64), np.full((hl, wl), 255, np.int64)
        for py, wy in ((Y >> 1, 3), ((Y >> 1) + np.where(Y & 1, 1, -1), 1)):
            for px, wx in ((X >> 1, 3), ((X >> 1) + np.where(X & 1, 1, -1), 1)):
                inside = (px >= 0) & (py >= 0) & (px < wp) & (py < hp)
                pxc, pyc = np.clip(px, 0, wp - 1), np.clip(py, 0, hp - 1)
                counts = inside & has[pyc, pxc]
                e = E_weight(np.abs(Gs[l] - Gs[l + 1][pyc, pxc])) if edge_aware else 1
                wt = np.where(counts, wx * wy * e, 0)
                S += wt
                acc += wt * val[pyc, pxc]
                evmin = np.where(counts, np.minimum(evmin, ev[pyc, pxc]), evmin)
        own = Ws[l] > 0
        filled = ~own & (S > 0)
        val = np.where(own, qs[l], np.where(filled, (acc + S // 2) // np.maximum(S, 1), 0))
        ev = np.where(own, l, evmin)
        has = own | filled
    # P4
    seed = W0 > 0
    got = ~seed & has & (val > 0)
    with np.errstate(all="ignore"):
        d_seed = (1.0 / rho.astype(np.float64)).astype(F32)
        d_fill = (65536.0 / (np.maximum(val, 1).astype(np.float64) * np.float64(rho_ref))).astype(F32)
    depth = np.where(seed, d_seed, np.where(got, d_fill, F32(0))).astype(F32)
    level = np.where(seed, 0, np.where(got, ev, 255)).astype(np.uint8)
    info = np.array([int(seed.sum()), int(got.sum()), int((~seed & ~got).sum()), int(level[got].max()) if got.any() else 0], np.int32)
    return dict(depth=depth, level=level, info=info, q=np.where(seed | got, val, 0))


# ---------------------------------------------------------------------------------------------------- scenes
def two_surface_grid(seed=1, gw=64, gh=48, share=0.30):
    """The fill tests' analytic grid: a slanted step edge between a surface of depth about 4.0 (left) and one of about 2.6 (right), both
    with mild slopes; the guide is 60 on the left and 180 on the right, each +-12 (hashed).  Seeds are a hashed `share` of the cells,
    without a 16 x 12 hole across the edge and without the three leftmost columns.  Returns dict(truth, guide u8, near mask, rho, w,
    hole mask, edge_x per row)."""
    Y, X = np.mgrid[0:gh, 0:gw].astype(np.float64)
    edge_x = gw * 0.5 + (np.arange(gh) - gh * 0.5) * 0.25          # the edge moves a quarter cell per row
    near = X >= edge_x[:, None]
    truth = np.where(near, 2.6 + 0.004 * (X - gw * 0.5) + 0.003 * Y, 4.0 - 0.006 * X + 0.004 * Y)
    noise = (hashed(gw * gh, 100 + seed) % 25 - 12).reshape(gh, gw)
    guide = (np.where(near, 180, 60) + noise).astype(np.uint8)
    is_seed = hashed_unit(gw * gh, seed).reshape(gh, gw) < share
    hole = np.zeros((gh, gw), bool)
    hole[gh // 2 - 6:gh // 2 + 6, gw // 2 - 8:gw // 2 + 8] = True
    is_seed &= ~hole
    is_seed[:, :3] = False
    rho = np.where(is_seed, (1.0 / truth).astype(F32), F32(0)).astype(F32)
    w = np.where(is_seed, 8, 0).astype(np.uint8)
    return dict(truth=truth, guide=guide, near=near, rho=rho, w=w, hole=hole, edge_x=edge_x, seed=is_seed)


def T_cp(k_prev, k_cur):
    """R_cp row-major then t_cp, X_cur = R_cp X_prev + t_cp, between two frames of synth.plane_camera_pose"""
    return Dc.T_rc(k_prev, k_cur)


def state_of(truth_grid, seed, lo=1, hi=200, share=0.8):
    """a state from an analytic depth grid: rho = 1 / depth on a hashed `share` of the cells, hashed weights lo..hi"""
    n = truth_grid.size
    on = hashed_unit(n, seed) < share
    rho = np.where(on, (1.0 / truth_grid.reshape(-1)).astype(F32), F32(0)).astype(F32)
    w = np.where(on, lo + hashed(n, seed + 1) % (hi - lo + 1), 0).astype(np.uint8)
    return rho.reshape(truth_grid.shape), w.reshape(truth_grid.shape)


def measurement_of(truth_grid, seed, err=0.02, share0=0.7):
    """a sweep-like measurement: depth = truth (1 + hashed error in +-err) where the hashed code is 0 (a `share0` of the cells), else 0 with
    a code 1..5; hashed conf"""
    n = truth_grid.size
    code = np.where(hashed_unit(n, seed) < share0, 0, 1 + hashed(n, seed + 1) % 5).astype(np.uint8)
    e = (hashed_unit(n, seed + 2) * 2 - 1) * err
    depth = np.where(code == 0, truth_grid.reshape(-1) * (1 + e), 0).astype(F32)
    conf = (hashed(n, seed + 3) % 256).astype(np.uint8)
    s = truth_grid.shape
    return depth.reshape(s), conf.reshape(s), code.reshape(s)


# ---------------------------------------------------------------------------------------------------- the case tables
# Measured with this restatement (tests/test_dense_cases.py prints them; its assertions are the conditions themselves -- strictly below,
# at least twice -- and none of these values):
#   fusion of K = 4 measurements with errors of +-2 %: the median relative error of a single measurement and of the fused image
#   fill on two_surface_grid(seed 1) with 30 % and 5 % seeds: over the hole the median and the largest relative error of the fill and of
#   the nearest-seed fill; in the band of 3 cells about the edge the share within 3 % of the truth, edge-aware and plain (E = 1)
#   the sweep's dense scenes (fuse without a state, fill at max_level 5): the share of the filled cells within 3 % of the analytic depth
DENSE_FILL_MEASURED = {
    "fusion_median_single": 0.00999, "fusion_median_fused": 0.00397,
    "seeds_30": dict(hole_median=(0.00251, 0.00335), hole_max=(0.0438, 0.4694), band_within3=(0.883, 0.277)),
    "seeds_05": dict(hole_median=(0.00359, 0.00375), hole_max=(0.0392, 0.4828), band_within3=(0.913, 0.070)),
    "dense_40_10_r2_filled_within3": 0.472,   # its holes lie where the reference frame sees nothing: median error of the filled 0.0575
    "dense_90_60_r2_filled_within3": 0.903,   # median error of the filled cells 0.0045
}


def _fuse_case(prev, T, calib8, width, height, step, meas, **kw):
    return dict(prev=prev, T=np.asarray(T, np.float64), calib8=tuple(calib8), width=width, height=height, step=step, meas=meas, kw=kw)


@functools.lru_cache(maxsize=None)
def fuse_cases():
    """name -> dict(prev (rho, w) or None, T [12], calib8, width, height, step, meas (depth, conf, code) or None, kw for fuse /
    Context.depth_fuse).  Grids of 64 x 48 (images 256 x 192) and 16 x 16 (64 x 64)."""
    out = {}
    cal = Dc.calib_of()
    tp, tc = Dc.two_depth_frame(10)[1], Dc.two_depth_frame(40)[1]
    prev = state_of(Dc.grid_truth(tp, 4), 11)
    meas = measurement_of(Dc.grid_truth(tc, 4), 21)
    T = T_cp(10, 40)
    out["scene_10_to_40"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, meas)
    out["no_previous_state"] = _fuse_case(None, T, cal, Dc.W, Dc.H, 4, meas)
    out["no_measurement"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, None)
    out["neither"] = _fuse_case(None, T, cal, Dc.W, Dc.H, 4, None)
    cald = Dc.calib_of(dist=Dc.K_DIST4)
    prevd = state_of(Dc.grid_truth(Dc.two_depth_frame(10, dist=Dc.K_DIST4)[1], 4), 12)
    measd = measurement_of(Dc.grid_truth(Dc.two_depth_frame(40, dist=Dc.K_DIST4)[1], 4), 22)
    out["distorted_10_to_40"] = _fuse_case(prevd, T, cald, Dc.W, Dc.H, 4, measd)
    out["decay_0"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, meas, decay=0)
    out["decay_256"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, meas, decay=256)
    out["w_max_40_saturates"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, meas, decay=256, w_max=40)
    out["rel_tol_tight"] = _fuse_case(prev, T, cal, Dc.W, Dc.H, 4, meas, rel_tol=0.004)
    # ---- 64 x 64
    w = h = 64
    cal = Dc.calib_of(w, h, 58.0)
    tp, tc = Dc.two_depth_frame(10, w, h, 58.0)[1], Dc.two_depth_frame(40, w, h, 58.0)[1]
    prev, meas = state_of(Dc.grid_truth(tp, 4), 13), measurement_of(Dc.grid_truth(tc, 4), 23)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    # every source lands on the principal point's cell; three inverse depths only, so most of the 256 keys tie in rho'
    three = np.array([0.25, 0.3125, 0.375], F32)[hashed(256, 5) % 3].reshape(16, 16)
    collapse = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], np.float64)
    out["collapse_all_into_one_ties"] = _fuse_case((three, np.full((16, 16), 77, np.uint8)), collapse, cal, w, h, 4, meas)
    shrink = np.array([0.25, 0, 0, 0, 0.25, 0, 0, 0, 1, 0, 0, 0], np.float64)   # sixteen sources per target cell
    out["shrink_quarter_ties"] = _fuse_case((three, prev[1]), shrink, cal, w, h, 4, meas)
    out["leaving_the_grid"] = _fuse_case(prev, np.concatenate([ident[:9], [1.6, -0.9, 0.0]]), cal, w, h, 4, meas)
    out["behind_the_camera"] = _fuse_case(prev, np.concatenate([ident[:9], [0.0, 0.0, -3.0]]), cal, w, h, 4, meas)   # P.z = 1 - 3 rho
    out["all_behind"] = _fuse_case(prev, np.concatenate([ident[:9], [0.0, 0.0, -9.0]]), cal, w, h, 4, None)
    out["identity_16x16"] = _fuse_case(prev, ident, cal, w, h, 4, meas)
    p1, m1 = state_of(tp, 14), measurement_of(tc, 24)
    out["step1"] = _fuse_case(p1, T, cal, w, h, 1, m1)
    p16, m16 = state_of(Dc.grid_truth(tp, 16), 15, share=1.0), measurement_of(Dc.grid_truth(tc, 16), 25)
    out["step16"] = _fuse_case(p16, T, cal, w, h, 16, m16)
    g8 = (Dc.grid_truth(tp[:, :60], 8), Dc.grid_truth(tc[:, :60], 8))   # 60 / 8 truncates to 7 columns
    out["width60_step8"] = _fuse_case(state_of(g8[0], 16), T, cal, 60, h, 8, measurement_of(g8[1], 26))
    return out


@functools.lru_cache(maxsize=None)
def oracle_fuse(name):
    c = fuse_cases()[name]
    return fuse(c["prev"], c["T"], c["calib8"], c["width"], c["height"], c["step"], c["meas"], **c["kw"])


def _fill_case(rho, w, gray, step, rho_ref, max_level, width=None, pad=0):
    return dict(rho=np.ascontiguousarray(rho, F32), w=np.ascontiguousarray(w, np.uint8), gray=np.ascontiguousarray(gray, np.uint8), step=step,
                rho_ref=float(rho_ref), max_level=max_level, width=width, pad=pad)


E_STEP_DIFFS = (7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 55, 56)   # |G_cell - G_parent| on both sides of every step of E


def e_step_guide():
    """16 columns x 28 rows: in row pair r every 2 x 2 block is (a, a + 2 d_r) per row, so its parent's guide is a + d_r and both children
    differ from it by exactly d_r"""
    g = np.zeros((2 * len(E_STEP_DIFFS), 16), np.int64)
    for r, d in enumerate(E_STEP_DIFFS):
        g[2 * r:2 * r + 2, 0::2] = 40
        g[2 * r:2 * r + 2, 1::2] = 40 + 2 * d
    return g.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fill_cases():
    """name -> dict(rho, w [gh,gw], gray [h,w] u8, step, rho_ref, max_level, width (or None), pad (extra bytes per row on the device))"""
    out = {}
    img, truth, _ = Dc.two_depth_frame(40)
    g4 = Dc.grid_truth(truth, 4)
    rho, w = state_of(g4, 31, lo=1, hi=128, share=0.3)
    ref = 2.0 / 1.5
    for L in (1, 2, 4, 5, 8):
        out["scene_64x48_L%d" % L] = _fill_case(rho, w, img, 4, ref, L)
    out["pitch_pad_16"] = _fill_case(rho, w, img, 4, ref, 5, pad=16)
    s = two_surface_grid()
    out["two_surface_L5"] = _fill_case(s["rho"], s["w"], s["guide"], 1, 1.0, 5)
    out["two_surface_L8"] = _fill_case(s["rho"], s["w"], s["guide"], 1, 1.0, 8)
    # sizes that are no multiple of the tile or of 2
    for gw_, gh_, L in ((7, 5, 3), (1, 1, 1), (1, 1, 8), (37, 29, 3), (50, 33, 5), (33, 65, 6), (17, 1, 4), (1, 19, 5)):
        n = gw_ * gh_
        t = 2.0 + hashed_unit(n, 40 + gw_).reshape(gh_, gw_)
        r_, w_ = state_of(t, 41 + gh_, share=0.2 if n > 1 else 1.0)
        gray = (hashed(n, 43 + gw_) % 256).reshape(gh_, gw_)
        out["odd_%dx%d_L%d" % (gw_, gh_, L)] = _fill_case(r_, w_, gray, 1, 1.0, L)
    # 64 x 64 image, step 4: a single seed in a corner
    img64 = Dc.two_depth_frame(40, 64, 64, 58.0)[0]
    for name, (y, x) in (("corner_seed_00", (0, 0)), ("corner_seed_15_15", (15, 15))):
        r_, w_ = np.zeros((16, 16), F32), np.zeros((16, 16), np.uint8)
        r_[y, x], w_[y, x] = 0.3, 9
        for L in (4, 8):
            out["%s_L%d" % (name, L)] = _fill_case(r_, w_, img64, 4, 1.0, L)
        out[name + "_flat_guide_L4"] = _fill_case(r_, w_, np.full((64, 64), 90, np.uint8), 4, 1.0, 4)
    out["no_seed"] = _fill_case(np.zeros((16, 16), F32), np.zeros((16, 16), np.uint8), img64, 4, 1.0, 5)
    t16 = Dc.grid_truth(Dc.two_depth_frame(40, 64, 64, 58.0)[1], 4)
    r_, w_ = state_of(t16, 51, share=1.0)
    out["all_seeds"] = _fill_case(r_, w_, img64, 4, 1.0, 5)
    # q clips at both ends: rho / rho_ref 65536 above 2^20 - 1, and rounding to 0
    r_, w_ = state_of(t16, 52, share=0.4)
    r_ = np.where(hashed(256, 53).reshape(16, 16) % 3 == 0, F32(40.0), np.where(hashed(256, 54).reshape(16, 16) % 3 == 0, F32(1e-6), r_)).astype(F32)
    r_ = np.where(w_ > 0, r_, F32(0)).astype(F32)
    out["q_clips_both_ends"] = _fill_case(r_, w_, img64, 4, 1.0, 4)
    g = e_step_guide()
    r_, w_ = state_of(2.0 + hashed_unit(g.size, 61).reshape(g.shape), 62, share=0.25)
    out["guide_on_every_E_step"] = _fill_case(r_, w_, g, 1, 1.0, 3)
    t8 = Dc.grid_truth(Dc.two_depth_frame(40, 64, 64, 58.0)[1][:, :60], 8)
    r_, w_ = state_of(t8, 63, share=0.3)
    out["width60_step8"] = _fill_case(r_, w_, img64, 8, 1.0, 3, width=60)
    return out


@functools.lru_cache(maxsize=None)
def oracle_fill(name):
    c = fill_cases()[name]
    return fill(c["rho"], c["w"], c["gray"], c["step"], c["rho_ref"], c["max_level"], width=c["width"])
