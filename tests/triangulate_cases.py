"""TEST INFRASTRUCTURE: triangulation cases that sit on the gates of triangulate.hip -- scenes, a case table and a numpy restatement of
the per-point arithmetic (same IEEE double operations in the same order as orc_triangulate, so its intermediate values -- rPoint, the
float projections, lDist, rDist -- are the oracle's).  test_triangulate_cases.py (CPU) asserts that every scene reaches what it is named
for; test_gpu_triangulate_cases.py runs the same cases on the GPU against the oracle, bit for bit.

  depth_l / depth_r    lPoint.z (rPoint.z) runs through 0.1 in steps of one ulp of a bearing component      `lp[2] < 0.1`, `rp[2] < 0.1`
  reproj_l / reproj_r  unpx_l (unpx_r) = the float projection + an offset that runs through 3.0 in steps of one float ulp of the pixel
                       coordinate, along +x, -x, +y, -y (distance == 3.0 exactly on the gate) and along a diagonal whose double norm is
                       not 3.0 but rounds to 3.0f                                                             `lDist > maxErr`, `rDist > maxErr`
  parallel             parallel and near-parallel bearings, zero baseline, bearings with f2u.z <= 0         a00 a11 - a10 a01 == 0, NaN
  scene-n              an ordinary scene at n = 1, 255, 256, 257, 513                                       the 256-thread block edge
  groups               8 transform blocks, unsorted group indices, one block unused, the last used once     T + 36 group[i]
  limit-e              the scene and the reprojection sweep at maxErr = 0, 3, 1e9, +inf"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from alvaar_amd import synth

K = (520.0, 520.0, 320.0, 240.0)
MAX_ERR = 3.0
SWEEP = 150            # depth sweeps: this many one-ulp steps on each side of the gate
AXIS_STEPS = 20        # reprojection sweeps: this many float ulps on each side of the gate
F32_ULP = 2.0 ** -15   # spacing of float pixel coordinates in [256, 512)


# ---- transform blocks ----------------------------------------------------------------------------------------------------------------
def quat_R(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def transform_blocks(pose_kf, pose_new):
    """T [nGroups, 36] = (R_lr, t_lr, R_rl, t_rl, R_wl, t_wl) of every keyframe pose7 (t, q = x y z w) against the new keyframe's"""
    Rn, tn = quat_R(pose_new[3:]), np.asarray(pose_new[:3], np.float64)
    T = np.zeros((len(pose_kf), 36))
    for g, p in enumerate(pose_kf):
        Rk, tk = quat_R(p[3:]), np.asarray(p[:3], np.float64)
        Rlr, tlr = Rk.T @ Rn, Rk.T @ (tn - tk)
        T[g] = np.concatenate([Rlr.ravel(), tlr, Rlr.T.ravel(), -Rlr.T @ tlr, Rk.ravel(), tk])
    return T


IDENT = (0.0, 0.0, 0.0, 1.0)


def pose7(t, q=IDENT):
    return np.array(list(t) + list(q), np.float64)


# ---- restatement -----------------------------------------------------------------------------------------------------------------------
def restate(T, group, bvl, bvr, unpxl, unpxr, K=K, max_err=MAX_ERR):
    """orc_triangulate in numpy, with the intermediate values the gates read"""
    fx, fy, cx, cy = (float(v) for v in K)
    G = np.asarray(T, np.float64)[np.asarray(group)]
    f1, f2 = np.asarray(bvl, np.float64), np.asarray(bvr, np.float64)
    ul, ur = np.asarray(unpxl, np.float32), np.asarray(unpxr, np.float32)

    def matvec(R, v):
        return np.stack([(R[:, 3 * i] * v[:, 0] + R[:, 3 * i + 1] * v[:, 1]) + R[:, 3 * i + 2] * v[:, 2] for i in range(3)], 1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def project(p):
        iz = 1. / p[:, 2]
        return (fx * (p[:, 0] * iz) + cx).astype(np.float32), (fy * (p[:, 1] * iz) + cy).astype(np.float32)

    def norm2f(dx, dy):
        dx, dy = dx.astype(np.float64), dy.astype(np.float64)
        return np.sqrt(dx * dx + dy * dy)

    with np.errstate(all="ignore"):
        tlr = G[:, 9:12]
        f2u = matvec(G[:, 0:9], f2)
        ru, rv = project(f2u)
        parallax = norm2f(ul[:, 0] - ru, ul[:, 1] - rv)
        b0, b1 = dot(tlr, f1), dot(tlr, f2u)
        a00, a10, a11 = dot(f1, f1), dot(f1, f2u), -dot(f2u, f2u)
        a01 = -a10
        det = a00 * a11 - a10 * a01
        invdet = 1.0 / det
        i00, i10, i01, i11 = a11 * invdet, -a10 * invdet, -a01 * invdet, a00 * invdet
        l0, l1 = i00 * b0 + i01 * b1, i10 * b0 + i11 * b1
        lp = (l0[:, None] * f1 + (tlr + l1[:, None] * f2u)) / 2
        rp = matvec(G[:, 12:21], lp) + G[:, 21:24]
        wp = matvec(G[:, 24:33], lp) + G[:, 33:36]
        lu, lv = project(lp)
        pu, pv = project(rp)
        ldist_d, rdist_d = norm2f(lu - ul[:, 0], lv - ul[:, 1]), norm2f(pu - ur[:, 0], pv - ur[:, 1])
        ldist, rdist = ldist_d.astype(np.float32), rdist_d.astype(np.float32)
        me = np.float32(max_err)
        behind = (lp[:, 2] < 0.1) | (rp[:, 2] < 0.1)
        status = np.where(behind, 1, np.where((ldist > me) | (rdist > me), 2, 0)).astype(np.uint8)
        return dict(lpt=lp, wpt=wp, inv_depth=1. / lp[:, 2], status=status, parallax=parallax, rpt=rp, det=det, lproj=np.stack([lu, lv], 1),
                    rproj=np.stack([pu, pv], 1), ldist=ldist, rdist=rdist, ldist_d=ldist_d, rdist_d=rdist_d)


OUT_KEYS = ("lpt", "wpt", "inv_depth", "status", "parallax")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _pix(p):
    """the float pixel of a camera-frame point"""
    return np.array([K[0] * p[0] / p[2] + K[2], K[1] * p[1] / p[2] + K[3]]).astype(np.float32)


def _step64(x, k):
    """x moved by k ulps (x > 0)"""
    return (np.full(np.shape(k), x, np.float64).view(np.int64) + np.asarray(k, np.int64)).view(np.float64)


def _scene(pose_kf, pose_new, group, bvl, bvr, unpxl, unpxr, **extra):
    pose_kf, pose_new = np.atleast_2d(np.asarray(pose_kf, np.float64)), np.asarray(pose_new, np.float64)
    s = dict(pose_kf=pose_kf, pose_new=pose_new, T=transform_blocks(pose_kf, pose_new), group=np.ascontiguousarray(group, np.int32),
             bvl=np.ascontiguousarray(bvl, np.float64), bvr=np.ascontiguousarray(bvr, np.float64),
             unpxl=np.ascontiguousarray(unpxl, np.float32), unpxr=np.ascontiguousarray(unpxr, np.float32))
    s.update(extra)
    for v in s.values():
        v.setflags(write=False)
    return s


def inputs(s):
    """the arguments of orc_triangulate / ctx.triangulate / restate, in order (without K and maxErr)"""
    return s["T"], s["group"], s["bvl"], s["bvr"], s["unpxl"], s["unpxr"]


# ---- depth gate sweeps -----------------------------------------------------------------------------------------------------------------
def _depth_sweep(right):
    """Identity rotations, one point.  left: the point is 0.1 in front of the keyframe and 0.2 in front of the new frame, and the x component
    of the left bearing moves by one ulp per row; right: the other way round.  The rows are centred on the pair of neighbouring steps
    between which the restated status changes (found by bisection over the step count)."""
    X = np.array([0.03, 0.02, 0.2 if right else 0.1])
    tn = np.array([0.05, 0.0, 0.1 if right else -0.1])
    f1, f2 = _unit(X), _unit(X - tn)
    pose_kf, pose_new = pose7((0, 0, 0)), pose7(tn)
    ul, ur = _pix(X), _pix(X - tn)

    def scene(k):
        k = np.atleast_1d(np.asarray(k, np.int64))
        n = len(k)
        bl, br = np.tile(f1, (n, 1)), np.tile(f2, (n, 1))
        (br if right else bl)[:, 0] = _step64((f2 if right else f1)[0], k)
        return _scene(pose_kf, pose_new, np.zeros(n, np.int32), bl, br, np.tile(ul, (n, 1)), np.tile(ur, (n, 1)), step=k)

    def status(k):
        return int(restate(*inputs(scene(k)))["status"][0])

    lo, hi = -(1 << 24), 1 << 24
    slo, shi = status(lo), status(hi)
    assert {slo, shi} == {0, 1}, (slo, shi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if status(mid) == slo:
            lo = mid
        else:
            hi = mid
    return scene(lo + np.arange(-SWEEP + 1, SWEEP + 1))


# ---- reprojection gate sweeps ----------------------------------------------------------------------------------------------------------
AXES = ("+x", "-x", "+y", "-y", "diag", "zero")
DIAG_SEARCH = 4000   # candidate x offsets tried on each side of 3 / sqrt(2)
DIAG_KEEP = 4        # kept of each kind: double norm below 3.0 and above 3.0, both rounding to 3.0f


def _reproj_sweep(right):
    """One well-triangulated point.  The swept image's observation is the float projection of the restated point plus an offset; the other
    image's is its float projection exactly.  Rows carry (axis, j): along an axis the offset is +-(3 + j ulp), j = -20 .. 20, so that row j = 0
    has distance 3.0 exactly and row j + 1 is its upper neighbour; the diagonal rows come in triples (j = -1, 0, 1) around offsets whose
    double norm is not 3.0 but rounds to 3.0f; `zero` is the projection itself (distance 0)."""
    pose_kf = pose7((0, 0, 0))
    pose_new = pose7((0.6, 0.05, 0.1), tuple(synth._quat_from_R(synth.so3_exp(np.array([0.01, 0.05, -0.02])))))
    X = np.array([0.5, 0.55, 5.0])        # projects near (372, 297) and (290, 300): every row stays inside [256, 512), where float pixels step by 2^-15
    Rn, tn = quat_R(pose_new[3:]), pose_new[:3]
    f1, f2 = _unit(X), _unit(Rn.T @ (X - tn))
    base = _scene(pose_kf, pose_new, [0], f1[None], f2[None], np.zeros((1, 2)), np.zeros((1, 2)))
    r0 = restate(*inputs(base))
    pl, pr = r0["lproj"][0], r0["rproj"][0]
    centre = pr if right else pl
    assert r0["status"][0] == 2 and (centre > 264).all() and (centre < 504).all()   # (status 2: the placeholder observations are far away)
    u = np.float32(F32_ULP)
    offs, axis, jj = [(0.0, 0.0)], [AXES.index("zero")], [0]
    for a, (sx, sy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        for j in range(-AXIS_STEPS, AXIS_STEPS + 1):
            d = MAX_ERR + j * F32_ULP
            offs.append((sx * d, sy * d))
            axis.append(a)
            jj.append(j)
    # diagonal: dx = a multiple of the ulp near 3 / sqrt(2), dy = the multiple of the ulp nearest sqrt(9 - dx^2); keep those whose distance
    # is 3.0f after the float cast although the double norm is not 3.0
    i = np.arange(-DIAG_SEARCH, DIAG_SEARCH + 1)
    dx = (np.rint(MAX_ERR / np.sqrt(2.0) / F32_ULP) + i) * F32_ULP
    dy = np.rint(np.sqrt(MAX_ERR * MAX_ERR - dx * dx) / F32_ULP) * F32_ULP
    nd = np.sqrt(dx * dx + dy * dy)
    hit = (nd.astype(np.float32) == np.float32(MAX_ERR)) & (nd != MAX_ERR)
    below, above = np.flatnonzero(hit & (nd < MAX_ERR))[:DIAG_KEEP], np.flatnonzero(hit & (nd > MAX_ERR))[:DIAG_KEEP]
    for k in np.concatenate([below, above]):
        for j in (-1, 0, 1):
            offs.append((-dx[k], -(dy[k] + j * F32_ULP)))      # observation = projection - offset: lu - ulx = +dx
            axis.append(AXES.index("diag"))
            jj.append(j)
    offs = np.array(offs, np.float64)
    n = len(offs)
    obs = (centre.astype(np.float64)[None] - offs).astype(np.float32)   # exact: multiples of the ulp inside one binade
    assert np.array_equal(obs.astype(np.float64), centre.astype(np.float64)[None] - offs)
    ul, ur = (np.tile(pl, (n, 1)), obs) if right else (obs, np.tile(pr, (n, 1)))
    return _scene(pose_kf, pose_new, np.zeros(n, np.int32), np.tile(f1, (n, 1)), np.tile(f2, (n, 1)), ul, ur, axis=np.array(axis, np.int32),
                  j=np.array(jj, np.int32))


# ---- parallel and near-parallel bearings -----------------------------------------------------------------------------------------------
# name -> (group, left bearing, right bearing, lPoint is NaN, parallax is finite); group 0 has baseline (0.1, 0, 0), group 1 none; identity
# rotations throughout.  Observations are the pixels of the bearings.
PARALLEL = {
    "parallel_z": (0, (0, 0, 1), (0, 0, 1), True, True),
    "parallel_oblique": (0, (0.6, 0, 0.8), (0.6, 0, 0.8), True, True),
    "parallel_unnormalised": (0, (0.5, 0.25, 1), (0.5, 0.25, 1), True, True),
    "diverging_1e-3": (0, _unit((0, 0, 1)), _unit((1e-3, 0, 1)), False, True),      # meets 100 behind the cameras: status 1
    "converging_1e-3": (0, _unit((0, 0, 1)), _unit((-1e-3, 0, 1)), False, True),    # meets 100 in front
    "diverging_1e-7": (0, _unit((0, 0, 1)), _unit((1e-7, 0, 1)), False, True),      # determinant 1e-14
    "diverging_1e-9": (0, _unit((0, 0, 1)), _unit((1e-9, 0, 1)), True, True),       # 1e-18 is below the double's resolution: determinant 0
    "zero_baseline": (1, _unit((0.1, 0.05, 1)), _unit((0.12, 0.05, 1)), False, True),     # lPoint = 0: status 1, inverse depth +inf
    "zero_baseline_parallel": (1, (0, 0, 1), (0, 0, 1), True, True),                      # 0 * inf
    "f2u_z_zero": (0, _unit((0.1, 0, 1)), (1, 0, 0), False, False),                       # 1 / 0 in the parallax projection
    "f2u_z_zero_y": (0, _unit((0.1, 0, 1)), (0, 1, 0), False, False),
    "f2u_z_negative": (0, _unit((0.1, 0, 1)), _unit((0.3, 0.1, -1)), False, True),
    "f1_z_zero": (0, (1, 0, 0), _unit((-0.1, 0, 1)), False, True),
    "ordinary": (0, _unit((0.02, 0.01, 1)), _unit((-0.03, 0.01, 1)), False, True),        # depth 2, between the hostile rows
}


def _parallel():
    names = list(PARALLEL)
    with np.errstate(all="ignore"):
        bl = np.array([PARALLEL[k][1] for k in names], np.float64)
        br = np.array([PARALLEL[k][2] for k in names], np.float64)
        pix = lambda b: np.nan_to_num(np.stack([K[0] * b[:, 0] / b[:, 2] + K[2], K[1] * b[:, 1] / b[:, 2] + K[3]], 1), nan=0.0, posinf=1e6, neginf=-1e6)
        return _scene([pose7((0, 0, 0)), pose7((0.1, 0, 0))], pose7((0.1, 0, 0)), [PARALLEL[k][0] for k in names], bl, br, pix(bl), pix(br))


# ---- ordinary scenes, group layouts ----------------------------------------------------------------------------------------------------
def _synth(n, ng, seed):
    pb = synth.make_triangulation_problem(n, ng, seed)
    assert pb["K"] == K
    return _scene(pb["pose_kf"], pb["pose_new"], pb["group"], pb["bvl"], pb["bvr"], pb["unpxl"], pb["unpxr"])


GROUP_ORDER = (5, 0, 6, 2, 1, 4)   # where the six keyframes of the synthetic scene go among 8 blocks: 3 stays unused, 7 is the last point's


def _groups():
    pb = synth.make_triangulation_problem(300, len(GROUP_ORDER), 23)
    pose_kf = np.zeros((8, 7))
    pose_kf[:, 6] = 1.0
    pose_kf[3, :3] = (7.0, -3.0, 2.0)          # read by no point
    group = np.array(GROUP_ORDER, np.int32)[pb["group"]]
    pose_kf[list(GROUP_ORDER)] = pb["pose_kf"]
    pose_kf[7] = pose_kf[group[-1]]
    group[-1] = 7
    return _scene(pose_kf, pb["pose_new"], group, pb["bvl"], pb["bvr"], pb["unpxl"], pb["unpxr"])


SIZES = (1, 255, 256, 257, 513)
LIMITS = (0.0, 3.0, 1e9, float("inf"))
_SCENES = {"depth_l": lambda: _depth_sweep(False), "depth_r": lambda: _depth_sweep(True), "reproj_l": lambda: _reproj_sweep(False),
           "reproj_r": lambda: _reproj_sweep(True), "parallel": _parallel, "groups": _groups}
_SCENES.update({f"scene-{n}": functools.partial(_synth, n, 3, 40 + k) for k, n in enumerate(SIZES)})
SWEEPS = ("depth_l", "depth_r", "reproj_l", "reproj_r")


@functools.lru_cache(maxsize=None)
def scene(name):
    return _SCENES[name]()


Case = namedtuple("Case", "id scene max_err")
CASES = tuple([Case(name, name, MAX_ERR) for name in _SCENES]
              + [Case(f"limit-{e:g}-{s}", s, e) for e in LIMITS for s in ("scene-257", "reproj_l", "parallel") if not (e == MAX_ERR)])
CASE_IDS = tuple(c.id for c in CASES)
GOLDEN_IDS = tuple(c.id for c in CASES if c.scene in ("parallel", "groups", "scene-257"))   # the reference pin: no sweeps, one size


def case(case_id):
    return next(c for c in CASES if c.id == case_id)


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """orc_triangulate's outputs of a case, computed once and read-only"""
    from oracles import orc_triangulate
    c = case(case_id)
    o = orc_triangulate(*inputs(scene(c.scene)), K, c.max_err)
    for v in o.values():
        v.setflags(write=False)
    return o


def same_bits(a, b):
    """bit for bit, except that where b is NaN a must be NaN (any sign and payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(b)
    ints = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(ints)[~nan], b.view(ints)[~nan]))


# ---- the reference pin -----------------------------------------------------------------------------------------------------------------
TOL = 1e-11          # test_triangulate._compare's rule: the reference rotates with quaternions, the restatement with the equivalent matrices
GATE_BAND = 1e-6


def near_gate(r, max_err):
    """rows whose status may differ between two implementations that agree to TOL: a gate value within GATE_BAND of its threshold"""
    with np.errstate(all="ignore"):
        me = np.float64(max_err)
        return ((np.abs(r["lpt"][:, 2] - 0.1) < GATE_BAND) | (np.abs(r["rpt"][:, 2] - 0.1) < GATE_BAND)
                | (np.abs(r["ldist_d"] - me) < GATE_BAND) | (np.abs(r["rdist_d"] - me) < GATE_BAND))


def close_to_reference(got, want, r, max_err):
    """None, or what differs: values to TOL relative (non-finite ones alike: NaN where NaN, the same infinity), parallax to 1e-4 pixels,
    statuses exact outside near_gate"""
    free = near_gate(r, max_err)
    if not np.array_equal(got["status"][~free], want["status"][~free]):
        return "status"
    for k, tol in (("lpt", TOL), ("wpt", TOL), ("inv_depth", TOL), ("parallax", 1e-4)):
        a, b = got[k], want[k]
        fin = np.isfinite(b)
        if not (np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])):
            return k + " (non-finite)"
        scale = np.maximum(1.0, np.abs(b[fin])) if tol == TOL else 1.0
        if fin.any() and (np.abs(a[fin] - b[fin]) / scale).max() >= tol:
            return k
    return None


def golden_case(z, case_id):
    """(scene inputs with the reference's transform blocks, the reference's outputs) of a case in tests/golden/triangulate_cases.npz"""
    c = case(case_id)
    s = {k: z[f"s_{c.scene}_{k}"] for k in ("T", "group", "bvl", "bvr", "unpxl", "unpxr")}
    return s, {k: z[f"c_{case_id}_{k}"] for k in OUT_KEYS}
