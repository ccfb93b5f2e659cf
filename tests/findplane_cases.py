"""alva_find_plane (alvaar_amd/csrc/find_plane.hip) restated in numpy, and the table of its edge cases.  numpy only, no GPU.

THE DISCRETE STAGE IS EXACT.  Up to and including the inlier set, the library computes a written sequence of single-rounded float32 and
float64 operations (it is built with -ffp-contract=off and correctly rounded float divide and sqrt), so restate() reproduces it bit for
bit: float32 arrays with one rounding per operation, float64 for the cross product and the orientation gate, np.sort(dist)[kth] for the
score.  tests/test_findplane_cases.py pins it to the C restatement oracle/alva_oracle_plane.c, tests/test_gpu_find_plane_cases.py holds
the kernels to it with no tolerance.  After the inlier set the sums are order-dependent and the eigenvector comes from another solver:
restate() gives them in float64 (math.fsum, numpy.linalg.eigh) and the tests bound the difference.

Every case of cases() is a small (points, pose7, samples3); build_cases() asserts ON THE RESTATEMENT ALONE that each case is what its
name says -- so that a kernel that takes rank kth +- 1, compares `<=` for `<` in the threshold or in the argmin, or evaluates the
orientation gate in float, must differ from the restatement in a named case (see SENTINELS at the end of this file)."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
SIN_TH_BITS = 0x3DB27EB6     # sinf(5.0f * 3.14159265358979323846f / 180.0f); pinned through the gate twins (test_findplane_cases.py)
SIN_TH = np.array([SIN_TH_BITS], np.uint32).view(F32)[0]
N_MIN, N_MAX, MIN_INLIERS = 32, 12288, 32
BEST_INIT = F32(1e10)
POSE_BASE = np.array([0.1, -0.05, 0.2, 0.0, 0.0, 0.0, 1.0])     # tests/test_plane.py's


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def kth_of(n):
    return max(int(0.2 * n), 20)


# ------------------------------------------------------------------------------------------------------------ the exact stage
def plane_of(P32, tri):
    """find_plane.hip plane_of: the unit 4-vector (a, b, c, d) as float32, or None for a triple without a plane"""
    p0, p1, p2 = (tuple(float(v) for v in P32[i]) for i in tri)           # the float copies, widened: every operation below is a double's
    u = (p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2])
    w = (p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2])
    pl = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
    pl.append(-(pl[0] * p0[0] + pl[1] * p0[1] + pl[2] * p0[2]))
    nn = math.sqrt(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2] + pl[3] * pl[3])
    if not nn > 0:
        return None
    return tuple(F32(v / nn) for v in pl)


def gate_value(a, b):
    """what the orientation gate compares with sinTh, in double"""
    return math.sqrt(float(b) * float(b) + float(a) * float(a))


def gate_value_float(a, b):
    """the same in float: NOT what the code does (a sentinel case tells the two apart)"""
    return np.sqrt(F32(b) * F32(b) + F32(a) * F32(a))


def plane_dists(P32, pl):
    a, b, c, d = pl
    f = F32(1.0) / np.sqrt(a * a + b * b + c * c + d * d)
    return np.abs(P32[:, 0] * a + P32[:, 1] * b + P32[:, 2] * c + d) * f


def restate(P, pose7, S, want_pose=True):
    """The whole of alva_find_plane.  P [n,3] float64, pose7 = Twc (t, q = x y z w), S [iters,3] int.  Returns a dict:
    launched, kth, scores [iters] f32 (+inf: skipped), planes [iters,4] f32 (zero where skipped), accepted, best, best_score f32, inlier
    [n] u8, n_in, found, and for n_in > 0 moments [13] f64 (math.fsum) with moment_abs [13] (the fsum of the terms' magnitudes) and
    moment_terms (the terms themselves), and for found cases pose [16] f32 with origin [3] f32 and eig (the four eigenvalues)."""
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    S = np.asarray(S).reshape(-1, 3)
    n, iters = len(P), len(S)
    r = dict(n=n, iters=iters, kth=kth_of(n), launched=n >= N_MIN, scores=np.full(iters, np.inf, F32), planes=np.zeros((iters, 4), F32),
             accepted=0, best=-1, best_score=BEST_INIT, inlier=np.zeros(n, np.uint8), n_in=0, found=False, pose=None)
    if n < N_MIN:
        return r
    assert n <= N_MAX and iters > 0 and S.min() >= 0 and S.max() < n
    P32 = P.astype(F32)
    for it in range(iters):
        pl = plane_of(P32, S[it])
        if pl is None or gate_value(pl[0], pl[1]) > float(SIN_TH):
            continue
        r["accepted"] += 1
        r["planes"][it] = pl
        r["scores"][it] = np.sort(plane_dists(P32, pl))[r["kth"]]
    for it in range(iters):                       # the first of the smallest
        if r["scores"][it] < r["best_score"]:
            r["best_score"], r["best"] = r["scores"][it], it
    threshold = F32(1.4) * r["best_score"]
    dist = plane_dists(P32, tuple(r["planes"][r["best"]])) if r["best"] >= 0 else np.zeros(n, F32)
    r["dist"], r["threshold"] = dist, threshold
    inl = dist < threshold
    r["inlier"], r["n_in"] = inl.astype(np.uint8), int(inl.sum())
    if r["n_in"] == 0:
        return r
    # ---- float64 from here: the ten entries of M (upper triangle, row by row) and the three sums; products of two floats are exact
    Q = np.column_stack([P32[inl].astype(np.float64), np.ones(r["n_in"])])
    terms = [Q[:, x] * Q[:, y] for x in range(4) for y in range(x, 4)] + [Q[:, k] for k in range(3)]
    r["moment_terms"] = terms
    r["moments"] = np.array([math.fsum(t) for t in terms])
    r["moment_abs"] = np.array([math.fsum(np.abs(t)) for t in terms])
    if r["n_in"] < MIN_INLIERS or not want_pose:
        return r
    r["found"] = True
    M = np.zeros((4, 4))
    M[np.triu_indices(4)] = r["moments"][:10]
    M = M + np.triu(M, 1).T
    ev, V = np.linalg.eigh(M)
    r["eig"] = ev
    r["pose"], r["origin"], r["normal"] = pose_from(V[:, 0], r["moments"][10:13], r["n_in"], pose7)
    return r


# ------------------------------------------------------------------------------------------------------------ the host float steps
def _rodrigues(rv):
    th = math.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    if th < 1e-300:
        return np.eye(3)
    k = [rv[0] / th, rv[1] / th, rv[2] / th]
    c, s = math.cos(th), math.sin(th)
    c1 = 1 - c
    K = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    return np.array([[c * (i == j) + c1 * k[i] * k[j] + s * K[i][j] for j in range(3)] for i in range(3)])


def pose_from(v, sums, n_in, pose7):
    """alva_find_plane after the eigenvector v (float64[4]; either sign) and the sums of the inliers' coordinates: one float32 operation
    at a time.  Returns (pose16 f32, origin f32[3], the flipped unit normal f32[3])"""
    a, b, c = F32(v[0]), F32(v[1]), F32(v[2])
    inv = F32(1.0) / F32(n_in)
    origin = np.array([F32(sums[k]) * inv for k in range(3)], F32)
    f = F32(1.0) / np.sqrt(a * a + b * b + c * c)
    p7 = [float(x) for x in pose7]
    qx, qy, qz, qw = p7[3:]
    R = [1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
         2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
         2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]
    t = [F32(p7[0]), F32(p7[1]), F32(p7[2])]
    Oc = [-(F32(R[3 * i]) * t[0] + F32(R[3 * i + 1]) * t[1] + F32(R[3 * i + 2]) * t[2]) for i in range(3)]
    mx = [Oc[k] - origin[k] for k in range(3)]
    if mx[0] * a + mx[1] * b + mx[2] * c > 0:
        a, b, c = -a, -b, -c
    nx, ny, nz = a * f, b * f, c * f
    v3 = [F32(0.0), -nz, ny]
    sa = F32(math.sqrt(float(v3[0]) * float(v3[0]) + float(v3[1]) * float(v3[1]) + float(v3[2]) * float(v3[2])))
    ang = F32(np.arctan2(sa, nx))
    R1 = _rodrigues([float(v3[k] * ang / sa) for k in range(3)])
    R2 = _rodrigues([1.0, 0.0, 0.0])
    out = np.zeros(16, F32)
    for col in range(3):
        for row in range(3):
            s = F32(0.0)
            for k in range(3):
                s = s + F32(R1[row, k]) * F32(R2[k, col])
            out[4 * col + row] = s
    out[12:15] = origin
    out[15] = 1.0
    return out, origin, np.array([nx, ny, nz], F32)


def margins(r):
    """orc_find_plane_margins from the restatement: (accepted, relative gap to the runner-up score, the smallest relative distance of a
    point from the threshold)"""
    if not r["accepted"]:
        return 0, 0.0, 0.0
    others = np.delete(r["scores"], r["best"])
    second = min(float(others.min()) if len(others) else 1e10, 1e10)
    thr = r["threshold"]
    return r["accepted"], (second - float(r["best_score"])) / float(r["best_score"]) if r["best_score"] > 0 else np.inf, \
        float((np.abs(r["dist"] - thr) / thr).min()) if thr > 0 else np.inf


# ------------------------------------------------------------------------------------------------------------ scenes
def scene(n_plane, n_clutter, seed, tilt=0.02, depth=4.0):
    """tests/test_plane.py's _scene: noisy points on a plane that faces the world z axis + clutter, shuffled"""
    rng = np.random.RandomState(seed)
    nrm = np.array([tilt, -0.5 * tilt, 1.0])
    nrm /= np.linalg.norm(nrm)
    xy = rng.uniform(-2, 2, (n_plane, 2))
    z = depth - (nrm[0] * xy[:, 0] + nrm[1] * xy[:, 1]) / nrm[2]
    P = np.column_stack([xy, z]) + 0.004 * rng.randn(n_plane, 3)
    Q = np.column_stack([rng.uniform(-2, 2, (n_clutter, 2)), rng.uniform(1.0, 8.0, n_clutter)])
    pts = np.ascontiguousarray(np.vstack([P, Q]))
    rng.shuffle(pts)
    return pts, POSE_BASE.copy()


def samples(n, iters, seed):
    """tests/test_plane.py's _samples"""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(np.sort(np.array([rng.choice(n, 3, replace=False) for _ in range(iters)]), axis=1).astype(np.int32))


def _f32(x):
    """float64 values that a float cast leaves unchanged"""
    return np.asarray(x, F32).astype(np.float64)


def _step(z, up=True, k=1):
    z = F32(z)
    for _ in range(k):
        z = np.nextafter(z, F32(np.inf if up else -np.inf))
    return z


TRI = np.array([[-1.0, -1.0, 4.0], [1.0, -1.0, 4.0], [0.0, 1.5, 4.0]])     # the plane z = 4, exactly: (a, b, c, d) = (0, 0, 1, -4) / sqrt(17)
C4 = math.sqrt(17.0)                                                        # a point at height z has distance |z - 4| / C4 from it


def _staged(dists, rng, side=None):
    """points at the given distances (of the 4-vector kind: |z - 4| / sqrt 17) from the plane z = 4"""
    dists = np.asarray(dists, np.float64)
    sg = rng.choice([-1.0, 1.0], len(dists)) if side is None else side
    return np.column_stack([rng.uniform(-1.5, 1.5, (len(dists), 2)), 4.0 + sg * dists * C4])


def _clutter(m, rng):
    """at least 0.5 (4-vector distance) from the plane z = 4"""
    return np.column_stack([rng.uniform(-1.5, 1.5, (m, 2)), rng.choice([-1.0, 1.0], m) * rng.uniform(2.2, 3.5, m) + 4.0])


def _case(P, S, pose7=None, **want):
    return dict(P=np.ascontiguousarray(_f32(P)), S=np.ascontiguousarray(S, np.int32).reshape(-1, 3), pose7=POSE_BASE.copy() if pose7 is None else
                np.asarray(pose7, np.float64), want=want)


def _plane_scene(n, seed, iters, frac=0.75):
    """a scene of n points, the samples drawn among its plane points so that most hypotheses pass the gate"""
    n_plane = int(frac * n)
    P, _ = scene(n_plane, n - n_plane, seed)
    near = np.flatnonzero(np.abs(P[:, 2] - 4.0 + (0.02 * P[:, 0] - 0.01 * P[:, 1])) < 0.02)
    rng = np.random.RandomState(seed + 100)
    S = np.sort(np.array([rng.choice(near, 3, replace=False) for _ in range(iters)]), axis=1)
    return P, S


# ------------------------------------------------------------------------------------------------------------ the builders
def _gate_twins():
    """Hypotheses through (0,0,4), (1,0,4+t), (0,1,4+s): normal (-t, -s, 1), gate value sqrt(t^2 + s^2) / |(n, d)|.  t ~ 0.36 puts the
    value just under sinTh; s ~ 0.001 is then stepped one float at a time, which moves the value by ~4e-10, a twentieth of a float ulp
    of sinTh (7.5e-9).  The first step that flips the decision gives the twins: one accepted, one rejected, so close that they pin
    sinTh to the bit.  The steps around them (16 of the 4000) are hypotheses that the gate decides differently in float than in double."""
    def hyp(zt, zs):
        P32 = np.array([[0.0, 0.0, 4.0], [1.0, 0.0, zt], [0.0, 1.0, zs]], F32)
        return plane_of(P32, (0, 1, 2))

    lo, hi = F32(4.30), F32(4.45)                                   # bisect zt = 4 + t (at s = 0.001) down to adjacent floats
    while _step(lo) != hi:
        mid = F32((float(lo) + float(hi)) / 2)
        pl = hyp(mid, F32(4.001))
        lo, hi = (lo, mid) if gate_value(pl[0], pl[1]) > float(SIN_TH) else (mid, hi)
    zt = float(_step(lo, up=False))                                 # one float inside, so that a smaller s has room to cross
    zs, rows = F32(4.0005), []
    for _ in range(4000):
        pl = hyp(zt, zs)
        g, gf = gate_value(pl[0], pl[1]), gate_value_float(pl[0], pl[1])
        rows.append((float(zs), g, g > float(SIN_TH), bool(gf > SIN_TH)))
        zs = _step(zs)
    flips = [k for k in range(1, len(rows)) if rows[k][2] != rows[k - 1][2]]
    assert flips, "the scan never crossed the gate"
    k = flips[0]
    acc, rej = (rows[k - 1], rows[k]) if rows[k][2] else (rows[k], rows[k - 1])
    odd = [row for row in rows if row[2] != row[3]]
    return zt, acc, rej, odd


def build_cases():
    """name -> case; every assert here is on the restatement alone"""
    T = {}
    rng = np.random.RandomState(20240)

    # ---- sizes
    for n in (31, 255, 256, 257):
        P, S = _plane_scene(n, 40 + n, 12)
        T["n%d" % n] = _case(P, S, launched=n >= 32, kth={31: 20, 255: 51, 256: 51, 257: 51}[n], found=n >= 100)
    # a uniform band of points around the winner gives ~1.4 kth inliers, 28 < 32 for kth = 20: the plane points of these are staged
    for n in (100, 104, 105):
        P = np.vstack([TRI, _staged(rng.uniform(0.0020, 0.0027, 60), rng), _clutter(n - 63, rng)])
        S = np.vstack([[[0, 1, 2]], [np.append(np.sort(rng.choice(63, 2, replace=False)), rng.randint(63, n)) for _ in range(7)]])   # 2 staged + 1 clutter
        T["n%d" % n] = _case(P, S, launched=True, kth={100: 20, 104: 20, 105: 21}[n], found=True, n_in=63)
    # n = 32: three points on the plane, 29 between 0.9 and 1.0 x 0.01 from it: the 21st distance x 1.4 covers all 32
    P = np.vstack([TRI, _staged(rng.uniform(0.009, 0.010, 29), rng)])
    T["n32"] = _case(P, [[0, 1, 2]], launched=True, kth=20, found=True, n_in=32, best=0)
    P, S = _plane_scene(12288, 77, 8, frac=0.6)
    T["n12288"] = _case(P, S, launched=True, kth=2457, found=True)

    # ---- iterations
    P, S = _plane_scene(120, 5, 1)
    T["one_iteration"] = _case(P, S, accepted=1, best=0, found=True)
    P, S = _plane_scene(150, 6, 3)
    wall = np.column_stack([rng.uniform(-1, 1, 20), np.full(20, 1.75), rng.uniform(3, 5, 20)])      # normal along y: fails the gate
    P = np.vstack([P, wall])
    S = np.vstack([[150, 151, 152], [153, 155, 160], [150, 160, 169], S])
    T["first_skipped"] = _case(P, S, skipped=[0, 1, 2], best_min=3, found=True)
    cloud = rng.uniform(-1, 1, (200, 3)) * [2, 2, 0.02] @ np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0.0]]) + [0, 0, 4]
    T["all_skipped"] = _case(cloud, samples(200, 20, 3), accepted=0, best=-1, n_in=200, found=True)

    # ---- triples without a plane
    P, S = _plane_scene(140, 8, 4)
    P = np.vstack([P, [[0.0, 0.0, 4.0], [0.5, 0.25, 4.0], [1.0, 0.5, 4.0]]])                            # exactly collinear in float
    S = np.vstack([[140, 141, 142], [S[0, 0], S[0, 0], S[0, 2]], [7, 7, 7], S])
    T["degenerate_triples"] = _case(P, S, skipped=[0, 1, 2], found=True)

    # ---- the orientation gate
    zt, acc, rej, odd = _gate_twins()
    P, S = _plane_scene(130, 9, 3)
    extra = [[0.0, 0.0, 4.0], [1.0, 0.0, zt], [0.0, 1.0, acc[0]], [0.0, 1.0, rej[0]]] + [[0.0, 1.0, row[0]] for row in odd[:2]]
    P = np.vstack([P, extra])
    S = np.vstack([[130, 131, 132], [130, 131, 133]] + [[130, 131, 134 + k] for k in range(len(odd[:2]))] + [S])
    T["gate_twins"] = _case(P, S, gate=[True, False] + [row[2] is False for row in odd[:2]], n_odd=len(odd[:2]), found=True)

    # ---- the winner among equal scores
    P, S = _plane_scene(160, 10, 10)
    r = restate(P, POSE_BASE, S, want_pose=False)
    w = S[r["best"]].copy()
    S = np.vstack([np.delete(S, r["best"], 0)[:9], [[0, 0, 0]]])
    S[[3, 7]] = w
    S[8] = w[[2, 0, 1]]
    S[9] = w[[1, 0, 2]]
    T["winner_ties"] = _case(P, S, best=3, tied=[3, 7], found=True)

    # ---- the radix select
    # 40 copies each of three points at 0.0099, 0.0104, 0.0109 from the plane: rank 40 of 200 lies inside the first run.  Their
    # coordinates are multiples of 2^-10, so that 40-fold sums are exact even in float (the C restatement accumulates the origin in float,
    # and equal addends round the same way every time)
    trio = np.array([[-1.25, 1.0, 4.0 + 42 / 1024], [1.25, 0.25, 4.0 - 44 / 1024], [-0.25, -1.5, 4.0 + 46 / 1024]])
    P = np.vstack([TRI, np.repeat(trio, 40, axis=0), _clutter(77, rng)])
    P[3:] = P[3:][rng.permutation(197)]
    T["radix_equal_keys"] = _case(P, [[0, 1, 2]], best=0, n_in=123, run=40, found=True)
    # a thin slab: every distance but the three samples' in [1/8, 1/8 (1 + 2^-7)): the first two byte passes see one bin
    slab = _staged(rng.uniform(0.125 * 1.0002, 0.125 * (1 + 2.0 ** -7) * 0.9998, 237), rng, side=np.ones(237))
    T["radix_thin_slab"] = _case(np.vstack([TRI, slab]), [[0, 1, 2]], best=0, n_in=240, top16=0x3E00, found=True)
    # 30 > kth = 20 points exactly on the plane: score 0, threshold 0, `0 < 0` is false: no inlier at all
    flat = np.column_stack([rng.randint(-12, 13, (27, 2)) / 8.0, np.full(27, 4.0)])
    T["score_zero"] = _case(np.vstack([TRI, flat, _staged(rng.uniform(0.002, 0.01, 30), rng)]), [[0, 1, 2]], best=0, score_bits=0, n_in=0, found=False)

    # ---- the inlier threshold: two points one float on either side of it
    # a distance near the threshold moves by ~1.2e-7 per float step of z (the sum a x + b y + c z + d is held in floats near 1), so the
    # threshold must be above 1.2e-2 for a point to come within 1e-5 of it: a thick band, threshold ~0.04
    P = np.vstack([TRI, _staged(rng.uniform(0.001, 0.12, 80), rng), _clutter(22, rng)])
    S = np.vstack([[[0, 1, 2]], [np.append(np.sort(rng.choice(83, 2, replace=False)), rng.randint(83, 105)) for _ in range(5)]])
    r = restate(P, POSE_BASE, S, want_pose=False)
    spare = [i for i in np.flatnonzero(r["dist"] > 10 * r["threshold"]) if i not in S][:2]
    pl, thr = tuple(r["planes"][r["best"]]), r["threshold"]
    P = _f32(P)
    for which, i in enumerate(spare):
        P[i, :2] = [[0.4, -0.3], [-0.6, 0.5]][which]
        inside = lambda z: plane_dists(np.array([[P[i, 0], P[i, 1], z]], F32), pl)[0] < thr
        z0 = -(float(pl[0]) * P[i, 0] + float(pl[1]) * P[i, 1] + float(pl[3])) / float(pl[2])
        lo, hi = F32(z0), F32(z0 + 0.5)                   # bisect the height above the plane at which the point stops being an inlier
        assert inside(lo) and not inside(hi)
        while _step(lo) != hi:
            mid = F32((float(lo) + float(hi)) / 2)
            lo, hi = (mid, hi) if inside(mid) else (lo, mid)
        P[i, 2] = float(lo if which == 0 else hi)
    T["threshold_edge"] = _case(P, S, best=r["best"], edge=(int(spare[0]), int(spare[1])), found=True)

    # ---- the inlier count: 32 is a plane, 31 is none
    d = np.concatenate([rng.uniform(0.0005, 0.0035, 17), [0.004], np.linspace(0.0042, 0.0054, 11)])       # sorted: rank 20 is 0.004
    staged = _staged(d, rng)
    for name, move in (("inliers32", 1.0), ("inliers31", 1.5)):
        Q = staged.copy()
        Q[-1, 2] = 4.0 + (Q[-1, 2] - 4.0) * move                                                       # 0.0054 -> 0.0081 > 1.4 x 0.004
        T[name] = _case(np.vstack([TRI, Q, _clutter(28, rng)]), [[0, 1, 2]], best=0, n_in=32 if move == 1.0 else 31, found=move == 1.0,
                        clutter_from=32)

    # ---- the pose
    P, S = _plane_scene(180, 12, 6)
    # Oc = -R t: at z = +9 and z = -9; the normal is turned AWAY from Oc - origin
    T["camera_above"] = _case(P, S, pose7=[0.3, -0.2, -9.0, 0, 0, 0, 1], found=True, nz_sign=-1)
    T["camera_below"] = _case(P, S, pose7=[0.3, -0.2, 9.0, 0, 0, 0, 1], found=True, nz_sign=1)
    q = np.array([0.18, -0.31, 0.42, 0.83])
    T["pose_rotated"] = _case(P, S, pose7=np.concatenate([[0.4, 1.1, -0.7], q / np.linalg.norm(q)]), found=True)

    # ---- ordinary scenes of tests/test_plane.py (n_plane, n_clutter, seed, iterations; samples seeded seed + 1)
    for n_plane, n_clutter, seed, iters in ORDINARY:
        P, _ = scene(n_plane, n_clutter, seed)
        T["scene_%d_%d_%d" % (n_plane, n_clutter, seed)] = _case(P, samples(len(P), iters, seed + 1), found=n_plane != 40)   # (40, 10): 27 inliers
    for name, c in T.items():
        c["name"] = name
        check_case(name, c)
    return T


# (300, 120, 4, 250) is one that tests/test_plane.py holds to 5e-2 only: a point lies 2.7e-5 (relative) from the inlier threshold; in
# (1500, 900, 7, 250) a point's distance EQUALS the threshold, and `<` leaves it out
ORDINARY = [(300, 120, 1, 250), (300, 120, 4, 250), (40, 10, 6, 60), (1500, 900, 7, 250)]
FLOAT_SENSITIVE = "scene_300_120_4"


def check_case(name, c):
    """the case is what its name says, by the restatement"""
    r = restate(c["P"], c["pose7"], c["S"])
    c["r"] = r
    w = c["want"]
    n = len(c["P"])
    assert np.array_equal(c["P"], _f32(c["P"])), name                     # float-representable: the float cast in the kernel is exact
    assert r["kth"] == w.get("kth", r["kth"]) and r["launched"] == w.get("launched", True), (name, r["kth"])
    assert r["found"] == w["found"], (name, r["n_in"])
    for key in ("best", "n_in", "accepted"):
        assert key not in w or r[key] == w[key], (name, key, r[key])
    assert "best_min" not in w or r["best"] >= w["best_min"], (name, r["best"])
    for it in w.get("skipped", []):
        assert np.isinf(r["scores"][it]), (name, it)
    finite = np.isfinite(r["scores"])
    assert int(finite.sum()) == r["accepted"]
    if r["best"] >= 0:
        # rank kth is told from its neighbours: the sorted distances of the winner differ at kth - 1, kth, kth + 1, unless the case is
        # about equal keys
        d = np.sort(r["dist"])
        k = r["kth"]
        c["rank_sensitive"] = bool(d[k - 1] < d[k] < d[k + 1])
        assert c["rank_sensitive"] or name in ("radix_equal_keys", "score_zero"), name
    if name == "n12288":
        assert n == N_MAX and r["accepted"] >= 4
    if name in ("n255", "n256", "n257"):
        assert r["accepted"] >= 4 and 0 < r["n_in"] < n
    if name == "all_skipped":
        assert r["inlier"].all() and r["best_score"] == BEST_INIT
    if name == "gate_twins":
        k = 2 + w["n_odd"]
        assert [bool(np.isfinite(s)) for s in r["scores"][:k]] == w["gate"], (name, r["scores"][:k])
        g = [gate_value(*plane_of(c["P"].astype(F32), c["S"][it])[:2]) for it in range(k)]
        assert g[0] <= float(SIN_TH) < g[1] and g[1] - g[0] < 1e-9 and max(abs(x - float(SIN_TH)) for x in g) < 1e-6, g     # under one float ulp of sinTh apart
        # the two further hypotheses are decided the other way by a float gate
        assert w["n_odd"] >= 1
        for it in range(2, k):
            pl = plane_of(c["P"].astype(F32), c["S"][it])
            assert (gate_value(pl[0], pl[1]) > float(SIN_TH)) != bool(gate_value_float(pl[0], pl[1]) > SIN_TH)
    if name == "winner_ties":
        s = bits(r["scores"])
        assert s[3] == s[7] == bits(r["best_score"])[0] and all(r["scores"][it] > r["best_score"] for it in range(10) if it not in (3, 7, 8, 9))
        assert r["scores"][8] >= r["best_score"] and r["scores"][9] >= r["best_score"]       # the permutations do not beat it
    if name == "radix_equal_keys":
        d = np.sort(r["dist"])
        k = r["kth"]
        assert k == 40 and d[k - 1] == d[k] == d[k + 1] and (d == d[k]).sum() == w["run"]   # rank kth inside a run of 40 equal keys
        assert d[3] == d[k] and d[42] == d[k] and d[43] > d[k]                                 # the run is ranks 3 .. 42
        _, counts = np.unique(c["P"], axis=0, return_counts=True)
        assert np.sort(counts)[-3:].tolist() == [40, 40, 40] and 120 >= 0.6 * n
    if name == "radix_thin_slab":
        key = bits(r["dist"])
        assert ((key >> 16) == w["top16"]).sum() == n - 3 and (key[:3] >> 16 != w["top16"]).all()
        assert len(np.unique(key[3:] >> 8)) > 30                                              # and the third pass sees many bins
    if name == "score_zero":
        assert bits(r["best_score"])[0] == 0 and (r["dist"] == 0).sum() == 30 > r["kth"] and r["threshold"] == 0
    if name == "threshold_edge":
        i, j = w["edge"]
        thr = r["threshold"]
        assert r["inlier"][i] == 1 and r["inlier"][j] == 0
        assert 0 < (thr - r["dist"][i]) / thr < 1e-5 and 0 <= (r["dist"][j] - thr) / thr < 1e-5, (r["dist"][i], r["dist"][j], thr)
        assert margins(r)[2] < 1e-5
    if name in ("inliers32", "inliers31"):
        assert (r["dist"][w["clutter_from"]:] >= 0.5).all() and r["inlier"][w["clutter_from"]:].sum() == 0
    if "nz_sign" in w:
        assert np.sign(r["normal"][2]) == w["nz_sign"], (name, r["normal"])
    if name == "pose_rotated":
        assert abs(np.linalg.norm(c["pose7"][3:]) - 1) < 1e-15 and abs(c["pose7"][6]) < 0.9
    if name == FLOAT_SENSITIVE:
        acc, gap, edge = margins(r)
        assert acc and not (gap > 1e-3 and edge > 1e-3), (gap, edge)      # tests/test_plane.py leaves it out of its tight comparison
    if name == "scene_1500_900_7":
        assert (r["dist"] == r["threshold"]).sum() == 1 and margins(r)[2] == 0
    if r["found"]:
        assert r["eig"][1] > 50 * max(r["eig"][0], 0.0), (name, r["eig"])  # the normal is well determined: eigenvalue ratio >= 50


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


# Which named case tells a subtly wrong kernel from the right one (build_cases() asserts the property each relies on):
SENTINELS = {
    "rank kth - 1 or kth + 1": "every case with c['rank_sensitive'] (the sorted distances differ at kth - 1, kth, kth + 1): the score's bits",
    "<= for < in the threshold": "score_zero (30 points at distance 0 become inliers: found), threshold_edge (dist < thr by one float)",
    "<= for < in the argmin": "winner_ties (best would be 7, or 8 / 9 if a permutation ties too)",
    "the gate in float": "gate_twins, hypotheses 2 and 3 (decided the other way by sqrtf(a a + b b) > sinTh)",
    "n_inliers < 32 off by one": "inliers32 / inliers31",
}
