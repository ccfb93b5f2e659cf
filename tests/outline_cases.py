"""The plane outline's definition (include/alvaar_hip.h, alva_plane_outlines) restated in numpy and Python integers, line for line, and
the scenes the tests run it on.  The reference has no plane outlines, so this file is what alva_plane_outlines is pinned to
(tests/test_outline_cases.py checks the restatement itself, tests/test_gpu_plane_outlines.py the kernel against it).

The outline is a set function of the plane's points with exact predicates: the projection into the plane's frame is IEEE double in the
written operation order (elementwise numpy does not contract a * b + c into an FMA), the grid coordinates are integers, and the hull is
decided by the sign of integer cross products (Python ints here, int64 on the device: differences stay below 2^23).  So the kernel is
compared with ==, on every output byte, and no case needs a margin."""
from __future__ import annotations

import functools

import numpy as np

import plane_cases as C

N_CAP = 16384
GRID = 1048576.0        # cells per extent
Q_MAX = 1 << 21         # grid coordinates are clamped to [-2^21, 2^21]
MIN_VERTICES, MAX_VERTICES = 8, 1024


def frame(rec):
    """(code, x, z, p, s) of a plane record: 5 no record, 4 a frame that cannot be used, 0 fine"""
    rec = np.asarray(rec, np.float32).astype(np.float64)
    x, z, p = rec[0:3], rec[8:11], rec[12:15]
    s = np.maximum(rec[16], rec[17])   # a NaN extent makes s NaN
    if rec[15] != 1:
        return 5, x, z, p, s
    if not (np.isfinite(s) and s > 0 and np.isfinite(x).all() and np.isfinite(z).all() and np.isfinite(p).all()):
        return 4, x, z, p, s
    return 0, x, z, p, s


def quantise(P, x, z, p, s):
    """the grid points [m, 2] int64 of the points P [m, 3]"""
    inv = GRID / s
    d = np.asarray(P, np.float64).reshape(-1, 3) - p
    u = (d[:, 0] * x[0] + d[:, 1] * x[1]) + d[:, 2] * x[2]
    v = (d[:, 0] * z[0] + d[:, 1] * z[1]) + d[:, 2] * z[2]
    qu = np.clip(np.rint(u * inv), -Q_MAX, Q_MAX).astype(np.int64)
    qv = np.clip(np.rint(v * inv), -Q_MAX, Q_MAX).astype(np.int64)
    return np.column_stack([qu, qv])


def cross(o, a, b) -> int:
    """cross(a - o, b - o) in Python integers"""
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(q):
    """the strictly convex vertices of the hull of the grid points q, counter-clockwise from the lexicographically smallest one: Andrew's
    monotone chain on the distinct points with <= 0 pops.  One point, or all collinear: the one or two end points (no area)"""
    pts = sorted(set((int(a), int(b)) for a, b in np.asarray(q).reshape(-1, 2)))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    out = lower[:-1] + upper[:-1]   # counter-clockwise, and lower[0] is the smallest point already
    k = out.index(min(out))
    return out[k:] + out[:k]


def area2(verts) -> int:
    return sum(verts[i][0] * verts[(i + 1) % len(verts)][1] - verts[(i + 1) % len(verts)][0] * verts[i][1] for i in range(len(verts)))


def oracle(P, labels, planes24, max_vertices=64):
    """Returns a dict: outline [n_planes, max_vertices, 2] float32, q (the same shape, int32), info [n_planes, 8] int32, area [n_planes]
    float64 and found (the return value)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    labels = np.asarray(labels, np.int32).reshape(-1)
    planes24 = np.asarray(planes24, np.float32).reshape(-1, 24)
    n_planes = len(planes24)
    assert len(labels) == len(P) and 1 <= n_planes <= 8 and MIN_VERTICES <= max_vertices <= MAX_VERTICES
    outline = np.zeros((n_planes, max_vertices, 2), np.float32)
    q = np.zeros((n_planes, max_vertices, 2), np.int32)
    info = np.zeros((n_planes, 8), np.int32)
    area = np.zeros(n_planes, np.float64)
    found = 0
    for k in range(n_planes):
        code, x, z, p, s = frame(planes24[k])
        if code:
            info[k, 0] = code
            continue
        mine = P[labels == k]
        if len(mine) < 3:
            info[k] = [1, 0, len(mine), 0, 0, 0, 0, 0]
            continue
        verts = hull(quantise(mine, x, z, p, s))
        if len(verts) < 3:
            info[k] = [2, 0, len(mine), 0, 0, 0, 0, 0]
            continue
        if len(verts) > max_vertices:
            info[k] = [3, 0, len(mine), 0, 0, 0, 0, 0]
            continue
        cell = s / GRID
        a2 = area2(verts)
        assert a2 > 0
        area[k] = ((np.float64(a2) * 0.5) * cell) * cell
        v = np.array(verts, np.int64)
        q[k, :len(verts)] = v
        outline[k, :len(verts)] = (v.astype(np.float64) * cell).astype(np.float32)
        info[k] = [0, len(verts), len(mine), 0, 0, 0, 0, 0]
        found += 1
    return dict(outline=outline, q=q, info=info, area=area, found=found)


# ---------------------------------------------------------------------------------------------------- scenes
def hand_frame(centre, extent_x, extent_z):
    """a plane record made by hand: x = (1, 0, 0), normal (0, 0, -1), z = x cross normal = (0, 1, 0)"""
    rec = np.zeros(24, np.float32)
    rec[0], rec[6], rec[9], rec[15] = 1, -1, 1, 1
    rec[12:15] = centre
    rec[16], rec[17] = extent_x, extent_z
    rec[18] = -centre[2]
    return rec


def detected(name, n_planes=None):
    """(P, labels, planes24) of a scene of plane_cases as its oracle detects it"""
    case, r = C.edge_cases()[name], C.oracle_of(name)
    planes = r["planes"] if n_planes is None else r["planes"][:n_planes]
    return case["P"], r["labels"].copy(), planes.copy()


CIRCLE_N, CIRCLE_R = 600, 1 << 19


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(P, labels, planes, kw): the scenes of tests/test_gpu_plane_outlines.py at the smallest sizes that exercise the kernel's
    edges; tests/test_outline_cases.py asserts on the CPU what each is meant to be.  Callers must not change them"""
    rng = np.random.RandomState(33)
    out = {}

    def add(name, P, labels, planes, **kw):
        out[name] = dict(P=np.ascontiguousarray(P, np.float64).reshape(-1, 3), labels=np.ascontiguousarray(labels, np.int32),
                         planes=np.ascontiguousarray(planes, np.float32).reshape(-1, 24), kw=kw)

    # one noisy plane at the wave and workgroup edges, labelled by the detector's oracle
    for n in (63, 64, 65, 511, 512, 513, 2049):
        add("n%d" % n, *detected("n%d" % n, 1))
    P, labels, planes = detected("n63", 1)
    first = np.nonzero(labels == 0)[0]
    for m in (2, 3):   # too few for a detection: the frame of n63, and m of its points
        lab = np.full(len(P), -1, np.int32)
        lab[first[:m]] = 0
        add("m%d" % m, P, lab, planes)
    P, _, planes = detected("n16384", 1)
    add("n16384", P, np.zeros(len(P), np.int32), planes)   # every point on the one plane
    add("base", *detected("base", 2))
    add("rotated", *detected("rotated", 2))
    add("base_max8", *detected("base_max8"))               # records 2 .. 7 are all zero
    add("exact_plane", *detected("exact_plane", 1))
    # labels: the two planes' indices interleaved (floor, wall, floor, wall, .. then the rest), labels -1 and >= n_planes, an empty plane
    P, labels, planes = detected("base", 2)
    i0, i1, rest = (np.nonzero(labels == v)[0] for v in (0, 1, -1))
    m = min(len(i0), len(i1))
    order = np.concatenate([np.column_stack([i0[:m], i1[:m]]).ravel(), i0[m:], i1[m:], rest])
    add("interleaved", P[order], labels[order], planes)
    lab = labels.copy()
    lab[rest[::2]] = 2        # >= n_planes
    lab[rest[1::4]] = -7
    lab[rest[3::8]] = 1 << 30   # (rest[7::8] stays -1)
    add("foreign_labels", P, lab, planes)
    add("wall_only", P, np.where(labels == 1, 1, -1), planes)   # plane 0 has a record and no point
    # degenerate sets, in a frame made by hand
    origin = C.POSE_BASE[:3]
    line = origin + np.column_stack([0.125 * np.arange(40), np.zeros(40), np.full(40, 4.0)])
    fr = hand_frame(origin + np.array([2.5, 0.0, 4.0]), 5.0, 1.0)
    add("collinear", line, np.zeros(40, np.int32), fr)
    add("identical", np.tile(line[7], (40, 1)), np.zeros(40, np.int32), fr)
    P, labels, planes = detected("n513", 1)
    add("duplicated", np.vstack([P, P]), np.concatenate([labels, labels]), planes)
    # a long march: 600 points on a circle of radius 2^19 cells (s = 2, so a cell is 2^-19 and the radius 1), built in the plane's frame.
    # Neighbours are 5490 cells apart and the sagitta is 28.7 cells, so every point is a strictly convex vertex, and none is strictly
    # inside the octagon through eight of them
    centre = origin + np.array([0.5, -0.25, 4.0])
    ang = 2 * np.pi * (np.arange(CIRCLE_N) + 0.3) / CIRCLE_N
    circle = centre + np.column_stack([np.cos(ang), np.sin(ang), np.zeros(CIRCLE_N)])
    circle = circle[rng.permutation(CIRCLE_N)]
    add("circle", circle, np.zeros(CIRCLE_N, np.int32), hand_frame(centre, 2.0, 1.0), max_vertices=1024)
    add("circle_64", circle, np.zeros(CIRCLE_N, np.int32), hand_frame(centre, 2.0, 1.0), max_vertices=64)
    # frame faults beside a good plane: no other plane of the call is disturbed
    P, labels, planes = detected("base", 2)
    for name, idx, val in (("zero_extents", (16, 17), 0.0), ("nan_centre", (13,), np.nan), ("inf_extent", (17,), np.inf)):
        for k in (0, 1):
            bad = planes.copy()
            bad[k, list(idx)] = val
            add("%s_%d" % (name, k), P, labels, bad)
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """the restatement's result for scenes()[name], computed once per process and shared: callers must not change it"""
    s = scenes()[name]
    return oracle(s["P"], s["labels"], s["planes"], **s["kw"])
