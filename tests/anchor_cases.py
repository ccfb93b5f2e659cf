"""Anchors restated in numpy: the two stages as include/alvaar_hip.h defines them (A1 - A3: alva_anchor_attach; U0 - U5:
alva_anchor_update) with the same operation order, the butterfly sums and the 12-sweep Jacobi, and the host list
alvaar_amd/csrc/slam/anchors.hpp with the rules of alva_system_create_anchors / alva_system_update_anchors around it (class Anchors).

Every float64 operation below is one IEEE operation in the order the header writes, so where the device follows the header the doubles
agree bit for bit; the tests still allow the project's bars (1e-9 relative for the doubles, 1e-6 for the float poses).

update() reports per anchor how far the case is from each decision a last bit could turn:
  trim_margin   the smallest |r_j - T| / T over the supports, T = max(3.7065 med, 1e-9 rho): keep iff r_j <= T
  gap_margin    |g - 1e-4| / 1e-4 with g = (l1 - l2) / sqrt(Spp Sqq), the smallest over the fits that ran; 1 when Spp Sqq = 0
  m_from_4, kept_from_4   integers: |m - 4|, |kept - 4| (0: exactly at the bound, which integers decide exactly)"""
from __future__ import annotations

import functools
import math

import numpy as np

MARGIN_MIN = 1e-7            # the project's bar for "far from a decision"
N_CAP, K_MIN, K_MAX, STRIDE = 16384, 8, 64, 64
TRIM_FACTOR, TRIM_FLOOR, GAP = 3.7065, 1e-9, 1e-4


# ------------------------------------------------------------------------------------------------ stage 1
def attach(P, pos3, K):
    """A1 - A3 -> (index [a,K] int32, dist2 [a,K] float64, count [a] int32)"""
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    pos = np.ascontiguousarray(pos3, np.float64).reshape(-1, 3)
    n, a = len(P), len(pos)
    index, dist2, count = np.full((a, K), -1, np.int32), np.zeros((a, K)), np.zeros(a, np.int32)
    for k in range(a):
        dx, dy, dz = P[:, 0] - pos[k, 0], P[:, 1] - pos[k, 1], P[:, 2] - pos[k, 2]
        d = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((np.arange(n), d.view(np.uint64)))[:min(K, n)]   # the total order (bits(d), i)
        count[k] = len(order)
        index[k, :len(order)], dist2[k, :len(order)] = order, d[order]
    return index, dist2, count


# ------------------------------------------------------------------------------------------------ stage 2
def wave_sum(terms):
    """64 lane terms in the __shfl_xor butterfly order, masks 1 2 4 .. 32: a balanced tree over adjacent pairs"""
    v = np.asarray(terms, np.float64)
    assert v.shape == (64,)
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return float(v[0])


def _dot(r, v):
    return (r[0] * v[0] + r[1] * v[1]) + r[2] * v[2]


def jacobi4(N):
    """cyclic Jacobi, exactly 12 sweeps -> (diagonal [4], V [4][4]: column k belongs to diagonal entry k)"""
    M = [[float(N[a][b]) for b in range(4)] for a in range(4)]
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    for _ in range(12):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = M[p][q]
                if abs(apq) < 1e-300:
                    continue
                th = (M[q][q] - M[p][p]) / (2 * apq)
                tt = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1))
                cs = 1 / math.sqrt(tt * tt + 1)
                sn = tt * cs
                M[p][p] -= tt * apq
                M[q][q] += tt * apq
                M[p][q] = M[q][p] = 0.0
                for k in range(4):
                    if k in (p, q):
                        continue
                    kp, kq = M[k][p], M[k][q]
                    M[k][p] = M[p][k] = cs * kp - sn * kq
                    M[k][q] = M[q][k] = sn * kp + cs * kq
                for k in range(4):
                    vp, vq = V[k][p], V[k][q]
                    V[k][p] = cs * vp - sn * vq
                    V[k][q] = sn * vp + cs * vq
    return [M[k][k] for k in range(4)], V


def rigid_fit(inside, p, q):
    """U1 - U3 over the lanes `inside` [64] bool; p, q [64,3] -> dict(det, R [3][3], t [3], rho, gap_margin)"""
    c = int(inside.sum())
    z = np.zeros(64)
    cp = [wave_sum(np.where(inside, p[:, k], z)) / float(c) for k in range(3)]
    cq = [wave_sum(np.where(inside, q[:, k], z)) / float(c) for k in range(3)]
    pc = np.stack([p[:, k] - cp[k] for k in range(3)], 1)
    qc = np.stack([q[:, k] - cq[k] for k in range(3)], 1)
    Spp = wave_sum(np.where(inside, (pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2], z))
    Sqq = wave_sum(np.where(inside, (qc[:, 0] * qc[:, 0] + qc[:, 1] * qc[:, 1]) + qc[:, 2] * qc[:, 2], z))
    out = dict(det=False, R=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], t=[cq[k] - cp[k] for k in range(3)],
               rho=math.sqrt(Spp / float(c)), gap_margin=np.inf)
    if c < 4:
        return out
    S = [[wave_sum(np.where(inside, pc[:, a] * qc[:, b], z)) for b in range(3)] for a in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    N[0][1] = N[1][0] = S[1][2] - S[2][1]
    N[0][2] = N[2][0] = S[2][0] - S[0][2]
    N[0][3] = N[3][0] = S[0][1] - S[1][0]
    N[1][2] = N[2][1] = S[0][1] + S[1][0]
    N[1][3] = N[3][1] = S[2][0] + S[0][2]
    N[2][3] = N[3][2] = S[1][2] + S[2][1]
    lam, V = jacobi4(N)
    i1 = 0
    for k in range(1, 4):
        if lam[k] > lam[i1]:
            i1 = k
    l2 = max(lam[k] for k in range(4) if k != i1)
    scale = math.sqrt(Spp * Sqq)
    out["gap_margin"] = abs((lam[i1] - l2) / scale - GAP) / GAP if scale > 0 else 1.0
    if lam[i1] - l2 <= GAP * scale:
        return out
    e = [V[r][i1] for r in range(4)]
    nq = math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
    w, x, y, zz = e[0] / nq, e[1] / nq, e[2] / nq, e[3] / nq
    R = [[1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y)],
         [2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x)],
         [2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)]]
    out.update(det=True, R=R, t=[cq[k] - _dot(R[k], cp) for k in range(3)])
    return out


def update_one(m, ref, cur, pose_ref):
    """U0 - U5 for one anchor: ref, cur [64,3] (rows >= m are not looked at), pose_ref [16] float32"""
    pose_ref = np.asarray(pose_ref, np.float32)
    res = dict(code=2, m=int(m), kept=int(m), R=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], t=[0.0, 0.0, 0.0],
               trim_margin=np.inf, gap_margin=np.inf, m_from_4=abs(int(m) - 4), kept_from_4=abs(int(m) - 4))
    if m == 0:
        res["pose"] = pose_ref.copy()
        return _finish(res)
    inside = np.arange(64) < m
    p, q = np.zeros((64, 3)), np.zeros((64, 3))
    p[:m], q[:m] = ref[:m], cur[:m]
    f = rigid_fit(inside, p, q)
    res.update(code=0 if f["det"] else 1, R=f["R"], t=f["t"], gap_margin=f["gap_margin"])
    if f["det"]:
        R, t = f["R"], f["t"]
        e = [q[:, k] - (((R[k][0] * p[:, 0] + R[k][1] * p[:, 1]) + R[k][2] * p[:, 2]) + t[k]) for k in range(3)]
        r = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        order = np.lexsort((np.arange(m), r[:m]))   # (r, lane)
        med = float(r[order[m // 2]])
        keep = inside & ((r <= TRIM_FACTOR * med) | (r <= TRIM_FLOOR * f["rho"]))
        T = max(TRIM_FACTOR * med, TRIM_FLOOR * f["rho"])
        res["trim_margin"] = float(np.min(np.abs(r[:m] - T)) / T) if T > 0 else 0.0
        kept = int(keep.sum())
        res.update(kept=kept, kept_from_4=abs(kept - 4), med=med)
        if 4 <= kept < m:
            g = rigid_fit(keep, p, q)
            res["gap_margin"] = min(res["gap_margin"], g["gap_margin"])
            res["refit_det"] = g["det"]
            if g["det"]:
                res.update(R=g["R"], t=g["t"])
    R, t = res["R"], res["t"]
    pr = pose_ref.astype(np.float64)
    pose = np.zeros(16, np.float32)
    for col in range(4):
        v = pr[4 * col:4 * col + 3]
        for row in range(3):
            rv = _dot(R[row], v)
            pose[4 * col + row] = np.float32(rv + t[row] if col == 3 else rv)
    pose[15] = 1
    res["pose"] = pose
    return _finish(res)


def _finish(res):
    res["rt12"] = np.array([v for row in res["R"] for v in row] + list(res["t"]), np.float64)
    res["info"] = np.array([res["code"], res["m"], res["kept"], 0, 0, 0, 0, 0], np.int32)
    return res


def update(count, ref, cur, pose_ref):
    """alva_anchor_update -> dict(pose [a,16] float32, rt12 [a,12], info [a,8] int32, per = the per-anchor dicts)"""
    count = np.asarray(count, np.int32).reshape(-1)
    ref, cur = np.asarray(ref, np.float64).reshape(-1, 64, 3), np.asarray(cur, np.float64).reshape(-1, 64, 3)
    pose_ref = np.asarray(pose_ref, np.float32).reshape(-1, 16)
    per = [update_one(int(count[a]), ref[a], cur[a], pose_ref[a]) for a in range(len(count))]
    return dict(pose=np.stack([r["pose"] for r in per]), rt12=np.stack([r["rt12"] for r in per]), info=np.stack([r["info"] for r in per]),
                per=per)


def margins_ok(r, exact=()):
    """every margin of one anchor's result >= MARGIN_MIN, except those named in `exact`, which must be 0"""
    ok = True
    for key in ("trim_margin", "gap_margin"):
        ok = ok and (r[key] == 0 if key in exact else r[key] >= MARGIN_MIN)
    for key in ("m_from_4", "kept_from_4"):
        if key in exact:
            ok = ok and r[key] == 0
    return ok


def margins_text(r):
    return "trim %.3g gap %.3g |m-4| %d |kept-4| %d" % (r["trim_margin"], r["gap_margin"], r["m_from_4"], r["kept_from_4"])


# ------------------------------------------------------------------------------------------------ the scenes
def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def pose_of(R=None, t=(0.0, 0.0, 0.0)):
    """a pose16 in findPlane's layout: out[4 c + r] = R[r][c], out[12..14] = t"""
    R = np.eye(3) if R is None else np.asarray(R)
    out = np.zeros(16, np.float32)
    for c in range(3):
        out[4 * c:4 * c + 3] = R[:, c]
    out[12:15] = t
    out[15] = 1
    return out


POSE_REF = pose_of(rot((0.3, -0.5, 0.8), 40.0), (0.25, -0.5, 1.5))
PLANTED_R, PLANTED_T = rot((0.2, 1.0, -0.4), 30.0), np.array([0.3, -0.2, 0.5])


def _pad(x):
    out = np.zeros((64, 3))
    out[:len(x)] = x
    return out


def _case(ref, cur, code, kept=None, pose_ref=POSE_REF, exact=(), R=None, t=None):
    m = len(ref)
    return dict(count=m, ref=_pad(ref), cur=_pad(cur), pose_ref=np.asarray(pose_ref, np.float32), code=code, kept=m if kept is None else kept,
                exact=tuple(exact), R=R, t=t)


def _moved(P, R, t):
    return P @ np.asarray(R).T + np.asarray(t)


@functools.lru_cache(maxsize=None)
def update_cases():
    """name -> dict(count, ref [64,3], cur [64,3], pose_ref [16], code, kept, exact = the margins that are 0 by construction, R, t = the
    planted motion where the case recovers one)"""
    rng = np.random.default_rng(20261019)
    P32 = rng.standard_normal((32, 3))
    c = {}
    c["planted32"] = _case(P32, _moved(P32, PLANTED_R, PLANTED_T), 0, R=PLANTED_R, t=PLANTED_T)
    # four of the 32 displaced by the support's diameter: the trim drops exactly them, and the refit recovers the motion
    diam = float(np.max(np.linalg.norm(P32[:, None] - P32[None], axis=2)))
    out = _moved(P32, PLANTED_R, PLANTED_T)
    for j, d in zip((3, 11, 20, 29), ((1, 0, 0), (0, -1, 0), (0, 0, 1), (-0.6, 0.8, 0))):
        out[j] += diam * np.array(d, np.float64)
    c["outliers4"] = _case(P32, out, 0, kept=28, R=PLANTED_R, t=PLANTED_T)
    c["identity"] = _case(P32, P32.copy(), 0, R=np.eye(3), t=np.zeros(3))
    c["translation"] = _case(P32, P32 + np.array([0.5, -0.25, 0.125]), 0, R=np.eye(3), t=np.array([0.5, -0.25, 0.125]))
    for deg in (1, 90, 180):
        R = rot((0.5, -0.3, 0.7), float(deg))
        c["rot%d" % deg] = _case(P32, _moved(P32, R, (0.1, 0.2, -0.3)), 0, R=R, t=np.array([0.1, 0.2, -0.3]))
    # sizes: 0 (U0), 1 and 3 (U2), 4 (the first size with a rotation), 63, 64
    P64 = rng.standard_normal((64, 3))
    Q64 = _moved(P64, PLANTED_R, PLANTED_T)
    c["m0"] = _case(P64[:0], Q64[:0], 2)
    c["m1"] = _case(P64[:1], Q64[:1], 1)
    c["m3"] = _case(P64[:3], Q64[:3], 1)
    c["m4"] = _case(P64[:4], Q64[:4], 0, exact=("m_from_4", "kept_from_4"), R=PLANTED_R, t=PLANTED_T)
    c["m63"] = _case(P64[:63], Q64[:63], 0, R=PLANTED_R, t=PLANTED_T)
    c["m64"] = _case(P64, Q64, 0, R=PLANTED_R, t=PLANTED_T)
    # five supports, two of them pulled apart along the line that joins them (residuals sum to zero and, that way, exert no torque: the
    # fit leaves them their whole displacement), the other three moved by a thousandth: the trim leaves three, fewer than a rotation
    # needs, and the first fit stands.  (With four supports no trim can leave three: the residuals sum to zero, so the largest is at most
    # three times the median's)
    P5 = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, -1.0, 0.0], [0.5, 0.5, -1.0]])
    R5 = rot((0, 0, 1), 10.0)
    Q5 = _moved(P5, R5, (0.05, 0.0, -0.02))
    u = R5 @ (P5[3] - P5[4])
    u /= np.linalg.norm(u)
    Q5[3] += 0.8 * u
    Q5[4] -= 0.8 * u
    Q5[:3] += np.array([[0.001, -0.002, 0.0015], [-0.002, 0.001, 0.0005], [0.0015, 0.0005, -0.001]])
    c["trim_to_3"] = _case(P5, Q5, 0, kept=3)
    # supports on one line: the rotation about the line is free
    s = np.linspace(-1.0, 1.0, 16)
    line = np.stack([0.5 + s * 0.6, -0.25 + s * 0.48, 1.0 + s * 0.64], 1)
    c["collinear"] = _case(line, line + np.array([0.125, 0.25, -0.5]), 1)
    # nearly on a line, on both sides of the gap test: g = (l1 - l2) / sqrt(Spp Sqq) is about 4 (eps / L)^2 for a perpendicular spread eps
    wob = rng.standard_normal((16, 3))
    wob -= np.outer(wob @ np.array([0.6, 0.48, 0.64]), np.array([0.6, 0.48, 0.64]))
    for name, eps, code in (("near_line_under", 0.0022, 1), ("near_line_over", 0.0075, 0)):
        pts = line + eps * wob
        c[name] = _case(pts, _moved(pts, rot((1, 2, 3), 25.0), (0.1, 0.0, -0.1)), code)
    return c


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    case = update_cases()[name]
    return update_one(case["count"], case["ref"], case["cur"], case["pose_ref"])


ATTACH_SIZES = (0, 3, 4, 511, 512, 513, 2049, 16384)   # and K - 1, K, K + 1 for each K


def attach_sizes(K):
    return sorted(set(ATTACH_SIZES + (K - 1, K, K + 1)))


@functools.lru_cache(maxsize=None)
def attach_points(n):
    """n random points about the origin, and three anchor positions among them"""
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal((n, 3)) * 2.0, np.array([[0.1, -0.2, 0.3], [2.0, 2.0, -1.0], [-30.0, 5.0, 0.0]])


def lattice():
    """an 11 x 11 x 11 integer lattice about an anchor at its centre point: many exactly equal distances (6 at d = 1, 12 at 2, 8 at 3 ..)"""
    g = np.arange(-5.0, 6.0)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(P), np.zeros((1, 3))


def duplicates():
    """40 distinct points, each present three times (indices i, i + 40, i + 80)"""
    rng = np.random.default_rng(77)
    P = rng.standard_normal((40, 3))
    return np.ascontiguousarray(np.concatenate([P, P, P])), np.array([[0.2, 0.1, -0.1]])


# ------------------------------------------------------------------------------------------------ the host list, restated
class Anchors:
    """csrc/slam/anchors.hpp and the rules of alva_system_create_anchors / alva_system_update_anchors around it.  The stages are handed
    in (attach_fn(P, pos3, K) -> (index, dist2, count); update_fn(count, ref, cur, pose_ref) -> (pose, rt12, info)), so the same class
    serves the numpy restatement and the replay through Context.anchor_attach / Context.anchor_update.  A map is (ids ascending [n],
    P [n,3]): the 3-D points, at most the newest 16384."""
    MAX = 64

    def __init__(self):
        self.list, self.next_id = [], 0

    def create(self, poses16, K, ids, P, attach_fn):
        poses = np.asarray(poses16, np.float32).reshape(-1, 16)
        out_ids, info = np.full(len(poses), -1, np.int32), np.zeros((len(poses), 8), np.int32)
        new = []
        for k, pose in enumerate(poses):
            info[k, 2] = len(ids)
            code = 4 if not np.isfinite(pose).all() else 1 if len(ids) < 4 else 3 if len(self.list) == self.MAX else 0
            info[k, 0] = code
            if code:
                continue
            a = dict(id=self.next_id, age=0, K=int(K), count0=0, sup=[], ref=np.zeros((0, 3)), ref_pose=pose.copy(), last=pose.copy())
            self.next_id += 1
            self.list.append(a)
            new.append((k, a))
            out_ids[k] = a["id"]
        if new:
            self._attach([a for _, a in new], np.stack([a["ref_pose"] for _, a in new]), ids, P, attach_fn)
            for k, a in new:
                info[k, 1] = len(a["sup"])
        return out_ids, info

    def _attach(self, anchors, poses, ids, P, attach_fn):
        index, _, count = attach_fn(P, poses[:, 12:15].astype(np.float64), 64)   # the first K of the 64 nearest are the K nearest
        for a, pose, idx, cnt in zip(anchors, poses, index, count):
            m = min(int(cnt), a["K"])
            a.update(ref_pose=pose.copy(), last=pose.copy(), count0=m, sup=[int(ids[i]) for i in idx[:m]], ref=P[idx[:m]].copy())

    def gather(self, ids, P):
        """-> (count [n], ref [n,64,3], cur [n,64,3], pose_ref [n,16]); supports that are gone leave the list for good"""
        row = {int(i): r for r, i in enumerate(ids)}
        n = len(self.list)
        count, ref, cur = np.zeros(n, np.int32), np.zeros((n, 64, 3)), np.zeros((n, 64, 3))
        for k, a in enumerate(self.list):
            alive = [j for j, s in enumerate(a["sup"]) if s in row]
            a["sup"], a["ref"] = [a["sup"][j] for j in alive], a["ref"][alive]
            count[k] = len(alive)
            ref[k, :len(alive)], cur[k, :len(alive)] = a["ref"], P[[row[s] for s in a["sup"]]]
        return count, ref, cur, np.stack([a["ref_pose"] for a in self.list]).reshape(n, 16)

    def update(self, ids, P, update_fn, attach_fn, on_stage=None):
        """one status-1 alva_system_update_anchors on the map (ids: EVERY 3-D point's id ascending, P their positions) -> (ids, poses, info)"""
        n = len(self.list)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros((0, 16), np.float32), np.zeros((0, 8), np.int32)
        count, ref, cur, pose_ref = self.gather(ids, P)
        pose, rt12, sinfo = update_fn(count, ref, cur, pose_ref)
        if on_stage:
            on_stage(dict(count=count, ref=ref, cur=cur, pose_ref=pose_ref, pose=pose, rt12=rt12, info=sinfo))
        info = np.zeros((n, 8), np.int32)
        again = []
        for k, a in enumerate(self.list):
            a["last"], a["age"] = pose[k].copy(), a["age"] + 1
            info[k] = [sinfo[k, 0], count[k], sinfo[k, 2], 0, a["age"], a["count0"], 0, 0]
            if count[k] < (a["count0"] + 1) // 2:
                again.append(k)
        cand_ids, cand_P = ids[-N_CAP:], P[-N_CAP:]
        if again and len(cand_ids) >= 4:
            for b in range(0, len(again), 16):
                which = again[b:b + 16]
                self._attach([self.list[k] for k in which], np.stack([pose[k] for k in which]), cand_ids, cand_P, attach_fn)
                for k in which:
                    info[k, 3], info[k, 5] = 1, self.list[k]["count0"]
        return np.array([a["id"] for a in self.list], np.int32), pose.copy(), info

    def not_tracking(self):
        """alva_system_update_anchors while the last status was not 1: code 6, the last pose, nothing changes"""
        n = len(self.list)
        info = np.zeros((n, 8), np.int32)
        for k, a in enumerate(self.list):
            info[k] = [6, len(a["sup"]), 0, 0, a["age"], a["count0"], 0, 0]
        poses = np.stack([a["last"] for a in self.list]).reshape(n, 16) if n else np.zeros((0, 16), np.float32)
        return np.array([a["id"] for a in self.list], np.int32), poses, info

    def remove(self, anchor_id):
        before = len(self.list)
        self.list = [a for a in self.list if a["id"] != anchor_id]
        return before - len(self.list)

    def clear(self):
        self.list = []


def oracle_fns():
    """the two stages as the restatement computes them, in the shape class Anchors takes"""
    def update_fn(count, ref, cur, pose_ref):
        r = update(count, ref, cur, pose_ref)
        return r["pose"], r["rt12"], r["info"]
    return attach, update_fn
