"""The scene mesh stages' definitions (include/alvaar_hip.h: alva_mesh_integrate M1-M5, alva_mesh_extract X1-X7) restated in numpy,
operation for operation, the analytic scenes the tests run them on and the two case tables.  The reference has no scene mesh, so this
file is what the two stages are pinned to (tests/test_mesh_cases.py checks the restatement against topology and analytic surfaces;
tests/test_gpu_mesh.py the kernels against it, bit for bit).

As in tests/depth_cases.py the geometry is float64 / float32 exactly where the definition says so, in its operation order (elementwise
numpy does not contract a * b + c), and every sum of more than two terms is an integer sum, so the GPU is compared with `==`."""
from __future__ import annotations

import functools

import numpy as np

import depth_cases as Dc

F32 = np.float32
W_MAX = 128   # the system call's constant (include/alvaar_system.h)


def hashed(n, seed):
    """n hashed 32-bit values (a fixed integer mix of the index: the same on every machine)"""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    for _ in range(2):
        x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
        x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return (x ^ (x >> np.uint64(16))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- alva_mesh_integrate
def integrate(q, w, origin3, voxel, trunc, T_cw12, calib8, width, height, step, meas, w_max=W_MAX):
    """alva_mesh_integrate.  q int16 / w uint8 [N,N,N] (index [k][j][i]; not modified), meas = (depth float32, conf uint8, code uint8),
    each [gh,gw].  Returns a dict: q, w (the volume after), info [8] int32, and for the tests cat [N,N,N] (0 updated, 1 hidden, 3
    outside, 4 no depth), free [N,N,N] bool, q_m and A [N,N,N] (the measurement and M5's numerator where updated, else 0)."""
    q0 = np.asarray(q, np.int16)
    N = q0.shape[0]
    assert q0.shape == (N, N, N) and np.asarray(w).shape == (N, N, N)
    q0 = q0.reshape(-1).astype(np.int64)
    w0 = np.asarray(w, np.uint8).reshape(-1).astype(np.int64)
    gw, gh = width // step, height // step
    o = np.asarray(origin3, np.float64).reshape(-1)
    voxel, trunc = np.float64(voxel), np.float64(trunc)
    Tm = np.asarray(T_cw12, np.float64).reshape(-1)
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    depth = np.asarray(meas[0], F32).reshape(-1)[:gw * gh]
    conf = np.asarray(meas[1], np.uint8).reshape(-1)[:gw * gh].astype(np.int64)
    code = np.asarray(meas[2], np.uint8).reshape(-1)[:gw * gh]
    idx = np.arange(N * N * N)
    i, j, k = idx % N, (idx // N) % N, idx // (N * N)
    # M1
    x = o[0] + (i.astype(np.float64) + 0.5) * voxel
    y = o[1] + (j.astype(np.float64) + 0.5) * voxel
    z = o[2] + (k.astype(np.float64) + 0.5) * voxel
    P = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
    cat = np.full(N * N * N, 3, np.int64)
    with np.errstate(all="ignore"):
        front = P[2] > 1e-9
        # M2
        up, vp = Dc.project_dist(calib8, P[0], P[1], P[2])
        fu, fv = np.floor(up), np.floor(vp)
        assert fu.dtype == F32
        inimg = front & (F32(0) <= fu) & (fu < F32(gw * step)) & (F32(0) <= fv) & (fv < F32(gh * step))
    c = np.where(inimg, (np.where(inimg, fv, 0).astype(np.int64) // step) * gw + np.where(inimg, fu, 0).astype(np.int64) // step, 0)
    # M3
    cat[inimg] = 4
    with np.errstate(all="ignore"):
        has = inimg & (code[c] == 0) & (depth[c] > F32(0))
    w_m = np.maximum(1, conf[c] >> 3)
    # M4
    with np.errstate(all="ignore"):
        s = depth[c].astype(np.float64) - P[2]
        hidden = has & (s < -trunc)
        tt = s / trunc
        upd = has & ~hidden
        free = upd & (tt >= 1.0)
        q_m = np.where(free, 32767, np.where(upd, np.rint(np.where(upd, tt, 0.0) * 32767.0), 0)).astype(np.int64)
    cat[hidden] = 1
    cat[upd] = 0
    # M5
    A = q0 * w0 + q_m * w_m
    S = w0 + w_m
    qn = (2 * A + S) // (2 * S)   # numpy's // is a floor
    wn = np.minimum(int(w_max), S)
    assert np.all(np.abs(A[upd]) < 2 ** 31)
    q1 = np.where(upd, qn, q0).astype(np.int16).reshape(N, N, N)
    w1 = np.where(upd, wn, w0).astype(np.uint8).reshape(N, N, N)
    info = np.array([upd.sum(), hidden.sum(), free.sum(), (cat == 3).sum(), (cat == 4).sum(), N, 0, 0], np.int32)
    return dict(q=q1, w=w1, info=info, cat=cat.reshape(N, N, N), free=free.reshape(N, N, N), q_m=np.where(upd, q_m, 0).reshape(N, N, N),
                A=np.where(upd, A, 0).reshape(N, N, N))


# ---------------------------------------------------------------------------------------------------- alva_mesh_extract
def extract(q, w, origin3, voxel, min_weight, max_vertices, max_triangles):
    """alva_mesh_extract.  Returns a dict: vertices, normals float32 [nv,3], triangles int32 [nt,3] (all empty unless the code is 0), info
    [8] int32, and for the tests cells [nv,3] (i, j, k of each vertex's cell)."""
    q = np.asarray(q, np.int16)
    N = q.shape[0]
    M = N - 1
    q = q.astype(np.int64)
    o = np.asarray(origin3, np.float64).reshape(-1)
    voxel = np.float64(voxel)
    # X1
    valid = np.asarray(w, np.uint8) >= min_weight
    inside = q < 0
    # X2 (arrays are [k][j][i]; corner c = dx | dy << 1 | dz << 2)
    corner = lambda a, c: a[(c >> 2):(c >> 2) + M, ((c >> 1) & 1):((c >> 1) & 1) + M, (c & 1):(c & 1) + M]
    n_in = sum(corner(inside, c).astype(np.int64) for c in range(8))
    active = functools.reduce(np.logical_and, [corner(valid, c) for c in range(8)]) & (n_in > 0) & (n_in < 8)
    ck, cj, ci = np.nonzero(active)   # ascending (k (N - 1) + j) (N - 1) + i: X5
    nv = len(ci)
    p = [ci, cj, ck]
    qc = [corner(q, c)[active] for c in range(8)]
    # X3
    tot, m = [np.zeros(nv, np.int64) for _ in range(3)], np.zeros(nv, np.int64)
    for a in range(3):
        for lo in range(8):
            if lo & (1 << a):
                continue
            hi = lo | (1 << a)
            cross = (qc[lo] < 0) != (qc[hi] < 0)
            qa, qb = np.abs(qc[lo]), np.abs(qc[hi])
            D = np.where(cross, qa + qb, 1)
            f = (2048 * qa + D) // (2 * D)
            for ax in range(3):
                tot[ax] += np.where(cross, 1024 * (p[ax] + ((lo >> ax) & 1)) + (f if ax == a else 0), 0)
            m += cross
    vertices, normals = np.zeros((nv, 3), F32), np.zeros((nv, 3), F32)
    # X4
    g = [sum(qc[c] if (c >> ax) & 1 else -qc[c] for c in range(8)) for ax in range(3)]
    L2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    length = np.sqrt(np.maximum(L2, 1).astype(np.float64))
    for ax in range(3):
        X = (tot[ax] + m // 2) // np.maximum(m, 1)
        vertices[:, ax] = (o[ax] + (X.astype(np.float64) / 1024.0 + 0.5) * voxel).astype(F32)
        normals[:, ax] = np.where(L2 == 0, F32(0), (g[ax].astype(np.float64) / length).astype(F32))
    # X6
    vid = np.full((N, N, N), -1, np.int64)   # by the cell's voxel index
    vid[ck, cj, ci] = np.arange(nv)
    act = np.zeros((N, N, N), bool)
    act[:M, :M, :M] = active
    vk, vj, vi = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    pv = [vi, vj, vk]
    keys, quads = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ok = (pv[a] < N - 1) & (pv[b] >= 1) & (pv[b] < N - 1) & (pv[c] >= 1) & (pv[c] < N - 1)
        k0, j0, i0 = np.nonzero(ok)
        v = [i0, j0, k0]

        def at(arr, da=0, db=0, dc=0):
            u = list(v)
            u[a], u[b], u[c] = u[a] + da, u[b] + db, u[c] + dc
            return arr[u[2], u[1], u[0]]

        emit = at(valid) & at(valid, 1) & (at(inside) != at(inside, 1)) & at(act, 0, -1, -1) & at(act, 0, 0, -1) & at(act) & at(act, 0, -1, 0)
        Q = np.stack([at(vid, 0, -1, -1), at(vid, 0, 0, -1), at(vid), at(vid, 0, -1, 0)], 1)[emit]
        ins = at(inside)[emit]
        keys.append((((k0 * N + j0) * N + i0) * 3 + a)[emit])
        quads.append(np.where(ins[:, None], Q[:, [0, 1, 2, 0, 2, 3]], Q[:, [0, 2, 1, 0, 3, 2]]))
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    triangles = quads[np.argsort(keys, kind="stable")].reshape(-1, 3).astype(np.int32)
    nt = len(triangles)
    # X7
    code = 3 if nv > max_vertices or nt > max_triangles else 1 if nv == 0 else 0
    info = np.array([code, nv, nt, valid.sum(), (valid & inside).sum(), N, 0, 0], np.int32)
    if code:
        vertices, normals, triangles = np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    return dict(vertices=vertices, normals=normals, triangles=triangles, info=info, cells=np.stack(p, 1) if code == 0 else np.zeros((0, 3), int))


# ---------------------------------------------------------------------------------------------------- analytic scenes
def calib_for(width, height, dist=(0.0, 0.0, 0.0, 0.0)):
    return np.array([0.9 * width, 0.9 * width, width / 2 - 0.5, height / 2 - 0.5, *dist], np.float64)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """T_cw12 of a camera at `eye` whose optical axis (+z) points at `target`; image y points along -up"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross(-np.asarray(up, np.float64), zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])   # R_cw: its rows are the camera's axes in the world
    return np.concatenate([R.reshape(-1), -R @ eye])


def render(scene, T_cw12, calib8, width, height, step):
    """The exact depth (camera z, float32 [gh,gw]; 0 where nothing is hit) of the grid pixels' centre rays.  scene: a list of ("plane", n3,
    d) for the surface n . X = d and ("box", lo3, hi3)"""
    gw, gh = width // step, height // step
    u = np.tile(np.arange(gw) * step + step // 2, gh)
    v = np.repeat(np.arange(gh) * step + step // 2, gw)
    uu, vv = Dc.undistort(calib8, u.astype(F32), v.astype(F32))
    Tm = np.asarray(T_cw12, np.float64)
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    C = -R.T @ t
    dirs = np.stack([(uu.astype(np.float64) - calib8[2]) / calib8[0], (vv.astype(np.float64) - calib8[3]) / calib8[1], np.ones(len(u))], 1) @ R
    best = np.full(len(u), np.inf)
    with np.errstate(all="ignore"):
        for item in scene:
            if item[0] == "plane":
                n, d = np.asarray(item[1], np.float64), float(item[2])
                lam = (d - n @ C) / (dirs @ n)
                lam = np.where(lam > 1e-6, lam, np.inf)
            else:
                lo, hi = np.asarray(item[1], np.float64), np.asarray(item[2], np.float64)
                t0, t1 = (lo - C) / dirs, (hi - C) / dirs
                near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
                lam = np.where((near <= far) & (near > 1e-6), near, np.inf)
            best = np.minimum(best, lam)
    return np.where(np.isfinite(best), best, 0.0).astype(F32).reshape(gh, gw)   # (the ray's direction has camera z = 1: lambda is the depth)


def full_meas(depth, conf=200):
    return depth, np.full(depth.shape, conf, np.uint8), np.zeros(depth.shape, np.uint8)


def empty_volume(N):
    return np.zeros((N, N, N), np.int16), np.zeros((N, N, N), np.uint8)


def hashed_volume(N, seed, q_lo=-32767, q_hi=32767, w_hi=255):
    n = N * N * N
    q = (q_lo + hashed(n, seed) % (q_hi - q_lo + 1)).astype(np.int16).reshape(N, N, N)
    w = (hashed(n, seed + 1) % (w_hi + 1)).astype(np.uint8).reshape(N, N, N)
    return q, w


# ---------------------------------------------------------------------------------------------------- the integrate cases
# the volume: the cube [-1, 1]^3 unless the case says otherwise; the wall: the plane z = 0.3 seen from z < 0
def _icase(name, N, gw, gh, step, eye, target, scene=None, dist=(0, 0, 0, 0), volume=None, meas_edit=None, w_max=W_MAX, origin=(-1.0, -1.0, -1.0),
           side=2.0, trunc_voxels=3.0, T_cw12=None, trunc=None):
    width, height = gw * step, gh * step
    calib = calib_for(width, height, dist)
    T = look_at(eye, target) if T_cw12 is None else np.asarray(T_cw12, np.float64)
    scene = [("plane", (0.0, 0.0, 1.0), 0.3)] if scene is None else scene
    meas = full_meas(render(scene, T, calib, width, height, step))
    if meas_edit is not None:
        meas = meas_edit(*[m.copy() for m in meas])
    q, w = empty_volume(N) if volume is None else volume
    voxel = side / N
    return dict(name=name, q=q, w=w, origin3=np.asarray(origin, np.float64), voxel=voxel, trunc=trunc_voxels * voxel if trunc is None else trunc,
                T_cw12=T, calib8=calib, width=width, height=height, step=step, meas=meas, w_max=w_max)


def _holes_and_codes(depth, conf, code):
    n = depth.size
    code = (hashed(n, 5) % 9).astype(np.uint8).reshape(code.shape)   # every code value 0..7, and 8 for "anything else"
    code[code == 8] = 255
    code[hashed(n, 6).reshape(code.shape) % 3 == 0] = 0
    d = depth.reshape(-1).copy()
    h = hashed(n, 7) % 16
    d[h == 0] = 0.0
    d[h == 1] = -1.0
    d[h == 2] = np.nan
    d[h == 3] = np.inf
    return d.reshape(depth.shape), conf, code


def _conf_edges(depth, conf, code):
    conf = np.array([0, 255, 7, 8, 15, 16, 248], np.uint8)[hashed(depth.size, 8) % 7].reshape(conf.shape)
    return depth, conf, code


@functools.lru_cache(maxsize=None)
def integrate_cases():
    cases = [
        _icase("wall_fronto", 16, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0)),
        _icase("wall_oblique", 17, 32, 24, 4, (1.6, -0.7, -2.2), (0.0, 0.1, 0.3)),
        _icase("distortion", 9, 32, 24, 4, (0.4, 0.2, -2.4), (0.0, 0.0, 0.3), dist=(-0.28, 0.07, 0.0011, -0.0007)),
        _icase("step1", 8, 16, 12, 1, (0.0, 0.3, -2.5), (0.0, 0.0, 0.0)),
        _icase("step8", 33, 64, 48, 8, (-0.5, 0.0, -2.6), (0.0, 0.0, 0.0)),
        _icase("step4_n32", 32, 64, 48, 4, (0.3, -0.2, -2.6), (0.0, 0.0, 0.0)),
        # the camera inside the volume: voxels behind it, voxels beside the image
        _icase("behind_and_outside", 8, 16, 12, 4, (0.1, 0.0, -0.4), (0.6, 0.2, 0.3)),
        _icase("holes_and_codes", 16, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), meas_edit=_holes_and_codes),
        _icase("conf_edges", 9, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), meas_edit=_conf_edges),
        _icase("n4", 4, 16, 12, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0)),
        _icase("n5", 5, 16, 12, 4, (0.2, 0.0, -2.5), (0.0, 0.0, 0.0)),
    ]
    # onto a volume that is not empty: the first view's result, seen from another pose
    first = cases[1]
    r = integrate(first["q"], first["w"], first["origin3"], first["voxel"], first["trunc"], first["T_cw12"], first["calib8"], first["width"],
                  first["height"], first["step"], first["meas"], first["w_max"])
    cases.append(_icase("second_view", 17, 32, 24, 4, (-1.2, 0.5, -2.3), (0.0, 0.0, 0.3), volume=(r["q"], r["w"])))
    # weights at and over w_max (a volume integrated with a larger w_max before), negative numerators
    cases.append(_icase("saturate", 9, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), volume=hashed_volume(9, 11), w_max=100))
    cases.append(_icase("negative_floor", 16, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), volume=hashed_volume(16, 13, -32767, 0, 9)))
    # s exactly -trunc and t exactly 1: identity rotation, everything a dyadic rational -- Pc.z = 1.125 + 0.25 k, the wall at depth 2.125,
    # trunc 0.5, so s = 1 (t = 1: free), 0.75 ... -0.5 (kept: q_m = -32767), -0.75 (hidden)
    exact = _icase("exact_edges", 8, 16, 12, 4, None, None, scene=[("plane", (0.0, 0.0, 1.0), 1.125)], origin=(-1.0, -1.0, 0.0), side=2.0,
                   T_cw12=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1.0], trunc=0.5)
    cases.append(exact)
    return cases


# ---------------------------------------------------------------------------------------------------- the extract cases
def sampled(N, dist_fn, trunc_voxels=3.0, origin=(-1.0, -1.0, -1.0), side=2.0, weight=255):
    """an analytic signed distance (positive outside the solid) sampled straight into q at the voxel centres, with full weights"""
    voxel = side / N
    c = np.asarray(origin)[:, None, None, None] + (np.stack(np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")[::-1]) + 0.5) * voxel
    d = dist_fn(c[0], c[1], c[2])   # arrays [k][j][i]; c[0] is x
    q = np.rint(np.clip(d / (trunc_voxels * voxel), -1.0, 1.0) * 32767.0).astype(np.int16)
    return q, np.full((N, N, N), weight, np.uint8), np.asarray(origin, np.float64), voxel


def sphere_dist(centre, radius):
    return lambda x, y, z: np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def box_dist(lo, hi):
    def f(x, y, z):
        p = np.stack([x, y, z])
        lo_, hi_ = np.asarray(lo)[:, None, None, None], np.asarray(hi)[:, None, None, None]
        d = np.maximum(lo_ - p, p - hi_)
        outside = np.sqrt((np.maximum(d, 0.0) ** 2).sum(0))
        return np.where(d.max(0) > 0, outside, d.max(0))
    return f


SPHERE_C, SPHERE_R = (0.05, -0.03, 0.02), 0.6   # in a volume of side 2 and N >= 16: a radius of at least 4.8 voxels, wholly inside


def _xcase(name, q, w, origin3, voxel, min_weight=1, max_vertices=1 << 20, max_triangles=1 << 21):
    return dict(name=name, q=q, w=w, origin3=origin3, voxel=voxel, min_weight=min_weight, max_vertices=max_vertices, max_triangles=max_triangles)


@functools.lru_cache(maxsize=None)
def extract_cases():
    cases = []
    q, w = empty_volume(8)
    cases.append(_xcase("empty", q, w, np.zeros(3), 0.25))
    q, w = empty_volume(4)
    w[1:3, 1:3, 1:3] = 255
    q[1:3, 1:3, 1:3] = 9000
    q[1, 1, 1] = -4000
    cases.append(_xcase("one_cell", q, w, np.array([0.5, -0.25, 3.0]), 0.125))
    q5, w5 = empty_volume(5)
    w5[:] = 3
    q5[:] = 700
    q5[:, :, :2] = -1300   # a plane between i = 1 and i = 2
    cases.append(_xcase("n5_plane_x", q5, w5, np.array([-0.3, 0.1, 0.7]), 0.2))
    q9 = np.broadcast_to(((np.arange(9) - 4) * 1000).astype(np.int16)[:, None, None], (9, 9, 9)).copy()   # q == 0 at k = 4: outside
    cases.append(_xcase("plane_through_centres", q9, np.full((9, 9, 9), 255, np.uint8), np.array([-1.0, -1.0, -1.0]), 2.0 / 9))
    for N in (16, 17, 32, 33):
        cases.append(_xcase(f"sphere_n{N}", *sampled(N, sphere_dist(SPHERE_C, SPHERE_R))))
    cases.append(_xcase("box_n16", *sampled(16, box_dist((-0.52, -0.4, -0.33), (0.47, 0.55, 0.41)))))
    cases.append(_xcase("box_n8", *sampled(8, box_dist((-0.52, -0.4, -0.33), (0.47, 0.55, 0.41)))))
    q, w, o, vx = sampled(17, sphere_dist(SPHERE_C, SPHERE_R))
    w = w.copy()
    w[:, :, :8] = 0
    cases.append(_xcase("half_valid", q, w, o, vx))
    q, w, o, vx = sampled(16, sphere_dist(SPHERE_C, SPHERE_R))
    w = (hashed(16 ** 3, 21) % 11).astype(np.uint8).reshape(16, 16, 16)
    w[4:12, 4:12, :] = 9   # (a region that passes the gate whole)
    cases.append(_xcase("min_weight", q, w, o, vx, min_weight=5))
    # the caps: hit exactly, exceeded by one
    q, w, o, vx = sampled(16, sphere_dist(SPHERE_C, SPHERE_R))
    full = extract(q, w, o, vx, 1, 1 << 20, 1 << 21)["info"]
    nv, nt = int(full[1]), int(full[2])
    cases.append(_xcase("caps_exact", q, w, o, vx, max_vertices=nv, max_triangles=nt))
    cases.append(_xcase("cap_vertices_over", q, w, o, vx, max_vertices=nv - 1, max_triangles=nt))
    cases.append(_xcase("cap_triangles_over", q, w, o, vx, max_vertices=nv, max_triangles=nt - 1))
    # a surface that leaves the volume: a sphere about a corner region, a wall that crosses every border
    cases.append(_xcase("touches_border", *sampled(17, sphere_dist((-0.8, 0.7, -0.9), 0.7))))
    cases.append(_xcase("hashed_n9", *hashed_volume(9, 31, -3000, 3000, 4), np.array([0.0, 0.0, 0.0]), 0.1, min_weight=1))
    return cases


def scan_case(N=65):
    """more than 1024 workgroups of 256 indices: the scan's threads take more than one workgroup each (for the GPU test only)"""
    return _xcase(f"sphere_n{N}", *sampled(N, sphere_dist(SPHERE_C, SPHERE_R)))


# ---------------------------------------------------------------------------------------------------- mesh properties (for the tests)
def used_vertices(triangles, nv):
    used = np.zeros(nv, bool)
    used[np.asarray(triangles).reshape(-1)] = True
    return used


def edge_census(triangles):
    """the directed edges of the triangles as keys a << 32 | b"""
    t = np.asarray(triangles, np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    return a, b


# ---------------------------------------------------------------------------------------------------- the end-to-end scene
E2E_N, E2E_GW, E2E_GH, E2E_STEP = 32, 64, 48, 4
E2E_WALL_Z = 0.6
E2E_BOX = ((-0.35, -0.3, 0.05), (0.3, 0.35, 0.6))   # stands on the wall, towards the cameras


def e2e_scene():
    return [("plane", (0.0, 0.0, 1.0), E2E_WALL_Z), ("box", *E2E_BOX)]


def e2e_poses():
    """8 poses on an arc in front of the wall, all looking at the box"""
    out = []
    for a in np.linspace(-0.9, 0.9, 8):
        out.append(look_at((2.6 * np.sin(a), -0.5 * np.cos(2 * a), 0.2 - 2.6 * np.cos(a)), (0.0, 0.0, 0.3)))
    return out


@functools.lru_cache(maxsize=None)
def e2e_run():
    """the arc's 8 exact depth images integrated into an empty N = 32 volume over [-1, 1]^3 and extracted with min_weight 2"""
    width, height = E2E_GW * E2E_STEP, E2E_GH * E2E_STEP
    calib = calib_for(width, height)
    q, w = empty_volume(E2E_N)
    origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / E2E_N
    for T in e2e_poses():
        r = integrate(q, w, origin, voxel, 3 * voxel, T, calib, width, height, E2E_STEP, full_meas(render(e2e_scene(), T, calib, width, height, E2E_STEP)))
        q, w = r["q"], r["w"]
    return dict(q=q, w=w, origin3=origin, voxel=voxel, mesh=extract(q, w, origin, voxel, 2, 1 << 20, 1 << 21))


def e2e_surface_distance(p):
    """the distance of points [n,3] from the scene's solid (the wall's half space z >= E2E_WALL_Z united with the box)"""
    p = np.asarray(p, np.float64)
    d_wall = E2E_WALL_Z - p[:, 2]   # positive in front
    lo, hi = np.asarray(E2E_BOX[0]), np.asarray(E2E_BOX[1])
    d = np.maximum(lo - p, p - hi)
    d_box = np.where(d.max(1) > 0, np.sqrt((np.maximum(d, 0.0) ** 2).sum(1)), d.max(1))
    return np.abs(np.minimum(d_wall, d_box))
