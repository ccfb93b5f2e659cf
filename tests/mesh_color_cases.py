"""The mesh colour stages' definitions (include/alvaar_hip.h: alva_color_thumb T1, alva_mesh_integrate_color M1-M5 + K1-K3,
alva_mesh_color_at A0-A4) restated in numpy, operation for operation, the case tables and the analytic painted scene.  The reference has
no mesh colour, so this file is what the three stages are pinned to (tests/test_mesh_color_cases.py checks the restatement against
tests/mesh_cases.py and an analytic painted scene; tests/test_gpu_mesh_color.py the kernels against it, bit for bit).

As in tests/mesh_cases.py the geometry is float64 / float32 exactly where the definition says so, in its operation order, and every
other sum is an integer sum, so the GPU is compared with `==`.  Colours are uint8 [..., 4] = (r, g, b, a); a colour volume is uint8
[N,N,N,4] = (r, g, b, wc) at the index [k][j][i] of the distance volume."""
from __future__ import annotations

import functools

import numpy as np

import depth_cases as Dc
import mesh_cases as Mc
import raycast_cases as Rc

F32 = np.float32
COLOR_STEP = 4   # the system's constant ALVA_MESH_COLOR_STEP (include/alvaar_system.h)


# ---------------------------------------------------------------------------------------------------- alva_color_thumb
def thumb(rgba, cstep):
    """T1.  rgba uint8 [h,w,4] -> uint8 [h // cstep, w // cstep, 4]"""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    tw, th = w // cstep, h // cstep
    assert 1 <= cstep <= 16 and tw >= 1 and th >= 1
    blocks = rgba[:th * cstep, :tw * cstep, :3].astype(np.int64).reshape(th, cstep, tw, cstep, 3)
    s = blocks.sum((1, 3))
    n = cstep * cstep
    out = np.full((th, tw, 4), 255, np.uint8)
    out[:, :, :3] = ((2 * s + n) // (2 * n)).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------- alva_mesh_integrate_color
def integrate_color(q, w, c, origin3, voxel, trunc, T_cw12, calib8, width, height, step, meas, thumb_img, cstep, w_max=Mc.W_MAX):
    """alva_mesh_integrate_color.  q, w, meas as for mesh_cases.integrate; c uint8 [N,N,N,4]; thumb_img uint8 [height // cstep, width //
    cstep, 4].  Nothing is modified.  Returns a dict: q, w, c (the volumes after), info [8] int32, and for the tests cat, free (as
    mesh_cases.integrate), colored [N,N,N] bool, in_thumb [N,N,N] bool (K1's last condition, where the voxel has a pixel)."""
    q0 = np.asarray(q, np.int16)
    N = q0.shape[0]
    q0 = q0.reshape(-1).astype(np.int64)
    w0 = np.asarray(w, np.uint8).reshape(-1).astype(np.int64)
    c0 = np.asarray(c, np.uint8).reshape(-1, 4).astype(np.int64)
    assert len(c0) == N * N * N
    gw, gh = width // step, height // step
    tw, th = width // cstep, height // cstep
    th_img = np.asarray(thumb_img, np.uint8).reshape(th * tw, 4).astype(np.int64)
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
        inimg = front & (F32(0) <= fu) & (fu < F32(gw * step)) & (F32(0) <= fv) & (fv < F32(gh * step))
    iu, iv = np.where(inimg, fu, 0).astype(np.int64), np.where(inimg, fv, 0).astype(np.int64)
    cell = np.where(inimg, (iv // step) * gw + iu // step, 0)
    # M3
    cat[inimg] = 4
    with np.errstate(all="ignore"):
        has = inimg & (code[cell] == 0) & (depth[cell] > F32(0))
    w_m = np.maximum(1, conf[cell] >> 3)
    # M4
    with np.errstate(all="ignore"):
        s = depth[cell].astype(np.float64) - P[2]
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
    q1 = np.where(upd, qn, q0).astype(np.int16).reshape(N, N, N)
    w1 = np.where(upd, wn, w0).astype(np.uint8).reshape(N, N, N)
    # K1
    tx, ty = iu // cstep, iv // cstep
    in_thumb = inimg & (tx < tw) & (ty < th)
    colored = upd & ~free & in_thumb
    # K2
    m = th_img[np.where(in_thumb, ty * tw + tx, 0)]
    # K3
    wc = c0[:, 3]
    Sc = wc + w_m
    c1 = c0.copy()
    for ch in range(3):
        c1[:, ch] = np.where(colored, (2 * (c0[:, ch] * wc + m[:, ch] * w_m) + Sc) // (2 * Sc), c0[:, ch])
    c1[:, 3] = np.where(colored, np.minimum(int(w_max), Sc), wc)
    assert c1.max() <= 255 and c1.min() >= 0
    info = np.array([upd.sum(), hidden.sum(), free.sum(), (cat == 3).sum(), (cat == 4).sum(), N, colored.sum(), 0], np.int32)
    return dict(q=q1, w=w1, c=c1.astype(np.uint8).reshape(N, N, N, 4), info=info, cat=cat.reshape(N, N, N), free=free.reshape(N, N, N),
                colored=colored.reshape(N, N, N), in_thumb=in_thumb.reshape(N, N, N))


# ---------------------------------------------------------------------------------------------------- alva_mesh_color_at
def color_at(c, origin3, voxel, points):
    """alva_mesh_color_at.  c uint8 [N,N,N,4], points float32 [n,3].  Returns a dict: rgba uint8 [n,4], code uint8 [n], info [8] int32, and
    for the tests f int [n,3] (A2's fractions) and n_col int [n] (how many of the cell's corners have a colour)."""
    c = np.asarray(c, np.uint8)
    N = c.shape[0]
    cf = c.reshape(-1, 4).astype(np.int64)
    o = np.asarray(origin3, np.float64).reshape(-1)
    voxel = np.float64(voxel)
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    with np.errstate(all="ignore"):
        # A0
        code4 = ~np.isfinite(p).all(1)
        # A1, A2
        inside = np.ones(n, bool)
        ic, f = [], []
        for a in range(3):
            g = (p[:, a].astype(np.float64) - o[a]) / voxel - 0.5
            inside &= (0.0 <= g) & (g <= np.float64(N - 1))
            i = Rc._clamp_int(np.floor(g), 0, N - 2)
            ic.append(i)
            f.append(Rc._clamp_int(np.rint((g - i.astype(np.float64)) * 256.0), 0, 256))
    # A3
    base = (ic[2] * N + ic[1]) * N + ic[0]
    S = np.zeros(n, np.int64)
    tot = np.zeros((n, 3), np.int64)
    n_col = np.zeros(n, np.int64)
    for k in range(8):
        v = cf[base + (k & 1) + ((k >> 1) & 1) * N + (k >> 2) * N * N]
        wt = [f[a] if (k >> a) & 1 else 256 - f[a] for a in range(3)]
        Wt = wt[0] * wt[1] * wt[2] * v[:, 3]
        S += Wt
        tot += v[:, :3] * Wt[:, None]
        n_col += v[:, 3] > 0
    code = np.where(code4, 4, np.where(~inside, 1, np.where(S == 0, 2, 0)))
    # A4
    Sd = np.where(S == 0, 1, S)
    rgba = np.zeros((n, 4), np.uint8)
    ok = code == 0
    rgba[:, :3] = np.where(ok[:, None], (2 * tot + Sd[:, None]) // (2 * Sd[:, None]), 0).astype(np.uint8)
    rgba[:, 3] = np.where(ok, 255, 0)
    info = np.array([n, (code == 0).sum(), (code == 1).sum(), (code == 2).sum(), (code == 4).sum(), 0, 0, N], np.int32)
    return dict(rgba=rgba, code=code.astype(np.uint8), info=info, f=np.stack(f, 1), n_col=n_col)


# ---------------------------------------------------------------------------------------------------- hashed inputs
def hashed_bytes(shape, seed):
    return (Mc.hashed(int(np.prod(shape)), seed) & 255).astype(np.uint8).reshape(shape)


def hashed_color_volume(N, seed, w_max=Mc.W_MAX, empty_share=0):
    """colours hashed, the weights drawn from {0, 1, w_max - 1, w_max} (and from 0 alone for `empty_share` of 8 more draws)"""
    c = hashed_bytes((N, N, N, 4), seed)
    pick = Mc.hashed(N * N * N, seed + 1) % (4 + empty_share)
    c[..., 3] = np.array([0, 1, w_max - 1, w_max] + [0] * empty_share, np.uint8)[pick].reshape(N, N, N)
    return c


# ---------------------------------------------------------------------------------------------------- the thumbnail cases
def thumb_cases():
    """dicts: name, buf uint8 [H,W,4] (the buffer), r0, c0, h, w (the image is buf[r0:r0 + h, c0:c0 + w]: a padded pitch, an offset base),
    img (that view), cstep"""
    cases = []

    def add(name, h, w, cstep, pad=0, off=0, seed=1):
        buf = np.ascontiguousarray(hashed_bytes((h + 1, w + pad + off, 4), seed + len(cases)))
        cases.append(dict(name=name, buf=buf, r0=1, c0=off, h=h, w=w, img=buf[1:, off:off + w], cstep=cstep))

    for cstep in (1, 3, 4, 16):
        add(f"cstep{cstep}_odd", 37, 53, cstep)                  # neither side a multiple of cstep (but for 1)
        add(f"cstep{cstep}_smallest", cstep, cstep, cstep)       # one cell
        add(f"cstep{cstep}_padded_offset", 35, 70, cstep, pad=9, off=3)
    add("two_blocks_each_way", 21, 4 * 64 + 7, 4)                # more than 64 cells across, more than 4 down
    add("vga", 480, 640, 4)
    return cases


# ---------------------------------------------------------------------------------------------------- the integrate-colour cases
def _ccase(ic, seed, cstep=COLOR_STEP, prior=None, thumb_img=None):
    N = ic["q"].shape[0]
    tw, th = ic["width"] // cstep, ic["height"] // cstep
    c = np.zeros((N, N, N, 4), np.uint8) if prior is None else prior
    t = hashed_bytes((th, tw, 4), seed) if thumb_img is None else thumb_img   # (also the alpha: K2 does not read it)
    return dict(ic, c=c, thumb=t, cstep=cstep)


@functools.lru_cache(maxsize=None)
def integrate_color_cases():
    cases = []
    eye, target = (0.4, 0.2, -2.4), (0.0, 0.0, 0.3)
    dist = (-0.28, 0.07, 0.0011, -0.0007)
    for n, N in enumerate((4, 8, 16, 32)):
        cases.append(_ccase(Mc._icase(f"n{N}_distortion", N, 32, 24, 4, eye, target, dist=dist), 40 + n))
        cases.append(_ccase(Mc._icase(f"n{N}_holes_and_codes", N, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), meas_edit=Mc._holes_and_codes), 50 + n))
        cases.append(_ccase(Mc._icase(f"n{N}_conf_edges", N, 32, 24, 4, (1.6, -0.7, -2.2), (0.0, 0.1, 0.3), meas_edit=Mc._conf_edges), 60 + n,
                            prior=hashed_color_volume(N, 70 + n)))
    # prior colour and prior distance, w_max other than the system's
    cases.append(_ccase(Mc._icase("prior_w100", 9, 32, 24, 4, (0.0, 0.0, -2.5), (0.0, 0.0, 0.0), volume=Mc.hashed_volume(9, 11), w_max=100), 81,
                        prior=hashed_color_volume(9, 82, w_max=100)))
    # 130 x 98 pixels at step 2, cstep 4: the thumbnail is 32 x 24, and the pixels of columns 128, 129 and rows 96, 97 have no cell in it
    # (the camera is near: the volume fills the image past its right and lower borders)
    cases.append(_ccase(Mc._icase("thumb_gate", 16, 65, 49, 2, (0.0, 0.0, -1.2), (0.0, 0.0, 0.1)), 83))
    # cstep other than the system's, and coarser than the depth grid
    cases.append(_ccase(Mc._icase("cstep1", 8, 16, 12, 4, (0.0, 0.3, -2.5), (0.0, 0.0, 0.0)), 84, cstep=1))
    cases.append(_ccase(Mc._icase("cstep16", 16, 32, 24, 4, (0.3, -0.2, -2.6), (0.0, 0.0, 0.0)), 85, cstep=16))
    return cases


def stride_case(N=81):
    """N^3 > 2048 x 256: the kernel's stride loop runs more than once (for the GPU test only)"""
    return _ccase(Mc._icase(f"n{N}", N, 64, 48, 4, (0.3, -0.2, -2.6), (0.0, 0.0, 0.0)), 86, prior=hashed_color_volume(N, 87))


def run_integrate_color(c):
    return integrate_color(c["q"], c["w"], c["c"], c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"],
                           c["step"], c["meas"], c["thumb"], c["cstep"], c["w_max"])


# ---------------------------------------------------------------------------------------------------- the colour-at cases
CA_N, CA_ORIGIN, CA_VOXEL = 8, np.array([-1.0, -1.0, -1.0]), 0.25   # dyadic: g is exact for the points below


def color_at_volume():
    """hashed; half of the draws have no colour, so cells have one, some, all and no coloured corner"""
    c = hashed_color_volume(CA_N, 91, empty_share=4)
    c[:2, :2, :2, 3] = 0        # the cell (0, 0, 0) and its neighbours: nothing
    c[6:, 6:, :2, 3] = 5        # the cell (0, 6, 6): all eight
    c[5, 5, 5, 3] = 77          # the cell (4, 4, 4): exactly one corner
    c[4, 4:6, 4:6, 3] = 0
    c[5, 4, 4:6, 3] = 0
    c[5, 5, 4, 3] = 0
    return c


def color_at_points():
    """float32 [n,3]: cell centres, faces and corners, A1's ends and a float32 either side of them, non-finite components"""
    o, vx, N = CA_ORIGIN, CA_VOXEL, CA_N
    at = lambda g: o + (np.asarray(g, np.float64) + 0.5) * vx
    pts = []
    gi = np.arange(N - 1)
    G = np.stack(np.meshgrid(gi, gi, gi, indexing="ij"), -1).reshape(-1, 3)
    pts.append(at(G + 0.5))                                  # every cell's centre: f = 128
    pts.append(at(G[::7].astype(np.float64)))                # corners: f = 0
    pts.append(at(G[::5] + np.array([0.5, 0.0, 0.25])))      # on a face
    pts.append(at(G[::11] + 1.0 - 1.0 / 1024))               # f = 256 by rounding
    lo, hi = at([0, 0, 0])[0], at([N - 1] * 3)[0]
    mid = at([3.3, 2.6, 4.1])
    for a in range(3):
        for e in (lo, hi):
            e32 = F32(e)
            assert float(e32) == e
            for v in (e32, np.nextafter(e32, F32(-9)), np.nextafter(e32, F32(9))):
                p = mid.copy()
                p[a] = v
                pts.append(p[None])
    pts.append(np.array([[hi, hi, hi], [lo, lo, lo], [hi, lo, hi]]))   # the volume's corners: i = N - 2 with f = 256, i = 0 with f = 0
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = mid.copy()
            p[a] = bad
            pts.append(p[None])
    pts.append(np.array([[3e38, 0, 0], [0, -3e38, 0], [1e9, 1e9, 1e9], [-5.0, 0.1, 0.1]]))   # far outside: the clamps come first
    return np.concatenate(pts).astype(F32)


def nudged_origins():
    """A1's ends to one double: the origin one double either side (the points are float32, and exactly on the ends for CA_ORIGIN)"""
    out = []
    for d in (-9.0, 9.0):
        for a in range(3):
            o = CA_ORIGIN.copy()
            o[a] = np.nextafter(o[a], d)
            out.append(o)
    return out


def end_points():
    lo, hi = CA_ORIGIN[0] + 0.5 * CA_VOXEL, CA_ORIGIN[0] + (CA_N - 0.5) * CA_VOXEL
    mid = (CA_ORIGIN + (np.array([3.3, 2.6, 4.1]) + 0.5) * CA_VOXEL)
    pts = []
    for a in range(3):
        for e in (lo, hi):
            p = mid.copy()
            p[a] = e
            pts.append(p)
    return np.asarray(pts, F32)


# ---------------------------------------------------------------------------------------------------- the painted end-to-end scene
# mesh_cases' wall with a box on it, seen from mesh_cases' 8 views, every surface painted with its own base colour plus a colour linear
# in the world coordinates.  The box is not mesh_cases' E2E_BOX: on that one 70.0 % of the used vertices lie within 1.5 voxels of a box
# edge (22.5 %) or of a silhouette in one of the views -- the 8 views' shadows of a box 0.55 deep sweep most of the wall beside it, and
# two of its faces are never seen -- against the 25 % the test allows.  This box has E2E_BOX's front (z = 0.3, the wall at 0.6) and
# leaves the volume on three sides: a step across the wall, one edge at its top, one at its foot, a face the views see from below
PAINT_BOX = ((-2.0, -2.0, 0.3), (2.0, 0.0, 0.6))


def paint_scene():
    return [("plane", (0.0, 0.0, 1.0), Mc.E2E_WALL_Z), ("box", *PAINT_BOX)]


PAINT_GRAD = np.array([[30.0, -20.0, 10.0], [-15.0, 25.0, 20.0], [20.0, 15.0, -30.0]])   # d(r, g, b) / d(x, y, z), counts per world unit
PAINT_BASE = {1: (150.0, 90.0, 60.0),      # the wall
              2: (60.0, 140.0, 100.0),     # the box's faces of constant x
              3: (100.0, 60.0, 160.0),     # of constant y
              4: (180.0, 170.0, 80.0)}     # of constant z


def surface_id(p, tol):
    """which surface the points [n,3] lie on (within tol): 1 the wall, 2 / 3 / 4 the box's faces of constant x / y / z; 0 none"""
    p = np.asarray(p, np.float64)
    lo, hi = np.asarray(PAINT_BOX[0]), np.asarray(PAINT_BOX[1])
    d_wall = np.abs(Mc.E2E_WALL_Z - p[:, 2])
    d = np.maximum(lo - p, p - hi)
    d_box = np.where(d.max(1) > 0, np.sqrt((np.maximum(d, 0.0) ** 2).sum(1)), -d.max(1))
    face = 2 + np.argmax(d, 1)
    sid = np.where(d_box <= d_wall, face, 1)
    return np.where(np.minimum(d_wall, d_box) <= tol, sid, 0)


def paint(p, sid):
    """the analytic colour (float64 [n,3]) of points on surface sid"""
    base = np.array([PAINT_BASE.get(int(s), (0.0, 0.0, 0.0)) for s in sid])
    return base + np.asarray(p, np.float64) @ PAINT_GRAD.T


def render_color(T_cw12, calib8, width, height):
    """the painted scene at full resolution: (rgba uint8 [height,width,4], sid int [height,width])"""
    depth = Mc.render(paint_scene(), T_cw12, calib8, width, height, 1).reshape(-1).astype(np.float64)
    u = np.tile(np.arange(width), height)
    v = np.repeat(np.arange(height), width)
    uu, vv = Dc.undistort(calib8, u.astype(F32), v.astype(F32))
    Tm = np.asarray(T_cw12, np.float64)
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    C = -R.T @ t
    dirs = np.stack([(uu.astype(np.float64) - calib8[2]) / calib8[0], (vv.astype(np.float64) - calib8[3]) / calib8[1], np.ones(len(u))], 1) @ R
    X = C + depth[:, None] * dirs
    sid = np.where(depth > 0, surface_id(X, 1e-3), 0)
    col = np.where((sid > 0)[:, None], np.clip(np.rint(paint(X, sid)), 0, 255), 0)
    rgba = np.concatenate([col, np.full((len(u), 1), 255.0)], 1).astype(np.uint8)
    return rgba.reshape(height, width, 4), sid.reshape(height, width)


@functools.lru_cache(maxsize=None)
def e2e_color_run():
    """mesh_cases.e2e_run with colour: every view rendered at full resolution, reduced with cstep 4 and fused; the mesh's vertices
    sampled from the colour volume"""
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib = Mc.calib_for(width, height)
    q, w = Mc.empty_volume(Mc.E2E_N)
    c = np.zeros((Mc.E2E_N,) * 3 + (4,), np.uint8)
    origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / Mc.E2E_N
    sids = []
    for T in Mc.e2e_poses():
        rgba, sid = render_color(T, calib, width, height)
        sids.append(sid)
        meas = Mc.full_meas(Mc.render(paint_scene(), T, calib, width, height, Mc.E2E_STEP))
        r = integrate_color(q, w, c, origin, voxel, 3 * voxel, T, calib, width, height, Mc.E2E_STEP, meas, thumb(rgba, COLOR_STEP), COLOR_STEP)
        q, w, c = r["q"], r["w"], r["c"]
    mesh = Mc.extract(q, w, origin, voxel, 2, 1 << 20, 1 << 21)
    return dict(q=q, w=w, c=c, origin3=origin, voxel=voxel, mesh=mesh, colors=color_at(c, origin, voxel, mesh["vertices"]), sids=sids, calib=calib,
                width=width, height=height)


def e2e_excluded(V, voxel, sids, calib, width, height, margin=1.5):
    """the vertices [n,3] within `margin` voxels of a box edge, or, in one of the views, of a silhouette or an edge between two painted
    surfaces: an image-space distance of margin voxels at the vertex's depth to a pixel whose right or lower neighbour is another surface"""
    V = np.asarray(V, np.float64)
    lo, hi = np.asarray(PAINT_BOX[0]), np.asarray(PAINT_BOX[1])
    out = np.zeros(len(V), bool)
    # the box's 12 edges: the distance to an edge along axis a is that of the other two coordinates to the edge's, and of a to its span
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        da = np.maximum(np.maximum(lo[a] - V[:, a], V[:, a] - hi[a]), 0.0)
        for eb in (lo[b], hi[b]):
            for ec in (lo[c], hi[c]):
                out |= np.sqrt(da ** 2 + (V[:, b] - eb) ** 2 + (V[:, c] - ec) ** 2) <= margin * voxel
    for T, sid in zip(Mc.e2e_poses(), sids):
        edge = np.zeros(sid.shape, bool)
        edge[:, :-1] |= sid[:, :-1] != sid[:, 1:]
        edge[:-1, :] |= sid[:-1, :] != sid[1:, :]
        ev, eu = np.nonzero(edge)
        R, t = T[:9].reshape(3, 3), T[9:]
        P = V @ R.T + t
        u, v = calib[0] * P[:, 0] / P[:, 2] + calib[2], calib[1] * P[:, 1] / P[:, 2] + calib[3]
        r = margin * voxel * calib[0] / P[:, 2] + 1.0   # (the edge lies between the pixel and its neighbour)
        for s in range(0, len(V), 256):
            d2 = (u[s:s + 256, None] - eu[None, :]) ** 2 + (v[s:s + 256, None] - ev[None, :]) ** 2
            out[s:s + 256] |= d2.min(1) <= r[s:s + 256] ** 2
    return out
