"""Match-to-map's case table: small maps BUILT, not drawn, so that every gate, threshold, scan position and entry form of
csrc/match_to_map.hip (Mapper::matchToMap restated) is reached on purpose.

A case is a map in the layout the helpers of oracles.py take (`pb`, `aux`), optional "has a descriptor" arrays (`mhd` per map point, `ohd`
per observation; None = the flat form applies), call arguments (`kw`), and what the case is FOR:
  claims   {local list position: {trace column: value}} -- what orc_match_to_map_trace must report there
  matches  {keypoint row: local map point row}          -- the whole expected result, stated by the case, not taken from the checker
tests/test_mtm_cases.py proves both on the CPU; tests/test_gpu_match_to_map_cases.py runs the three device entry points over the table.

Exactness.  Keyframe rotations are the identity, translations and camera coordinates are binary fractions, fx = fy = 512, no distortion:
a camera point (k / 512, l / 512, 1) projects to exactly (cx + k, cy + l), and every quantity a threshold is compared with is a float
the case chooses.  A threshold case comes as TWINS: one map AT the threshold and one a single float / double past it.  `exact` holds
the quantity recomputed here in the kernel's own operation order; the CPU test checks it equals the threshold bit for bit.

Consistency.  A keypoint lies in the cell Frame::addKeypointToGrid puts it in, cells are filled in insertion order, and every grid entry
observes the frame -- so the compiled reference can run the same maps -- except in `rec_grid_entry_without_frame_obs`, which exists
for the record form's guard against exactly that."""
from __future__ import annotations

import numpy as np

F32 = np.float32
FX = 512.0
CY = 240.0
MIN_DIST_DEFAULT = F32(32 * F32(0.2) * 8.)     # 51.2f


def desc_bits(n, byte0=0):
    """32 descriptor bytes with the first n bits set (from byte `byte0`): hamming(desc_bits(a), desc_bits(b)) = |a - b|"""
    d = np.zeros(32, np.uint8)
    for b in range(n):
        d[byte0 + (b >> 3)] |= np.uint8(1 << (b & 7))
    return d


class MapBuilder:
    """Rows are map points; a row with an observation in the LAST keyframe (the frame) is a frame keypoint, stored in the frame's grid in
    insertion order."""

    def __init__(self, n_kf=2, W=640, H=480, cell=35, cx=320.0, kf_t=None):
        self.calib = np.array([FX, FX, cx, CY, 0, 0, 0, 0, W, H], np.float64)
        self.cell, self.n_kf, self.frame = cell, n_kf, n_kf - 1
        self.kf_t = np.zeros((n_kf, 3))
        for k in range(n_kf - 1):
            self.kf_t[k] = (0.0, 0.0, 1.0 + k) if kf_t is None else kf_t[k]      # further back: what the frame sees, they see
        self.rows, self.kp_order = [], []

    def proj(self, X, kf):
        """CameraCalibration::projectCamToImageDist of world point X in keyframe kf, in its operation order (zero distortion)"""
        cp = np.asarray(X, np.float64) + self.kf_t[kf]
        iz = 1.0 / cp[2]
        xf, yf = F32(cp[0] * iz), F32(cp[1] * iz)
        return F32(np.float64(xf) * self.calib[0] + self.calib[2]), F32(np.float64(yf) * self.calib[1] + self.calib[3])

    def add(self, X, obs, is3d=1, has_desc=1):
        """obs: [(keyframe index, (px, py), desc32, flagged)]"""
        obs = sorted(((int(k), (F32(p[0]), F32(p[1])), np.asarray(d, np.uint8), bool(f)) for k, p, d, f in obs), key=lambda o: o[0])
        assert len({o[0] for o in obs}) == len(obs)
        self.rows.append(dict(X=np.asarray(X, np.float64), obs=obs, is3d=is3d, has_desc=has_desc))
        row = len(self.rows) - 1
        if any(o[0] == self.frame for o in obs):
            self.kp_order.append(row)
        return row

    def keypoint(self, px, py, bits=0, also=(), flagged=True, has_desc=1, desc=None):
        """a tracked map point holding the frame keypoint at (px, py); `also` = [(keyframe, (px, py))] further observations"""
        d = desc_bits(bits) if desc is None else desc
        return self.add((0.25, 0.125, 4.0), [(k, p, d, flagged) for k, p in also] + [(self.frame, (px, py), d, flagged)], has_desc=has_desc)

    def point_at(self, pu, pv, z=1.0):
        return np.array([(np.float64(pu) - self.calib[2]) / FX * z, (np.float64(pv) - CY) / FX * z, z])

    def local_point(self, pu, pv, z=1.0, kfs=(0,), bits=0, is3d=1, has_desc=1, flagged=True, X=None, descs=None):
        """an old map point whose projection into the frame is exactly (pu, pv), observed -- without error -- in keyframes kfs"""
        X = self.point_at(pu, pv, z) if X is None else np.asarray(X, np.float64)
        fl = flagged if isinstance(flagged, (list, tuple)) else [flagged] * len(kfs)
        ds = descs if descs is not None else [desc_bits(bits)] * len(kfs)
        return self.add(X, [(k, self.proj(X, k), ds[i], fl[i]) for i, k in enumerate(kfs)], is3d=is3d, has_desc=has_desc)

    def filler(self):
        """a row that takes part in nothing: not 3-D, not in the frame"""
        return self.add((0.0, 0.0, 3.0), [(0, (50.0, 50.0), desc_bits(200), True)], is3d=0)

    def finish(self, local, flags=None):
        n_mp = len(self.rows)
        W, H, cs = self.calib[8], self.calib[9], self.cell
        ncw, nch = int(np.ceil(F32(W) / F32(cs))), int(np.ceil(F32(H) / F32(cs)))
        mp_id = (500 + 3 * np.arange(n_mp)).astype(np.int32)
        obs_ptr, obs_kf, obs_px, obs_desc, ohd, frame_obs = [0], [], [], [], [], {}
        for m, r in enumerate(self.rows):
            for k, p, d, f in r["obs"]:
                if k == self.frame:
                    frame_obs[m] = len(obs_kf)
                assert 0 <= p[0] < W and 0 <= p[1] < H, "every keyframe holds its keypoints inside the image"
                obs_kf.append(k)
                obs_px.append(p)
                obs_desc.append(d)
                ohd.append(1 if f else 0)
            obs_ptr.append(len(obs_kf))
        cells = [[] for _ in range(ncw * nch)]
        for m in self.kp_order:
            px = obs_px[frame_obs[m]]
            assert 0 <= px[0] < W and 0 <= px[1] < H, "a frame keypoint lies inside the image"
            cells[int(np.floor(px[1] / F32(cs))) * ncw + int(np.floor(px[0] / F32(cs)))].append(int(mp_id[m]))
        cell_ptr = np.zeros(len(cells) + 1, np.int32)
        cell_ptr[1:] = np.cumsum([len(c) for c in cells])
        kf_pose = np.zeros((self.n_kf, 7))
        kf_pose[:, :3], kf_pose[:, 6] = -self.kf_t, 1.0          # T_wc of an identity rotation: centre = -t_cw
        kf_q = np.zeros((self.n_kf, 4))
        kf_q[:, 3] = 1.0
        pb = dict(calib=self.calib, cell_size=cs, kf_id=np.arange(10, 10 + self.n_kf, dtype=np.int32), kf_pose=kf_pose, mp_id=mp_id,
                  mp_wpt=np.array([r["X"] for r in self.rows], np.float64).reshape(n_mp, 3), mp_is3d=np.array([r["is3d"] for r in self.rows], np.uint8),
                  obs_ptr=np.array(obs_ptr, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_px=np.array(obs_px, np.float32).reshape(-1, 2),
                  obs_desc=np.array(obs_desc, np.uint8).reshape(-1, 32), frame_kp_order=np.array([frame_obs[m] for m in self.kp_order], np.int32),
                  local=mp_id[np.asarray(local, np.int64)].astype(np.int32) if len(local) else np.zeros(0, np.int32), num_kp3d=100)
        aux = dict(kf_q=kf_q, kf_t=self.kf_t.copy(), grid_cells=len(cells), num_cells_w=ncw, cell_ptr=cell_ptr,
                   cell_kp=np.array([i for c in cells for i in c], np.int32), local_order=pb["local"].copy())
        mhd = np.array([r["has_desc"] for r in self.rows], np.uint8)
        ohd = np.array(ohd, np.uint8)
        need = bool((mhd == 0).any() or (ohd == 0).any()) if flags is None else flags
        return pb, aux, (mhd if need else None), (ohd if need else None)


CASES = []
TWINS = []    # (kept case, dropped case, the ending of the dropped twin's point, the gate column that takes the candidate or None)


def _case(name, group, m, local, claims, matches, scan=True, exact=None, rec=None, only=None, flags=None, **kw):
    pb, aux, mhd, ohd = m.finish(local, flags)
    CASES.append(dict(name=name, group=group, pb=pb, aux=aux, mhd=mhd, ohd=ohd, kw=kw, claims=claims, matches=dict(matches), scan=scan,
                      exact=exact or {}, rec=rec or {}, only=only))
    return CASES[-1]


def _twin(kept, dropped, end, gate=None):
    TWINS.append((kept, dropped, end, gate))


def _pxdist(pu, pv, kx, ky):
    dx, dy = F32(F32(pu) - F32(kx)), F32(F32(pv) - F32(ky))
    return F32(np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ------------------------------------------------------------------------------------------------------------------ point gates
# In every one of these a keypoint with an identical descriptor sits one pixel from the projection: a missing gate gives a match.
def _point_gate(name, end, scan, match, cx=320.0, flags=None, kf_t=None, **lp):
    m = MapBuilder(cx=cx, kf_t=kf_t)
    pu, pv = lp.pop("pu", 320.0), lp.pop("pv", 240.0)
    kx, ky = lp.pop("kp", (min(max(pu, 0.0) + 1.0, 639.0), min(max(pv, 0.0), 479.0)))
    also_frame = lp.pop("observed", False)
    kfs = lp.pop("kfs", (0,))
    M = m.local_point(pu, pv, kfs=kfs + ((m.frame,) if also_frame else ()), **lp)
    K = m.keypoint(kx, ky)
    claims = {0: dict(end=end)}
    if scan:
        claims[0].update(total=1 + (1 if also_frame else 0), nvalid=1)
    return _case(name, "point", m, [M], claims, {K: M} if match else {}, scan=scan, flags=flags)


_point_gate("pt_observed_in_frame", "observed", False, False, observed=True)
_point_gate("pt_not_3d", "not3d_or_nodesc", False, False, is3d=0)
_point_gate("pt_no_desc_empty_obs", "not3d_or_nodesc", False, False, kfs=())
_point_gate("pt_no_desc_flag", "not3d_or_nodesc", False, False, has_desc=0)
_point_gate("pt_has_desc_flag", "matched", True, True, flags=True)
_twin("pt_has_desc_flag", "pt_no_desc_flag", "not3d_or_nodesc")
# depth: campt[2] < 0.1 with campt = wpt (frame translation 0): the double 0.1 is kept, the double below it dropped
_point_gate("pt_z_eq_0p1", "matched", True, True, z=0.1, kf_t=[(0.0, 0.0, 0.5)]).update(exact=dict(z=(0.1, 0.1)))
_point_gate("pt_z_below_0p1", "behind", False, False, z=float(np.nextafter(0.1, 0.0)), kf_t=[(0.0, 0.0, 0.5)])
_twin("pt_z_eq_0p1", "pt_z_below_0p1", "behind")
# view cone: |z / |p|| < cos(atan(max half-fov tangent)); (636, 470) is inside the image but outside the cone, (636, 240) has the same
# x and is inside it
_point_gate("pt_view_corner_rejected", "view", False, False, pu=636.0, pv=470.0)
_point_gate("pt_view_axis_same_x_passes", "matched", True, True, pu=636.0, pv=240.0)
_twin("pt_view_axis_same_x_passes", "pt_view_corner_rejected", "view")
# image bounds.  pu == 0 needs cx = 300: with cx = 320 the float below 0 already leaves the view cone
_point_gate("pt_pu_eq_0", "matched", True, True, cx=300.0, pu=0.0).update(exact=dict(pu=(0.0, 0.0)))
_point_gate("pt_pu_below_0", "outside", False, False, cx=300.0, pu=0.0, kp=(1.0, 240.0),
            X=(float(_down(-300.0 / 512.0)), 0.0, 1.0))
_twin("pt_pu_eq_0", "pt_pu_below_0", "outside")
_point_gate("pt_pv_eq_0", "matched", True, True, pv=0.0, kp=(321.0, 0.0))
_point_gate("pt_pv_below_0", "outside", False, False, pv=0.0, kp=(321.0, 0.0), X=(0.0, float(_down(-240.0 / 512.0)), 1.0))
_twin("pt_pv_eq_0", "pt_pv_below_0", "outside")
_point_gate("pt_pu_eq_W", "outside", False, False, pu=640.0, kp=(639.0, 240.0)).update(exact=dict(pu=(640.0, 640.0)))
_point_gate("pt_pu_below_W", "matched", True, True, pu=float(_down(640.0)), kp=(639.0, 240.0))
_twin("pt_pu_below_W", "pt_pu_eq_W", "outside")
_point_gate("pt_pv_eq_H", "outside", False, False, pv=480.0, kp=(320.0, 479.0))
_point_gate("pt_pv_below_H", "matched", True, True, pv=float(_down(480.0)), kp=(320.0, 479.0))
_twin("pt_pv_below_H", "pt_pv_eq_H", "outside")


# ------------------------------------------------------------------------------------------------ the scan over the 2 x 2 cells
def _scan_map(occ, valid, cell=35, ckp=9, rkp=7, W=640, H=480, m_bits=0):
    """One local point projecting half a pixel inside cell (rkp, ckp), next to the junction of the four cells the walk visits, which hold
    occ[0..3] keypoints in walk order.  valid = {scan position: descriptor distance}: those keypoints lie within 2 px of the projection;
    all the others lie in the same cells, 5 px or more away (the pixel gate takes them)."""
    m = MapBuilder(cell=cell, W=W, H=H)
    jx, jy = float(ckp * cell), float(rkp * cell)
    M = m.local_point(jx + 0.5, jy + 0.5, bits=m_bits)
    rows, p = {}, 0
    for j, n in enumerate(occ):
        sx, sy = (-1.0 if j in (0, 2) else 1.0), (-1.0 if j in (0, 1) else 1.0)
        for _ in range(n):
            if p in valid:
                rows[p] = m.keypoint(jx + 0.5 * sx, jy + 0.5 * sy, bits=valid[p] + m_bits)
            else:
                m.keypoint(jx + sx * (4.0 + 0.5 * (p % 8)), jy + sy * 4.0, bits=0)
            p += 1
    assert all(q in rows for q in valid)
    return m, M, rows


def _scan(name, group, occ, valid, best, sec, end="matched", merges=(0, 0, 0), **kw):
    mkw = {k: kw.pop(k) for k in ("cell", "ckp", "rkp", "W", "H") if k in kw}
    m, M, rows = _scan_map(occ, valid, **mkw)
    total = sum(occ)
    claim = dict(end=end, total=total, px=total - len(valid), nvalid=len(valid), best_pos=best, sec_pos=sec, merge_better=merges[0],
                 merge_equal=merges[1], merge_worse=merges[2], best_dist=float(valid[best]))
    if sec >= 0:
        claim["sec_dist"] = float(valid[sec])
    return _case(name, group, m, [M], {0: claim}, {rows[best]: M} if end == "matched" else {}, **kw)


OCC150 = [40, 50, 30, 30]      # chunk boundaries (64, 128) fall inside the second and the fourth cell
# neighbourhood sizes: a worse candidate first, the best one last
for n, occ in ((1, [0, 0, 0, 1]), (63, [20, 20, 20, 3]), (64, [30, 30, 2, 2]), (65, [30, 30, 3, 2]), (128, [64, 0, 64, 0]), (129, [60, 9, 0, 60]),
               (150, OCC150)):
    v = {0: 10} if n == 1 else {0: 12, n - 1: 10}
    chunks_apart = (n - 1) // 64 > 0
    _scan(f"scan_size_{n}", "scan", occ, v, n - 1, 0 if n > 1 else -1, merges=(1, 0, 0) if chunks_apart else (0, 0, 0))
# a single valid candidate at each position where a chunk begins or ends
for p in (0, 63, 64, 127, 128, 149):
    _scan(f"scan_only_valid_at_{p}_chunk{p // 64}", "scan", OCC150, {p: 10}, p, -1)
_scan("scan_equal_best_chunk0_chunk2_later_wins", "scan", OCC150, {5: 0, 135: 0}, 135, 5, merges=(0, 1, 0))
_scan("scan_equal_best_chunk0_chunk1_later_wins", "scan", OCC150, {3: 0, 70: 0}, 70, 3, merges=(0, 1, 0))
_scan("scan_equal_nonzero_chunk0_chunk1_ratio_rejects", "scan", OCC150, {3: 10, 70: 10}, 70, 3, end="ratio_reject", merges=(0, 1, 0))
_scan("scan_best_chunk0_second_chunk2", "scan", OCC150, {5: 9, 135: 10}, 5, 135, merges=(0, 0, 1))
_scan("scan_second_chunk0_best_chunk2", "scan", OCC150, {5: 10, 135: 9}, 135, 5, merges=(1, 0, 0))
_scan("scan_two_valid_in_chunk2_none_before_best_first", "scan", OCC150, {130: 9, 140: 10}, 130, 140)
_scan("scan_two_valid_in_chunk2_none_before_best_last", "scan", OCC150, {130: 10, 140: 9}, 140, 130)
# a later chunk between best and second: the second distance must drop to it -- (10, 30) passes the ratio test, (10, 11) does not
_scan("scan_later_chunk_between_best_and_second_rejects", "scan", OCC150, {3: 10, 10: 30, 135: 11}, 3, 135, end="ratio_reject", merges=(0, 0, 1))
_scan("scan_later_chunk_between_best_and_second_kept", "scan", OCC150, {3: 10, 10: 30, 135: 12}, 3, 135, merges=(0, 0, 1))
_scan("scan_three_equal_in_one_chunk_last_wins", "scan", OCC150, {3: 0, 20: 0, 40: 0}, 40, 20)
_scan("scan_three_chunks_each_better", "scan", OCC150, {10: 30, 100: 20, 140: 10}, 140, 100, merges=(2, 0, 0))
_scan("scan_three_chunks_each_worse", "scan", OCC150, {10: 10, 100: 20, 140: 12}, 10, 140, merges=(0, 0, 2))

# ------------------------------------------------------------------------------------------------------------------- cell walk
_scan("walk_occupancy_0_70_0_5_chunk_boundary_inside_cell", "walk", [0, 70, 0, 5], {63: 30, 64: 12, 72: 10}, 72, 64, merges=(1, 0, 0))
_scan("walk_occupancy_3_0_2_0", "walk", [3, 0, 2, 0], {1: 12, 4: 10}, 4, 1)
for cell, ckp, rkp, W, H in ((16, 20, 15, 640, 480), (35, 9, 7, 640, 480), (64, 5, 4, 640, 480), (64, 5, 3, 600, 450), (35, 8, 6, 600, 450)):
    _scan(f"walk_cell{cell}_W{W}_one_keypoint_per_cell", "walk", [1, 1, 1, 1], {0: 30, 1: 20, 2: 10, 3: 12}, 2, 3, cell=cell, ckp=ckp, rkp=rkp, W=W, H=H)


def _walk(name, pu, pv, kps, total, match_index, end):
    """kps: keypoints (px, py); the one at match_index (or None) is the expected match"""
    m = MapBuilder()
    M = m.local_point(pu, pv)
    K = [m.keypoint(x, y) for x, y in kps]
    return _case(name, "walk", m, [M], {0: dict(end=end, total=total)}, {K[match_index]: M} if match_index is not None else {})


_walk("walk_row0_cells_above_skipped", 320.0, 20.0, [(300.0, 20.0), (321.0, 20.0)], 2, 1, "matched")
_walk("walk_col0_cells_left_skipped", 20.0, 240.0, [(21.0, 215.0), (21.0, 240.0)], 2, 1, "matched")
_walk("walk_last_row", 320.0, 475.0, [(321.0, 476.0), (310.0, 440.0)], 2, 0, "matched")
_walk("walk_last_col", 632.0, 240.0, [(633.0, 241.0), (600.0, 220.0)], 2, 0, "matched")
# one pixel away, but in a cell the walk does not visit (it looks up and left only)
_walk("walk_keypoint_right_of_cell_not_visited", 69.5, 100.0, [(70.5, 100.0), (40.0, 80.0)], 1, None, "no_valid")
_walk("walk_keypoint_left_of_cell_visited", 70.5, 100.0, [(69.5, 100.0)], 1, 0, "matched")
_twin("walk_keypoint_left_of_cell_visited", "walk_keypoint_right_of_cell_not_visited", "no_valid")
_walk("walk_keypoint_below_cell_not_visited", 100.0, 69.5, [(100.0, 70.5), (80.0, 40.0)], 1, None, "no_valid")
_walk("walk_keypoint_above_cell_visited", 100.0, 70.5, [(100.0, 69.5)], 1, 0, "matched")
_twin("walk_keypoint_above_cell_visited", "walk_keypoint_below_cell_not_visited", "no_valid")


# ------------------------------------------------------------------------------------------------------------ candidate gates
def _px_case(name, kx, kp3, end, dist=None):
    """projection (0.5, 240), keypoint (kx, 240): pxDist = kx - 0.5 exactly, floats in [2, 8) being dense enough to hold both"""
    m = MapBuilder()
    M = m.local_point(0.5, 240.0)
    K = m.keypoint(kx, 240.0)
    ok = end == "matched"
    return _case(name, "gate", m, [M], {0: dict(end=end, total=1, px=0 if ok else 1, nvalid=1 if ok else 0)}, {K: M} if ok else {},
                 exact=dict(pxDist=(_pxdist(0.5, 240.0, kx, 240.0), F32(dist))) if dist is not None else None, num_kp3d=kp3)


_px_case("gate_px_eq_max_kept", 2.5, 30, "matched", 2.0)
_px_case("gate_px_next_float_dropped", _up(2.5), 30, "no_valid", _up(2.0))
_twin("gate_px_eq_max_kept", "gate_px_next_float_dropped", "no_valid", "px")
# fewer than 30 3-D keypoints in the frame double the pixel gate: 4.0 is kept with 29 and dropped with 30
_px_case("gate_px_eq_doubled_max_kp3d_29_kept", 4.5, 29, "matched", 4.0)
_px_case("gate_px_eq_doubled_max_kp3d_30_dropped", 4.5, 30, "no_valid", 4.0)
_twin("gate_px_eq_doubled_max_kp3d_29_kept", "gate_px_eq_doubled_max_kp3d_30_dropped", "no_valid", "px")
_px_case("gate_px_next_float_after_doubled_max_kp3d_29_dropped", _up(4.5), 29, "no_valid", _up(4.0))
_twin("gate_px_eq_doubled_max_kp3d_29_kept", "gate_px_next_float_after_doubled_max_kp3d_29_dropped", "no_valid", "px")
_px_case("gate_px_eq_doubled_max_kp3d_10_kept", 4.5, 10, "matched", 4.0)


def _shared_case(name, m_kfs, k_kf, end):
    """the keypoint's map point is also observed in keyframe k_kf (without error): a candidate unless the local point is observed there too"""
    m = MapBuilder(n_kf=5)
    M = m.local_point(320.0, 240.0, kfs=m_kfs)
    K = m.keypoint(321.0, 240.0, also=[(k_kf, m.proj(m.rows[M]["X"], k_kf))])
    ok = end == "matched"
    return _case(name, "gate", m, [M], {0: dict(end=end, total=1, shared_kf=0 if ok else 1, nvalid=1 if ok else 0)}, {K: M} if ok else {})


_shared_case("gate_shared_kf_first_of_list", (0, 1, 2), 0, "no_valid")
_shared_case("gate_shared_kf_last_of_list", (0, 1, 2), 2, "no_valid")
_shared_case("gate_shared_kf_only_entry", (1,), 1, "no_valid")
_shared_case("gate_no_shared_kf_list_of_three", (0, 1, 2), 3, "matched")
_shared_case("gate_no_shared_kf_list_of_one", (1,), 3, "matched")
for d in ("gate_shared_kf_first_of_list", "gate_shared_kf_last_of_list"):
    _twin("gate_no_shared_kf_list_of_three", d, "no_valid", "shared_kf")
_twin("gate_no_shared_kf_list_of_one", "gate_shared_kf_only_entry", "no_valid", "shared_kf")


def _coproj_case(name, kx0, end):
    """The keypoint's map point is seen in the frame 1.0 px from the local point's projection, and in keyframe 0 -- where the local point
    projects to exactly (1, 240) -- at (kx0, 240): errors 1.0 and kx0 - 1, mean (1 + (kx0 - 1)) / 2 in floats."""
    m = MapBuilder(n_kf=3, kf_t=[(-319.0 / 512.0, 0.0, 0.0), (0.125, 0.0, 0.0)])
    M = m.local_point(320.0, 240.0, kfs=(1,))
    assert m.proj(m.rows[M]["X"], 0) == (F32(1.0), F32(240.0))
    K = m.keypoint(321.0, 240.0, also=[(0, (kx0, 240.0))])
    ok = end == "matched"
    co = F32(np.float64(F32(0.0)) + np.float64(_pxdist(321.0, 240.0, 320.0, 240.0)))
    co = F32(np.float64(co) + np.float64(_pxdist(kx0, 240.0, 1.0, 240.0)))
    return _case(name, "gate", m, [M], {0: dict(end=end, total=1, coproj=0 if ok else 1, nvalid=1 if ok else 0)}, {K: M} if ok else {},
                 exact=dict(meanCoProj=(co / F32(2.0), F32(2.0) if ok else _up(2.0))))


_coproj_case("gate_coproj_mean_eq_max_errors_1_and_3_kept", 4.0, "matched")
_coproj_case("gate_coproj_mean_next_float_dropped", _up(4.0), "no_valid")
_twin("gate_coproj_mean_eq_max_errors_1_and_3_kept", "gate_coproj_mean_next_float_dropped", "no_valid", "coproj")


def _flag_case(name, end, gate, k_has_desc=1, m_flagged=True, m_bits=(0,), k_bits=0, k_flagged=True, flags=None):
    m = MapBuilder(n_kf=3)
    M = m.local_point(320.0, 240.0, kfs=tuple(range(len(m_bits))), descs=[desc_bits(b) for b in m_bits], flagged=m_flagged)
    K = m.keypoint(321.0, 240.0, bits=k_bits, has_desc=k_has_desc, flagged=k_flagged)
    ok = end == "matched"
    claim = dict(end=end, total=1, nvalid=1 if ok else 0)
    if gate:
        claim[gate] = 1
    return _case(name, "gate", m, [M], {0: claim}, {K: M} if ok else {}, flags=flags)


_flag_case("gate_keypoint_map_point_without_desc", "no_valid", "kp_nodesc", k_has_desc=0)
_flag_case("gate_keypoint_map_point_with_desc", "matched", None, flags=True)
_twin("gate_keypoint_map_point_with_desc", "gate_keypoint_map_point_without_desc", "no_valid", "kp_nodesc")
_flag_case("gate_all_descriptor_pairs_unflagged_distance_1000", "no_valid", "desc", m_flagged=False)
_flag_case("gate_keypoint_observation_unflagged_distance_1000", "no_valid", "desc", k_flagged=False)
# the local point's unflagged observation is identical to the keypoint's descriptor; the flagged one is 60 bits away
_flag_case("gate_unflagged_observation_would_give_minimum", "no_valid", "desc", m_bits=(0, 60), m_flagged=[False, True])
_flag_case("gate_same_observations_all_flagged", "matched", None, m_bits=(0, 60), flags=True)
_twin("gate_same_observations_all_flagged", "gate_unflagged_observation_would_give_minimum", "no_valid", "desc")


# ---------------------------------------------------------------------------------------- descriptor threshold and ratio test
def _dist_case(name, dists, end, best=None, ratio=0.2):
    """keypoints at the listed descriptor distances, all within the pixel gate, in scan order"""
    m = MapBuilder()
    M = m.local_point(320.0, 240.0)
    K = [m.keypoint(321.0, 240.0 + 0.25 * i, bits=d) for i, d in enumerate(dists)]
    min_dist = F32(32 * F32(ratio) * 8.)
    nvalid = sum(1 for d in dists if F32(d) <= min_dist)
    claim = dict(end=end, total=len(dists), nvalid=nvalid, desc=len(dists) - nvalid)
    if best is not None:
        claim.update(best_pos=best, best_dist=float(dists[best]))
    return _case(name, "ratio" if len(dists) > 1 else "desc", m, [M], {0: claim}, {K[best]: M} if end == "matched" else {},
                 exact=dict(minDist=(min_dist, F32(64.0))) if ratio == 0.25 else None, dist_ratio=ratio)


_dist_case("desc_ratio_0p25_dist_64_eq_min_valid", [64], "matched", 0, ratio=0.25)
_dist_case("desc_ratio_0p25_dist_65_invalid", [65], "no_valid", ratio=0.25)
_twin("desc_ratio_0p25_dist_64_eq_min_valid", "desc_ratio_0p25_dist_65_invalid", "no_valid", "desc")
_dist_case("desc_default_dist_51_valid", [51], "matched", 0)
_dist_case("desc_default_dist_52_invalid", [52], "no_valid")
_twin("desc_default_dist_51_valid", "desc_default_dist_52_invalid", "no_valid", "desc")
_dist_case("ratio_single_valid_dist_50_no_test_applies", [50], "matched", 0)
_dist_case("ratio_single_valid_beside_invalid_no_test_applies", [60, 50, 70], "matched", 1)
_dist_case("ratio_9_10_kept", [10, 9], "matched", 1)
_dist_case("ratio_18_20_kept", [18, 20], "matched", 0)
_dist_case("ratio_19_20_dropped", [19, 20], "ratio_reject", 0)
_twin("ratio_18_20_kept", "ratio_19_20_dropped", "ratio_reject")
_dist_case("ratio_9_9_dropped", [9, 9], "ratio_reject", 1)
_dist_case("ratio_0_0_kept_later_wins", [0, 0], "matched", 1)
_dist_case("ratio_second_eq_min_dist_57_64_kept", [57, 64], "matched", 0, ratio=0.25)
_dist_case("ratio_second_eq_min_dist_58_64_dropped", [58, 64], "ratio_reject", 0, ratio=0.25)
_twin("ratio_second_eq_min_dist_57_64_kept", "ratio_second_eq_min_dist_58_64_dropped", "ratio_reject")
_dist_case("ratio_second_past_min_dist_58_65_single_valid_kept", [58, 65], "matched", 0, ratio=0.25)


# ------------------------------------------------------------------------------------------------------------------ arbitration
def _arb_map(dists):
    """local points that all claim ONE keypoint, at the given descriptor distances"""
    m = MapBuilder()
    Ms = [m.local_point(320.0 + 0.5 * i, 240.0, bits=d) for i, d in enumerate(dists)]
    K = m.keypoint(321.0, 240.5, bits=0)
    fill = [m.filler() for _ in range(12)]
    return m, Ms, K, fill


def _arb(name, dists, positions, n_local, winner, reverse=False):
    m, Ms, K, fill = _arb_map(dists)
    local = [fill[i] for i in range(n_local)]
    for M, p in zip(Ms, positions):
        local[p] = M
    if reverse:
        local = local[::-1]
    claims = {li: dict(end="matched" if r == Ms[winner] else "lost_arbitration", total=1, nvalid=1) for li, r in enumerate(local) if r in Ms}
    return _case(name, "arbitration", m, local, claims, {K: Ms[winner]})


_arb("arb_two_claims_5_5_same_workgroup_later_wins", (5, 5), (0, 1), 2, 1)
_arb("arb_two_claims_5_5_reversed_list", (5, 5), (0, 1), 2, 0, reverse=True)
_arb("arb_5_5_7_same_workgroup", (5, 5, 7), (0, 1, 2), 3, 1)
_arb("arb_5_5_7_reversed_list_moves_winner", (5, 5, 7), (0, 1, 2), 3, 0, reverse=True)
_arb("arb_7_5_5_same_workgroup", (7, 5, 5), (0, 1, 2), 3, 2)
_arb("arb_5_7_5_same_workgroup", (5, 7, 5), (0, 1, 2), 3, 2)
_arb("arb_5_5_7_different_workgroups", (5, 5, 7), (0, 5, 9), 10, 1)
_arb("arb_5_5_7_different_workgroups_reversed_list", (5, 5, 7), (0, 5, 9), 10, 0, reverse=True)
_arb("arb_7_5_5_different_workgroups", (7, 5, 5), (1, 4, 11), 12, 2)
_arb("arb_5_7_5_different_workgroups", (5, 7, 5), (3, 4, 8), 9, 2)
_arb("arb_smaller_distance_beats_later_position", (5, 7), (0, 7), 8, 0)


# ------------------------------------------------------------------------------------------------------------------------ sizes
def _size_local(n_local):
    m = MapBuilder()
    Ms = [m.local_point(100.0 + 40.0 * i, 240.0) for i in range(5)]
    Ks = [m.keypoint(101.0 + 40.0 * i, 240.0) for i in range(5)]
    claims = {li: dict(end="matched", nvalid=1) for li in range(n_local)}
    return _case(f"size_n_local_{n_local}", "size", m, Ms[:n_local], claims, {Ks[i]: Ms[i] for i in range(n_local)}, scan=n_local > 0)


for n in (0, 1, 3, 4, 5):
    _size_local(n)


def _size_mp(n_mp):
    """the local point is row 0 and the keypoint the LAST row, so the per-row kernels' last block decides the result"""
    m = MapBuilder()
    if n_mp == 1:     # the one row is the frame's one keypoint and the one local point: observed, nothing to match
        K = m.keypoint(321.0, 240.0)
        return _case("size_n_mp_1", "size", m, [K], {0: dict(end="observed")}, {}, scan=False)
    M = m.local_point(320.0, 240.0)
    for _ in range(n_mp - 2):
        m.filler()
    K = m.keypoint(321.0, 240.0)
    assert K == n_mp - 1
    return _case(f"size_n_mp_{n_mp}", "size", m, [M], {0: dict(end="matched", total=1)}, {K: M})


for n in (1, 255, 256, 257):
    _size_mp(n)


# ------------------------------------------------------------------------------------------------------------ record form only
def _rec_40_entries():
    """a record with MP_ENT_CAP = 40 entries of which 38 are kept (one names a keyframe outside the table, one lacks the holds-the-keypoint
    flag), in a keyframe table at its limit of 64"""
    m = MapBuilder(n_kf=64, kf_t=[(k / 256.0, -0.0625, 0.0) for k in range(63)])
    M = m.local_point(320.0, 240.0, kfs=tuple(range(38)), descs=[desc_bits(3 + (k % 5), byte0=8) for k in range(38)])
    K = m.keypoint(321.0, 240.0, desc=desc_bits(3, byte0=8), also=[(50, m.proj(m.rows[M]["X"], 50))])
    extra = {M: [(3, 7, (5.0, 5.0)), (10 + 40, 1, (9.0, 9.0))]}
    return _case("rec_40_entries_38_kept_kf_table_64", "records", m, [M], {0: dict(end="matched", total=1, nvalid=1, best_dist=0.0)}, {K: M},
                 only="records", rec=dict(extras=False, extra_ents=extra))


_rec_40_entries()


def _rec_slots():
    m = MapBuilder()
    Ms = [m.local_point(100.0 + 40.0 * i, 240.0) for i in range(3)]
    Ks = [m.keypoint(101.0 + 40.0 * i, 240.0) for i in range(3)]
    # rows 0..5 -> slots on both sides of the chunk boundary
    return _case("rec_slots_4095_4096_two_chunks", "records", m, Ms, {li: dict(end="matched") for li in range(3)}, {Ks[i]: Ms[i] for i in range(3)},
                 only="records", rec=dict(slot_of=[4095, 4096, 7, 4097, 4094, 8191], n_slots=8192))


_rec_slots()


def _rec_holes():
    """Descriptor tables with history.  Keyframes 0..3 + the frame (4).
    pair A: the keypoint's table went add(kf 1) add(kf 2) add(frame) remove(kf 2): slot 1 is a FREE_KEY hole between two live slots and still
            holds the removed descriptor -- identical to the local point's.  The live ones are 60 bits away: no match.
    pair B: the same history with live distances (80, 10): matched at 10 through the slot BEHIND the hole.
    pair C: the local point's table went add(kf 0) add(kf 1) remove(kf 0) add(kf 2): the freed slot is taken again, so slot order (kf 2, kf 1)
            is not keyframe order; its removed descriptor was the keypoint's own."""
    m = MapBuilder(n_kf=5)
    ops = {}
    z, d10, d60, d80 = desc_bits(0), desc_bits(10), desc_bits(60), desc_bits(80)
    MA = m.local_point(100.0, 240.0, kfs=(0,), descs=[z])
    KA = m.add((0.25, 0.125, 4.0), [(1, m.proj(m.rows[MA]["X"], 1), d60, True), (4, (101.0, 240.0), d60, True)])
    ops[KA] = [(0, 11, d60), (0, 12, z), (0, 14, d60), (1, 12, None)]
    MB = m.local_point(200.0, 240.0, kfs=(0,), descs=[z])
    KB = m.add((0.25, 0.125, 4.0), [(1, m.proj(m.rows[MB]["X"], 1), d80, True), (4, (201.0, 240.0), d10, True)])
    ops[KB] = [(0, 11, d80), (0, 12, z), (0, 14, d10), (1, 12, None)]
    MC = m.local_point(300.0, 240.0, kfs=(1, 2), descs=[d60, d60])
    KC = m.keypoint(301.0, 240.0, desc=z)
    ops[MC] = [(0, 10, z), (0, 11, d60), (1, 10, None), (0, 12, d60)]
    return _case("rec_descriptor_tables_with_free_key_holes", "records", m, [MA, MB, MC],
                 {0: dict(end="no_valid", total=1, desc=1), 1: dict(end="matched", best_dist=10.0), 2: dict(end="no_valid", total=1, desc=1)},
                 {KB: MB}, only="records", rec=dict(desc_ops=ops))


_rec_holes()


def _rec_grid_entry():
    """The flat map is consistent; for the record form one MORE grid entry, at scan position 0, names a row whose record does not observe
    the frame (the other local point).  The expected result is the checker's on the flat map, i.e. with that entry removed."""
    m = MapBuilder()
    M = m.local_point(320.0, 240.0)
    other = m.local_point(100.0, 100.0)
    K = m.keypoint(321.0, 240.0)
    c = _case("rec_grid_entry_without_frame_obs", "records", m, [M, other], {0: dict(end="matched", total=1), 1: dict(end="no_valid", total=0)},
              {K: M}, only="records")
    aux = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c["aux"].items()}
    at = int(np.flatnonzero(aux["cell_kp"] == c["pb"]["mp_id"][K])[0])
    cell = int(np.searchsorted(aux["cell_ptr"], at, side="right") - 1)
    aux["cell_kp"] = np.insert(aux["cell_kp"], at, c["pb"]["mp_id"][other]).astype(np.int32)
    aux["cell_ptr"][cell + 1:] += 1
    c["rec"]["aux"] = aux
    return c


_rec_grid_entry()

BY_NAME = {c["name"]: c for c in CASES}
FLAT_CASES = [c for c in CASES if c["mhd"] is None and c["only"] is None]       # need no flags: all three entry forms, and the reference
FLAG_CASES = [c for c in CASES if c["only"] is None]
RECORD_CASES = list(CASES)


def expected_rows(case):
    """the case's stated result as match_of_mp [n_mp] (row indices, -1 elsewhere)"""
    out = np.full(len(case["pb"]["mp_id"]), -1, np.int32)
    for k, mrow in case["matches"].items():
        out[k] = mrow
    return out


def permuted(case, seed):
    """The same map with its rows in another order (ids, cells and local list unchanged, hence indices relabelled).  Returns (case', perm)
    with row i of case' = row perm[i] of case."""
    pb, n = case["pb"], len(case["pb"]["mp_id"])
    perm = np.random.RandomState(seed).permutation(n)
    q = dict(pb)
    cnt = np.diff(pb["obs_ptr"])[perm]
    q["obs_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    oi = np.concatenate([np.arange(pb["obs_ptr"][r], pb["obs_ptr"][r + 1]) for r in perm]).astype(np.int64)
    new_of_old = np.empty(len(oi), np.int64)
    new_of_old[oi] = np.arange(len(oi))
    for k in ("obs_kf", "obs_px", "obs_desc"):
        q[k] = np.ascontiguousarray(pb[k][oi])
    for k in ("mp_id", "mp_wpt", "mp_is3d"):
        q[k] = np.ascontiguousarray(pb[k][perm])
    q["frame_kp_order"] = new_of_old[pb["frame_kp_order"]].astype(np.int32)
    c = dict(case, pb=q, mhd=None if case["mhd"] is None else case["mhd"][perm], ohd=None if case["ohd"] is None else case["ohd"][oi])
    return c, perm


# ------------------------------------------------------------------------------------------------------- maps as records
def records_of(pb, shuffle_seed=0, slot_of=None, n_slots=None, mp_has_desc=None, obs_has_desc=None, extras=True, extra_ents=None, desc_ops=None,
               **_unused):
    """The flat map as map-point RECORDS (csrc/slam/mp_rec.hpp) in pinned chunks + the operations that fill the descriptor tables:
    row m -> a record slot (a permutation by default: slots are recycled in the product, rows and slots do not coincide; `slot_of` names
    them), an entry per observation {keyframe id, observed | holds-the-keypoint | has-a-descriptor, px}, plus -- like a live map has them
    -- entries the gather must drop.  extras=True adds to every 7th row an observer keyframe that is not in the keyframe table and to every
    11th an entry without the holds-the-keypoint flag; extra_ents = {row: [(keyframe id, flags, px)]} adds chosen ones.
    has_desc is mp_has_desc[m] (default: the row has observations); the row's descriptor table gets one add per observation flagged in
    obs_has_desc (default: all), or the operations desc_ops[row] = [(op, keyframe id, desc32 | None)] (capi.MedoidStore)."""
    import torch
    from alvaar_amd.capi import Context
    dt = Context.mp_record_dtype()
    n_mp = len(pb["mp_id"])
    if slot_of is None:
        n_slots = n_mp + 500 if n_slots is None else n_slots
        slot_of = np.random.RandomState(shuffle_seed).permutation(n_slots)[:n_mp].astype(np.int32)
    else:
        slot_of = np.asarray(slot_of, np.int32)
        assert len(slot_of) == n_mp and len(set(slot_of.tolist())) == n_mp and n_slots > int(slot_of.max())
    n_chunks = (n_slots + 4095) // 4096
    chunks = [torch.zeros(4096 * dt.itemsize, dtype=torch.uint8).pin_memory() for _ in range(n_chunks)]
    views = [c.numpy().view(dt) for c in chunks]
    ops = []
    kf_id = pb["kf_id"]
    for m in range(n_mp):
        s = int(slot_of[m])
        r = views[s >> 12][s & 4095]
        r["X"], r["id"], r["is3d"], r["observed"], r["dev_slot"], r["inv_depth"] = pb["mp_wpt"][m], pb["mp_id"][m], pb["mp_is3d"][m], 1, s, -1.0
        a, b = int(pb["obs_ptr"][m]), int(pb["obs_ptr"][m + 1])
        flagged = [obs_has_desc is None or bool(obs_has_desc[o]) for o in range(a, b)]
        ents = [(int(kf_id[pb["obs_kf"][o]]), 7 if flagged[o - a] else 3, pb["obs_px"][o]) for o in range(a, b)]
        if extras and m % 7 == 0:
            ents.append((3, 1 | 2 | 4, np.array([5.0, 5.0], np.float32)))          # keyframe 3 is not in the table (ids start at 10)
        if extras and m % 11 == 0:   # observed-by without a keypoint, in a keyframe of the table that does not observe the point otherwise
            free = [int(k) for k in kf_id[:-1] if int(k) not in {e[0] for e in ents}]
            if free:
                ents.append((free[0], 1, np.array([9.0, 9.0], np.float32)))
        for kf, fl, px in (extra_ents or {}).get(m, ()):
            ents.append((int(kf), int(fl), np.asarray(px, np.float32)))
        ents.sort(key=lambda e: e[0])
        assert len(ents) <= Context.MP_ENT_CAP and len({e[0] for e in ents}) == len(ents)
        r["n_ent"], r["n_obs"], r["has_desc"] = len(ents), len(ents), (1 if b > a else 0) if mp_has_desc is None else int(mp_has_desc[m])
        for i, (kf, fl, px) in enumerate(ents):
            r["ent"][i]["kf"], r["ent"][i]["flags"], r["ent"][i]["px"] = kf, fl, px
        ops.append((s, 3, -1, None, 0))
        if desc_ops is not None and m in desc_ops:
            for op, kf, d in desc_ops[m]:
                ops.append((s, int(op), int(kf), d, 0))
        else:
            for o in range(a, b):
                if flagged[o - a]:
                    ops.append((s, 0, int(kf_id[pb["obs_kf"][o]]), pb["obs_desc"][o], 0))
    table = torch.tensor([c.data_ptr() for c in chunks], dtype=torch.int64).cuda()
    return chunks, table, slot_of, ops, n_slots
