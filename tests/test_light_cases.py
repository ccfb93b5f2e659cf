"""CPU: the numpy restatement of light estimation (tests/light_cases.py) against what it restates -- the committed table against the sRGB
curve, the whole chain (bin, fuse, estimate) against the analytic projection of a known environment, and the blend's properties.  The
kernels are compared with the restatement bit for bit in tests/test_gpu_light.py.

The bounds of the analytic test are twice the restatement's own worst errors over the three light directions (128 x 96 frames, 90 x 74
degrees, 28 rotations that cover the sphere, p = 4), measured when the test was written:
    direction 0.453 degrees; band 0: 0.00265, band 1: 0.00304, band 2: 0.00466 (absolute, with L00 about 0.64 - 0.71)."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import light_cases as Lc

ROOT = Path(__file__).resolve().parent.parent
MEASURED = dict(angle_deg=0.4533, band0=0.00265, band1=0.00304, band2=0.00466)


def test_table_is_the_srgb_curve_within_one_and_monotone():
    t = Lc.lut().astype(np.int64)
    want = 65535.0 * Lc.srgb_to_linear(np.arange(256) / 255.0)
    assert np.abs(t - want).max() <= 1.0
    assert t[0] == 0 and t[255] == 65535 and (np.diff(t) >= 0).all()


def test_header_defines_the_stages_and_the_constants():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    for step in ("B1", "B2", "B3", "B4", "B5", "F1", "F2", "F3", "E1", "E2", "E3", "E4", "E5"):
        assert re.search(r"\*\s+%s " % step, hip), step
    for name, value in (("ALVA_LIGHT_N", Lc.N), ("ALVA_LIGHT_CELLS", Lc.CELLS), ("ALVA_LIGHT_ACC_WORDS", Lc.ACC_WORDS),
                        ("ALVA_LIGHT_STATE_BYTES", Lc.STATE_BYTES)):
        assert re.search(r"#define %s %d\b" % (name, value), hip), name
    for name, value in (("ALVA_LIGHT_STEP", Lc.STEP), ("ALVA_LIGHT_MIN_PIXELS", Lc.MIN_PIXELS), ("ALVA_LIGHT_W_NEW", Lc.W_NEW),
                        ("ALVA_LIGHT_W_MAX", Lc.W_MAX)):
        assert re.search(r"#define %s %d\b" % (name, value), sysh), name
    assert "not photometric" in hip.lower() or "NOT photometric" in sysh
    assert "DISTANT" in hip and "DISTANT" in sysh


def test_cells_faces_ties_and_boundaries():
    # the six axes land in the middle of their faces: a = b = 0 is the boundary between cells 3 and 4, and belongs to 4
    for face, d in enumerate(([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])):
        assert Lc.cell_of(*map(float, d)) == (face * 8 + 4) * 8 + 4
    # ties: x before y before z
    assert Lc.cell_of(1.0, 1.0, 0.5) // 64 == 0 and Lc.cell_of(-1.0, 1.0, 1.0) // 64 == 1
    assert Lc.cell_of(0.5, 1.0, 1.0) // 64 == 2 and Lc.cell_of(0.5, -1.0, -1.0) // 64 == 3
    # a = +1 exactly is clamped into the last cell, a = -1 is the first
    c = int(Lc.cell_of(1.0, 1.0, -1.0))
    assert (c % 8, (c // 8) % 8) == (7, 0)
    # nothing for a non-finite or a zero direction
    assert Lc.cell_of(np.nan, 0.0, 1.0) == -1 and Lc.cell_of(np.inf, 0.0, 1.0) == -1 and Lc.cell_of(0.0, 0.0, 0.0) == -1
    # every cell centre maps to its own cell
    d = Lc.cell_dirs()
    assert np.array_equal(Lc.cell_of(d[:, 0], d[:, 1], d[:, 2]), np.arange(Lc.CELLS))


def test_basis_table_integrates_the_sphere():
    T = Lc.basis_table()
    assert abs(T[0].sum() - 4 * np.pi * 0.282095) < 1e-12
    assert np.abs(T[1:].sum(axis=1)).max() < 1e-12            # the cube's symmetry: every higher basis function integrates to zero
    # the quadrature of Y_k Y_k' is close to the identity (how well 384 cells carry second-order harmonics)
    d = Lc.cell_dirs()
    Y = np.array(Lc.sh_basis(d[:, 0], d[:, 1], d[:, 2]))
    G = (T / 1.0) @ Y.T
    print("largest deviation of the cube-map quadrature from orthonormality", np.abs(G - np.eye(9)).max())
    assert np.abs(G - np.eye(9)).max() < 0.02


def test_bin_sums_and_consecutive_bins_add():
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (20, 36, 4), dtype=np.uint8)
    calib = (30.0, 31.0, 17.5, 9.5, 0.0, 0.0, 0.0, 0.0)
    acc = Lc.bin_frame(rgba, calib, Lc.rot_y(20).reshape(-1), 4)
    cells = acc[:Lc.FRAME].reshape(-1, 4).astype(np.int64)
    lin = Lc.lut()[rgba[:20, :36, :3]].astype(np.int64)
    assert [int(v) for v in acc[Lc.FRAME:Lc.FRAME + 6]] == [lin[..., 0].sum(), lin[..., 1].sum(), lin[..., 2].sum(), 20 * 36,
                                                              int((rgba[..., :3] >= 250).any(axis=2).sum()), 5 * 9]
    assert cells.sum(axis=0).tolist() == [int(v) for v in acc[Lc.FRAME:Lc.FRAME + 4]]   # every block joined one cell
    no_R = Lc.bin_frame(rgba, calib, None, 4)
    assert not no_R[:Lc.FRAME].any() and np.array_equal(no_R[Lc.FRAME:], acc[Lc.FRAME:])
    twice = Lc.bin_frame(rgba, calib, Lc.rot_y(20).reshape(-1), 4, acc=acc.copy())
    assert np.array_equal(twice, 2 * acc)
    # the strips that the grid cuts off are not read: 36 x 20 at step 16 is 2 x 1 blocks
    acc16 = Lc.bin_frame(rgba, calib, None, 16)
    assert int(acc16[Lc.FRAME + 3]) == 2 * 256 and int(acc16[Lc.FRAME + 5]) == 2
    assert int(acc16[Lc.FRAME]) == lin[:16, :32, 0].sum()


@pytest.fixture(scope="module")
def sessions():
    Rs = Lc.sphere_rotations()
    return {name: Lc.run_session(Rs, l) for name, l in Lc.LIGHTS.items()}


def test_analytic_environment_direction_and_coefficients(sessions):
    worst = dict(angle_deg=0.0, band0=0.0, band1=0.0, band2=0.0)
    for name, l in Lc.LIGHTS.items():
        sh, pd, pc, amb, info, L = Lc.estimate(sessions[name])
        assert info[0] == 0 and info[1] == Lc.CELLS and info[6] == 1, (name, info)
        want = Lc.analytic_sh(l)
        err = np.abs(L - want)
        ang = float(np.degrees(np.arccos(np.clip(pd.astype(np.float64) @ l, -1.0, 1.0))))
        got = dict(angle_deg=ang, band0=float(err[0].max()), band1=float(err[1:4].max()), band2=float(err[4:].max()))
        print(name, got)
        for k, v in got.items():
            worst[k] = max(worst[k], v)
        assert np.array_equal(sh, L.astype(np.float32))
        # the primary light's intensity is the band-1 amplitude of b max(0, t)^p: b 2 pi / (p + 2)
        assert np.abs(pc.astype(np.float64) - Lc.ENV_B * 2 * np.pi / (Lc.ENV_P + 2)).max() < 2 * MEASURED["band1"] / 0.488603
    print("worst", worst)
    for k, v in worst.items():
        assert v <= 2 * MEASURED[k], (k, v)


def _look_at(l):
    z = Lc.unit(l)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = Lc.unit(np.cross(up, z))
    return np.stack([x, np.cross(z, x), z], axis=1)


def test_partial_coverage_one_rotation():
    """One frame that looks at the light.  The cells it does not see take the mean of those it does (E1), so the estimate's component along
    the view axis comes only from WHERE in the view the brightness sits: a light in view gives a direction inside the hemisphere seen; a
    light outside the view pulls the direction to the view's edge, not beyond it (nothing is extrapolated), which is why the frame here
    looks at the light."""
    for name, l in Lc.LIGHTS.items():
        R = _look_at(l)
        st = Lc.run_session([R], l)
        sh, pd, pc, amb, info, L = Lc.estimate(st)
        assert info[0] == 0 and 0 < info[1] < Lc.CELLS and info[5] == 1 and info[6] == 1, (name, info)
        assert info[2] >= info[1] and info[3] == (Lc.ENV_W // Lc.STEP) * (Lc.ENV_H // Lc.STEP)
        assert float(pd.astype(np.float64) @ R[:, 2]) > 0.0, (name, pd)
        assert (st["W"][st["W"] > 0] == Lc.W_NEW).all()


def _acc_for(cells, values, n=Lc.MIN_PIXELS):
    acc = np.zeros(Lc.ACC_WORDS, np.uint64)
    for c, v in zip(cells, values):
        acc[4 * c:4 * c + 3] = np.uint64(v) * np.uint64(n)
        acc[4 * c + 3] = n
    acc[Lc.FRAME:Lc.FRAME + 6] = [1000 * n, 2000 * n, 3000 * n, n, 7, 4]
    return acc


def test_fuse_weights_saturate_and_unobserved_cells_never_change():
    st = Lc.empty_state()
    seen = []
    for _ in range(10):
        st = Lc.fuse(_acc_for([5, 200], [40000, 100]), st)
        seen.append(int(st["W"][5]))
    assert seen == [32, 64, 96, 128, 160, 192, 224, 224, 224, 224]
    assert st["E"][5].tolist() == [40000] * 3 and st["E"][200].tolist() == [100] * 3
    assert st["latch"].tolist() == [1000, 2000, 3000, 7, 4, 2, 10, 10]
    # frames that observe other cells, or none: cells 5 and 200 keep value and weight
    before = (st["E"][[5, 200]].copy(), st["W"][[5, 200]].copy())
    for _ in range(5):
        st = Lc.fuse(_acc_for([6], [9]), st)
    st = Lc.fuse(_acc_for([5], [1], n=Lc.MIN_PIXELS - 1), st)          # too few pixels: touched, not observed
    assert np.array_equal(st["E"][[5, 200]], before[0]) and np.array_equal(st["W"][[5, 200]], before[1])
    assert st["latch"][6] == 15 and st["latch"][7] == 16 and st["latch"][5] == 1
    # a frame without pixels keeps the latch, and zeroes the accumulators like every fuse
    acc = np.zeros(Lc.ACC_WORDS, np.uint64)
    latch = st["latch"].copy()
    st = Lc.fuse(acc, st)
    assert np.array_equal(st["latch"], latch) and not acc.any()


def test_fuse_replaces_a_changed_environment_at_the_stated_rate():
    st = Lc.empty_state()
    for _ in range(8):
        st = Lc.fuse(_acc_for([17], [60000]), st)
    assert st["W"][17] == Lc.W_MAX and st["E"][17, 0] == 60000
    keep = Lc.W_MAX / (Lc.W_MAX + Lc.W_NEW)
    for target in (1000, 65535):
        gap = first = abs(int(st["E"][17, 0]) - target)
        for k in range(40):
            st = Lc.fuse(_acc_for([17], [target]), st)
            new_gap = abs(int(st["E"][17, 0]) - target)
            assert new_gap <= gap * keep + 1, (target, k, gap, new_gap)   # (+ 1: the integer division rounds down)
            gap = new_gap
        assert gap <= first * keep ** 40 + 1 / (1 - keep), (target, gap)   # the geometric series of the + 1


def test_estimate_codes_and_uniform_environment():
    st = Lc.empty_state()
    sh, pd, pc, amb, info, L = Lc.estimate(st)
    assert info.tolist() == [5, 0, 0, 0, 0, 0, 0, 0] and not sh.any() and amb.tolist() == [0.0, 1.0, 1.0, 1.0]
    st = Lc.fuse(Lc.bin_frame(Lc.render_env(np.eye(3), Lc.LIGHTS["oblique"]), Lc.ENV_CALIB, None, Lc.STEP), st)
    sh, pd, pc, amb, info, L = Lc.estimate(st)
    assert info[0] == 1 and info[1] == 0 and info[6] == 0 and not sh[1:].any() and not pd.any() and not pc.any()
    M = st["latch"][:3].astype(np.float64)
    assert np.allclose(sh[0], 0.282095 * 4 * np.pi * M / 65535.0, rtol=1e-6) and 0 < amb[0] < 1
    assert np.allclose(amb[1:], [M[0] / M[1], 1.0, M[2] / M[1]], rtol=1e-6)
    # a uniform environment has no direction: the higher bands are rounding only and the primary light is invalid
    st = Lc.empty_state()
    st["E"][:] = [30000, 20000, 10000]
    st["W"][:] = Lc.W_NEW
    sh, pd, pc, amb, info, L = Lc.estimate(st)
    assert info[0] == 0 and info[1] == Lc.CELLS and info[6] == 0 and not pd.any() and not pc.any()
    assert np.abs(L[1:]).max() < 1e-12 and np.allclose(L[0], 0.282095 * 4 * np.pi * np.array([30000, 20000, 10000]) / 65535.0, rtol=1e-12)
