"""The light estimation stages (alva_light_bin, alva_light_fuse, alva_light_estimate) on the GPU against their numpy restatement
tests/light_cases.py: accumulators, state and every output are EQUAL, bit for bit.  Both sides do the same IEEE operations in the same
order and every other sum is an integer sum, so there is no tolerance.  The shapes are the smallest that reach each way of going wrong:
one block row, strips the grid cuts off, padded and unaligned rows, several workgroups adding into the same cells, all six faces, a block
centre exactly on a cell boundary and on the |x| = |y| tie, the largest and the smallest sums."""
from __future__ import annotations

import numpy as np
import pytest

import light_cases as Lc

pytestmark = pytest.mark.gpu

H45 = 0.7071067811865476


def _frame(rgba, pad_px=0):
    """the frame on the device in rows of (width + pad_px) pixels; the padding is saturated white, which no sum may contain"""
    import torch
    h, w = rgba.shape[:2]
    buf = torch.full((h, w + pad_px, 4), 255, dtype=torch.uint8, device="cuda")
    buf[:, :w] = torch.from_numpy(np.ascontiguousarray(rgba)).cuda()
    return buf[:, :w]


def _random(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _calib(w, h, f=None, cx=None, cy=None, dist=(0.0, 0.0, 0.0, 0.0)):
    f = 0.6 * w if f is None else f
    return (f, f * 1.01, w / 2 + 0.3 if cx is None else cx, h / 2 - 0.2 if cy is None else cy) + tuple(dist)


def _bin_equal(ctx, rgba, calib, R, step, pad_px=0, acc=None, want=None):
    got = ctx.light_bin(_frame(rgba, pad_px), calib, R, step, acc=acc)
    want = Lc.bin_frame(rgba, calib, R, step, acc=want)
    g = got.cpu().numpy().view(np.uint64)
    bad = np.nonzero(g != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), g[bad[:8]].tolist(), want[bad[:8]].tolist())
    return got, want


SIX = {"+x": Lc.rot_y(90), "-x": Lc.rot_y(-90), "+y": Lc.rot_x(-90), "-y": Lc.rot_x(90), "+z": np.eye(3), "-z": Lc.rot_y(180)}


@pytest.mark.parametrize("step", [2, 4, 16])
def test_bin_one_block_row_per_step(ctx, step):
    rgba = _random(16, 32, 10 + step)
    _, want = _bin_equal(ctx, rgba, _calib(32, 16), (Lc.rot_y(25) @ Lc.rot_x(-10)).reshape(-1), step)
    assert int(want[Lc.FRAME + 5]) == (32 // step) * (16 // step) and want[:Lc.FRAME].any()


def test_bin_cut_off_strips_and_padded_rows(ctx):
    rgba = _random(20, 36, 21)
    rgba[16:] = 255
    rgba[:, 32:] = 255                      # the strips right of and below the 2 x 1 grid: reading them would show in every sum
    R = Lc.rot_x(15).reshape(-1)
    _, want = _bin_equal(ctx, rgba, _calib(36, 20), R, 16)
    assert int(want[Lc.FRAME + 3]) == 512
    for pad in (4, 1, 3):                   # rows of 16-byte multiples, and rows whose start is only 4-byte aligned (no wide loads)
        _bin_equal(ctx, rgba, _calib(36, 20), R, 16, pad_px=pad)
        _bin_equal(ctx, _random(20, 36, 22), _calib(36, 20), R, 4, pad_px=pad)
        _bin_equal(ctx, _random(21, 37, 23), _calib(37, 21), R, 3, pad_px=pad)


def test_bin_several_workgroups_add_into_the_same_cells(ctx):
    rgba = _random(64, 256, 31)
    calib = _calib(256, 64, f=900.0)        # 16 degrees wide: 4 x 4 workgroups, a handful of cells
    _, want = _bin_equal(ctx, rgba, calib, Lc.rot_y(33).reshape(-1), 2)
    cells = want[:Lc.FRAME].reshape(-1, 4)
    assert 0 < (cells[:, 3] > 0).sum() <= 12 and int(cells[:, 3].max()) > 64 * 64   # more pixels than any one workgroup sees


def test_bin_all_six_faces_and_non_finite_directions(ctx):
    rgba = _random(48, 64, 41)
    calib = _calib(64, 48, f=30.0)
    for name, R in SIX.items():
        _, want = _bin_equal(ctx, rgba, calib, (R @ Lc.rot_x(7)).reshape(-1), 4)
        counts = want[:Lc.FRAME].reshape(6, 64, 4)[:, :, 3].sum(axis=1)
        assert counts.argmax() == list(SIX).index(name), (name, counts.tolist())
    R = Lc.rot_y(40)
    R[1, 0] = np.nan                        # every block's y is NaN: no cell, the frame's sums as ever
    _, want = _bin_equal(ctx, rgba, calib, R.reshape(-1), 4)
    assert not want[:Lc.FRAME].any() and int(want[Lc.FRAME + 3]) == 64 * 48
    _, want = _bin_equal(ctx, rgba, calib, np.zeros(9), 4)   # a zero direction joins no cell either
    assert not want[:Lc.FRAME].any()


def test_bin_cell_boundary_and_axis_tie(ctx):
    rgba = _random(16, 32, 51)
    # the principal point on the centre of block (4, 2) at step 4: a = b = 0 exactly, the boundary between cells 3 and 4
    calib = (40.0, 40.0, 18.0, 10.0, 0.0, 0.0, 0.0, 0.0)
    cell, dw = Lc.block_cells(calib, np.eye(3).reshape(-1), 4, 8, 4)
    assert dw[0][2, 4] == 0.0 and dw[1][2, 4] == 0.0 and cell[2, 4] == (4 * 8 + 4) * 8 + 4
    _bin_equal(ctx, rgba, calib, np.eye(3).reshape(-1), 4)
    # that block's direction on the |x| = |y| tie (x wins, a = 1 is clamped into the last cell), and on the |x| = |z| tie
    for R in (np.array([[H45, 0, H45], [-H45, 0, H45], [0, -1, 0]]), np.array([[H45, 0, H45], [0, 1, 0], [-H45, 0, H45]])):
        cell, dw = Lc.block_cells(calib, R.reshape(-1), 4, 8, 4)
        assert abs(dw[0][2, 4]) == max(abs(dw[1][2, 4]), abs(dw[2][2, 4])) and cell[2, 4] // 64 == 0
        _bin_equal(ctx, rgba, calib, R.reshape(-1), 4)


def test_bin_extreme_frames_no_rotation_distortion_and_consecutive_bins(ctx):
    white = np.full((64, 256, 4), 255, np.uint8)
    calib = _calib(256, 64, f=900.0)
    _, want = _bin_equal(ctx, white, calib, np.eye(3).reshape(-1), 2)
    assert int(want[Lc.FRAME]) == 65535 * 256 * 64 and int(want[Lc.FRAME + 4]) == 256 * 64
    _, want = _bin_equal(ctx, np.zeros((16, 32, 4), np.uint8), _calib(32, 16), np.eye(3).reshape(-1), 4)
    assert not want[Lc.FRAME:Lc.FRAME + 3].any() and int(want[Lc.FRAME + 3]) == 512 and want[3:Lc.FRAME:4].any()
    rgba = _random(48, 64, 61)
    _, want = _bin_equal(ctx, rgba, _calib(64, 48), None, 4)
    assert not want[:Lc.FRAME].any() and want[Lc.FRAME:].any()
    dist = _calib(64, 48, f=40.0, dist=(-0.28, 0.09, 0.002, -0.001))
    _bin_equal(ctx, rgba, dist, Lc.rot_y(-20).reshape(-1), 4)
    plain = Lc.block_cells(_calib(64, 48, f=40.0), Lc.rot_y(-20).reshape(-1), 4, 16, 12)[0]
    assert (Lc.block_cells(dist, Lc.rot_y(-20).reshape(-1), 4, 16, 12)[0] != plain).any()   # the distortion moves blocks between cells
    # two bins without a fuse in between add up
    got, want = _bin_equal(ctx, rgba, dist, Lc.rot_y(-20).reshape(-1), 4)
    got, want = _bin_equal(ctx, _random(48, 64, 62), dist, Lc.rot_y(10).reshape(-1), 4, acc=got, want=want)
    assert int(want[Lc.FRAME + 5]) == 2 * 16 * 12


def _acc(entries, frame=(0, 0, 0, 0, 0, 0)):
    acc = np.zeros(Lc.ACC_WORDS, np.uint64)
    for c, (sr, sg, sb, n) in entries.items():
        acc[4 * c:4 * c + 4] = [sr, sg, sb, n]
    acc[Lc.FRAME:Lc.FRAME + 6] = frame
    return acc


def _fuse_equal(ctx, acc, state_dev, state, **kw):
    import torch
    dev = torch.from_numpy(acc.view(np.int64).copy()).cuda()
    state_dev, was = ctx.light_fuse(dev, state_dev, want_acc=True, **kw)
    want = Lc.fuse(acc.copy(), state, **kw)
    assert np.array_equal(was.cpu().numpy().view(np.uint64), acc)
    assert not dev.cpu().numpy().any()                                   # zeroed for the next frame
    got = state_dev.cpu().numpy()
    bad = np.nonzero(got != Lc.pack_state(want))[0]
    assert bad.size == 0, bad[:8].tolist()
    return state_dev, want


def test_fuse_threshold_weights_and_counter(ctx):
    mp = Lc.MIN_PIXELS
    # n = min_pixels - 1 is touched but not observed; n = min_pixels is observed
    acc = _acc({7: (6553500, 100 * (mp - 1), 5 * (mp - 1), mp - 1), 8: (65535 * mp, 123 * mp + 17, 0, mp), 383: (1 << 40, 1 << 39, 3 << 38, 1 << 24)},
               frame=(10 * mp, 20 * mp, 30 * mp, mp, 3, 4))
    dev, st = _fuse_equal(ctx, acc, None, Lc.empty_state())
    assert st["W"][7] == 0 and st["W"][8] == Lc.W_NEW and st["E"][8].tolist() == [65535, 123, 0] and st["latch"].tolist() == [10, 20, 30, 3, 4, 3, 1, 1]
    # W goes 0 -> w_new -> ... -> w_max and stays, while the value moves towards each frame's mean
    seen = []
    for k in range(9):
        acc = _acc({8: ((1000 + 7000 * k) * mp + k, 50000 * mp, 3 * mp, mp)}, frame=(k, k, k, 1 + k, 0, 1))
        dev, st = _fuse_equal(ctx, acc, dev, st)
        seen.append(int(st["W"][8]))
    assert seen == [64, 96, 128, 160, 192, 224, 224, 224, 224] and st["latch"][6] == 10
    # a frame that observes no cell: the counter stays, the latch follows the frame; then a frame without pixels keeps the latch
    dev, st2 = _fuse_equal(ctx, _acc({9: (5, 5, 5, mp - 1)}, frame=(700, 800, 900, 10, 1, 2)), dev, st)
    assert st2["latch"][6] == 10 and st2["latch"][7] == st["latch"][7] + 1 and st2["latch"][:3].tolist() == [70, 80, 90]
    dev, st3 = _fuse_equal(ctx, _acc({}), dev, st2)
    assert np.array_equal(st3["latch"], st2["latch"])
    # other constants
    _fuse_equal(ctx, _acc({8: (999 * 5, 7 * 5, 0, 5)}, frame=(1, 2, 3, 5, 0, 1)), dev, st3, min_pixels=5, w_new=200, w_max=255)


def _estimate_equal(ctx, st):
    import torch
    got = ctx.light_estimate(torch.from_numpy(Lc.pack_state(st)).cuda())
    want = Lc.estimate(st)
    for name, g, w in zip(("sh", "primary_dir", "primary_rgb", "ambient"), got[:4], want[:4]):
        assert g.dtype == np.float32 and np.array_equal(g.reshape(-1).view(np.uint32), w.reshape(-1).view(np.uint32)), (name, g, w)
    assert np.array_equal(got[4], want[4]), (got[4], want[4])
    return want


def test_estimate_no_cell_one_cell_all_cells(ctx):
    st = Lc.empty_state()
    assert _estimate_equal(ctx, st)[4][0] == 5
    st["latch"][:] = [30000, 20000, 10000, 5, 19200, 0, 0, 3]
    sh, pd, pc, amb, info, L = _estimate_equal(ctx, st)
    assert info[0] == 1 and sh[0].all() and not sh[1:].any() and not pd.any() and amb[0] > 0
    st["E"][100] = [60000, 50000, 40000]
    st["W"][100] = 32
    sh, pd, pc, amb, info, L = _estimate_equal(ctx, st)            # one cell: the others take its value, a uniform environment
    assert info[0] == 0 and info[1] == 1 and info[6] == 0
    rng = np.random.default_rng(5)
    st["E"][:] = rng.integers(0, 65536, (Lc.CELLS, 3))
    st["W"][:] = rng.integers(1, 225, Lc.CELLS)
    st["latch"][1] = 0                                             # M_G = 0: the colour correction is (1, 1, 1)
    sh, pd, pc, amb, info, L = _estimate_equal(ctx, st)
    assert info[1] == Lc.CELLS and amb[1:].tolist() == [1.0, 1.0, 1.0]
    st["W"][::3] = 0                                               # a third of the cells filled with the mean of the others
    assert _estimate_equal(ctx, st)[4][1] == Lc.CELLS - 128


def test_estimate_uniform_environment_and_one_bright_cell_per_face(ctx):
    st = Lc.empty_state()
    st["E"][:] = [30000, 20000, 10000]
    st["W"][:] = 64
    sh, pd, pc, amb, info, L = _estimate_equal(ctx, st)
    assert info[6] == 0 and not pd.any() and not pc.any() and np.abs(sh[1:]).max() < 1e-6
    dirs = Lc.cell_dirs()
    for face in range(6):
        st = Lc.empty_state()
        st["E"][:] = 2000
        st["W"][:] = 32
        cell = (face * 8 + 2) * 8 + 5
        st["E"][cell] = [65535, 60000, 50000]
        sh, pd, pc, amb, info, L = _estimate_equal(ctx, st)
        axis = np.zeros(3)
        axis[face // 2] = -1.0 if face & 1 else 1.0
        assert info[6] == 1 and float(pd @ axis) > 0.5 and float(pd.astype(np.float64) @ dirs[cell]) > 0.999, (face, pd)
        assert abs(float(np.linalg.norm(pd.astype(np.float64))) - 1.0) < 1e-6 and (pc > 0).all()
