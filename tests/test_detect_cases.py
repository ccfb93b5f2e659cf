"""CPU: the grid detector's cases (tests/detect_cases.py).  The plain-C oracle is pinned to the compiled reference on every case -- the
point list bitwise with its order, the count, the new threshold -- and at every cell size the blur and lambda_min of single cells, so
that the oracle has the reference's authority wherever tests/test_gpu_detect_grid_cases.py compares the kernels with it.  The
conditions each case has to meet (non-empty, points at the image border, capacities below the count, ...) are asserted on the oracle's
result; the GPU tests assert them again."""
import numpy as np
import pytest

import detect_cases as D
from oracles import Orc, Ref


@pytest.mark.ref
@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_oracle_matches_reference(name):
    c = D.case(name)
    mq = c.max_quality
    for r in D.oracle_of(name):
        rp, rmq = Ref.detect_grid(c.gray, c.cell, c.occupied, c.roi, mq, cap=D.BIG_CAP)
        assert r["n"] == len(rp)
        assert r["max_quality"] == rmq
        assert np.array_equal(r["pts"].view(np.uint32), rp.view(np.uint32))
        mq = rmq
    if c.cap is not None:   # the capacity only cuts the list
        op, omq = Orc.detect_grid(c.gray, c.cell, c.occupied, c.roi, c.max_quality, cap=c.cap)
        rp, rmq = Ref.detect_grid(c.gray, c.cell, c.occupied, c.roi, c.max_quality, cap=c.cap)
        first = D.oracle_of(name)[0]
        assert omq == rmq == first["max_quality"] and len(op) == len(rp) == c.cap
        assert np.array_equal(op.view(np.uint32), rp.view(np.uint32)) and np.array_equal(op.view(np.uint32), first["pts"][:c.cap].view(np.uint32))


@pytest.mark.ref
@pytest.mark.parametrize("cell", D.CELLS)
def test_cell_blur_and_mineig_match_reference(cell):
    """single cells at every cell size, on the texture and on the low-entropy image (blur sums with acc & 15 == 8 in the vector columns
    and in the scalar tail, saturation): the first cell, an inner one, the last, and one at an offset that is no multiple of the cell"""
    w, h = D.dims(cell)
    nw, nh = D.grid_of(cell)
    halves = np.zeros(2, np.int64)
    for g in (D.texture(w, h, 100 + cell), D.low_entropy(w, h, 200 + cell)):
        for x, y in ((0, 0), (3 * cell, 2 * cell), ((nw - 1) * cell, (nh - 1) * cell), (cell + 1, cell + 3), (w - cell, h - cell)):
            ob, oe = Orc.cell_mineig(g, x, y, cell)
            rb, re_ = Ref.cell_mineig(g, x, y, cell)
            assert np.array_equal(ob, rb), (x, y)
            assert np.array_equal(oe.view(np.uint32), re_.view(np.uint32)), (x, y)
        halves += _half_sums(g, cell)
    assert halves[0] > 0 and (halves[1] > 0 or cell % 4 == 0)   # (no scalar tail when 4 divides the cell)


def _half_sums(g, cell):
    """pixels whose 3x3 blur sum is an odd multiple of 8 with an even quotient (there half-up and half-to-even differ), counted in the
    vector columns and in the scalar tail columns (x % cell >= cell & ~3) of a grid of cells from (0, 0)"""
    p = np.pad(g.astype(np.int32), 1, mode="reflect")
    k = np.array([1, 2, 1])
    acc = sum(k[j] * k[i] * p[j:j + g.shape[0], i:i + g.shape[1]] for j in range(3) for i in range(3))
    tail = (np.arange(g.shape[1]) % cell) >= (cell & ~3)
    differ = ((acc & 15) == 8) & (((acc >> 4) & 1) == 0)
    return np.array([differ[:, ~tail].sum(), differ[:, tail].sum()])


@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_case_conditions(name):
    D.check_conditions(name)


def test_cases_cover_what_they_are_meant_to():
    cells = {D.case(n).cell for n in D.CASE_NAMES}
    assert set(D.CELLS) <= cells and {c % 4 for c in cells} == {0, 1, 2, 3}
    for cell in D.SIZE_VARIANT_CELLS:   # the last column and row are skipped by the border rule
        for extra in (0, 1):
            c = D.case("low_c%d_plus%d" % (cell, extra))
            h, w = c.gray.shape
            assert w == cell * (w // cell) + extra and h == cell * (h // cell) + extra
            raw = D.oracle_of("low_c%d_plus%d" % (cell, extra))[0]["raw"]
            assert (raw[:, 0] < (w // cell - 1) * cell).all() and (raw[:, 1] < (h // cell - 1) * cell).all()
    # the three branches of the adaptive threshold, over three calls each
    got = {f for n in D.SEQUENCES for f in D.factors(n)}
    assert got == {0.5, 1.0, 1.5}
    for n in D.SEQUENCES:
        assert D.case(n).calls == 3 and len(D.oracle_of(n)) == 3
    # capacities: 0, 1, the primaries, one more, all but one
    for base, cell in (("roi_full_c8", 8), ("tex_c17", 17)):
        f = D.oracle_of(base)[0]
        caps = [D.case("cap_%s_c%d" % (t, cell)).cap for t in ("0", "1", "nprim", "nprim1", "nm1")]
        assert caps == [0, 1, f["n_primaries"], f["n_primaries"] + 1, f["n"] - 1] and len(set(caps)) == 5
    # ROIs: default, full, unaligned, cutting, empty
    for cell in (8, 7):
        h, w = D.case("roi_full_c%d" % cell).gray.shape
        assert D.case("roi_full_c%d" % cell).roi == (0, 0, w, h) and D.case("roi_default_c%d" % cell).roi == (20, 20, w - 40, h - 40)
        assert D.case("roi_empty_c%d" % cell).roi[2] == 0
        assert any(v % cell for v in D.case("roi_unaligned_c%d" % cell).roi)


def test_occupancy_edges_hold_what_the_docstring_says():
    for cell in (8, 7):
        c = D.case("occ_edges_c%d" % cell)
        h, w = c.gray.shape
        p = c.occupied
        nw, nh = w // cell, h // cell
        fx = p[:, 0] - np.floor(p[:, 0])
        assert ((p[:, 0] % cell == 0) & (p[:, 0] > 0)).any() and ((p[:, 1] % cell == 0) & (p[:, 1] > 0)).any()       # on a cell boundary
        half = p[fx == 0.5, 0]
        assert (np.floor(half) % 2 == 0).any() and (np.floor(half) % 2 == 1).any()                                     # .5, both parities
        assert (p == [0, 0]).all(1).any() and (p == [w - 1, h - 1]).all(1).any()                                       # corners
        assert (p[:, 0] >= nw * cell).any() and (p[:, 1] >= nh * cell).any()                                           # remainder strip
        assert len(np.unique(p, axis=0)) < len(p)                                                                      # duplicates
        assert (np.rint(p[:, 0]) >= w).any()                                                                           # centre outside the image
        below = np.nextafter(np.float32(cell), np.float32(0))
        assert (p[:, 0] == below).any() and int(below / np.float32(cell)) == 0                                         # one float below: cell 0
