"""The grid detector's cases: what csrc/detect_grid.hip branches on, at the smallest sizes that still reach each branch.

A case is (gray, cell, occupied, roi, max_quality, cap) plus `calls` (the adaptive threshold is carried over that many calls) and
`expect`, the conditions its oracle result has to meet so that the GPU comparison cannot pass vacuously.  tests/test_detect_cases.py
pins the plain-C oracle to the compiled reference on every case and asserts the conditions; tests/test_gpu_detect_grid_cases.py compares
the kernels bitwise with the reference (the oracle where the reference is absent) and asserts the conditions again.

Everything is generated deterministically (numpy RandomState, the project's synth texture).  Images are about 24 x 18 cells (12 x 9 for
cells above 17), so a case costs a fraction of a second on the CPU."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from alvaar_amd import synth
from oracles import Orc, Ref, ref_available

Case = namedtuple("Case", "gray cell occupied roi max_quality cap calls expect")

# every cell size at which the kernels take another path:
#   4 .. 11  fewer than 64 (4 .. 7) or 128 entries per cell: less than one / two ballot chunks, radius 1 and 2, cand_stride padding
#   6, 14, 22   cell % 4 == 2;  5, 17, 33   % 4 == 1;  7, 11, 23, 39   % 4 == 3: the half-up tail of the blur is 2, 1, 3 columns wide
#   16 | 17  one wave | four waves per cell (n2 <= 256);  16 | 17, 22 | 23, 32 | 33: the sort pads to 256 | 512 | 1024 | 2048;  40 the maximum
CELLS = (4, 5, 6, 7, 8, 11, 14, 16, 17, 22, 23, 32, 33, 39, 40)
SIZE_VARIANT_CELLS = (7, 16, 40)   # w = cell * nw and cell * nw + 1: the rule x0 + cell < w - 1 skips the last column and row


def grid_of(cell):
    return (24, 18) if cell <= 17 else (12, 9)


def dims(cell, extra=2):
    nw, nh = grid_of(cell)
    return cell * nw + extra, cell * nh + extra


# ------------------------------------------------------------------------------------------------------------ images
def texture(w, h, seed):
    return synth.frame_gray(synth.texture_canvas(w, h, seed), 2, w, h, noise_seed=seed)


def low_entropy(w, h, seed, flat=True):
    """pixels from {0, 8, 255} with probabilities .45 / .45 / .1: blur sums with acc & 15 == 8 (the half-rounding split), equal lambda_min
    values inside a cell (the sort's index tie-break) and a saturated blur are all frequent.  Two additions: the outer 5 px are drawn
    from {0, 255} evenly, which puts the strongest corners of the border cells where the refinement window leaves the image, and a
    rectangle of about a ninth of the image, not aligned to the cells, is flat (unless flat=False), so that some cells find nothing and the
    top-up rule lets secondaries of the others through"""
    rng = np.random.RandomState(seed)
    g = rng.choice(np.array([0, 8, 255], np.uint8), size=(h, w), p=[0.45, 0.45, 0.10])
    ring = rng.choice(np.array([0, 255], np.uint8), size=(h, w))
    inner = np.zeros((h, w), bool)
    inner[5:h - 5, 5:w - 5] = True
    g = np.where(inner, g, ring)
    if flat:
        g[h // 3 + 1:2 * h // 3 - 2, w // 3 + 3:2 * w // 3 + 1] = 8
    return np.ascontiguousarray(g, np.uint8)


def periodic(w, h, period, seed, flat=False):
    """one random period x period tile repeated from (0, 0): the period divides the cell, so every cell away from the image border sees
    the same pixels, and inside a cell the pattern repeats"""
    tile = np.random.RandomState(seed).randint(0, 256, (period, period)).astype(np.uint8)
    g = np.tile(tile, (h // period + 1, w // period + 1))[:h, :w].copy()
    if flat:
        g[h // 3 + 1:2 * h // 3 - 2, w // 3 + 3:2 * w // 3 + 1] = 8
    return g


def constant(w, h, value=90):
    return np.full((h, w), value, np.uint8)


# ------------------------------------------------------------------------------------------------------------ occupancy
def _f32(pts):
    return np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 2), np.float32)


def occ_uniform(w, h, n, seed):
    rng = np.random.RandomState(seed)
    return _f32(np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1))


def occ_edges(w, h, cell):
    """points on the cell boundaries (k * cell, and half a pixel and one float either side of it: the float division px / cell decides
    the cell, cvRound(px) the circle's centre, half-to-even, with centres of both parities), the image's corners, circles the image border
    clips, a centre that rounds to outside the image, the strip right of and below the last full cell, and duplicates"""
    nw, nh = w // cell, h // cell
    pts = []
    for k in range(1, nw + 1):
        y = (k % nh) * cell + cell * 0.5 + 0.25
        for d in (-0.5, 0.0, 0.5):
            pts.append((k * cell + d, y))
        pts.append((np.nextafter(np.float32(k * cell), np.float32(0)), y + 1))
    for k in range(1, nh + 1):
        x = ((3 * k) % nw) * cell + cell * 0.5 - 0.25
        for d in (-0.5, 0.0, 0.5):
            pts.append((x, k * cell + d))
        pts.append((x + 1, np.nextafter(np.float32(k * cell), np.float32(0))))
    for k in range(1, min(nw, nh), 2):
        for d in (-0.5, 0.0, 0.5):
            pts.append((k * cell + d, k * cell + d))
    pts += [(2.5, 3.5), (3.5, 2.5), (10.5, 11.5), (11.5, 10.5), (0.5, 0.5), (1.5, 1.5)]        # .5 ties of both parities
    pts += [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1)]                                      # corners
    pts += [(1, h * 0.5), (w - 2, h * 0.25), (w * 0.5, 1.25), (w * 0.75, h - 1.75)]              # circles clipped by the border
    pts += [(w - 0.5, h - 0.5), (w - 0.75, 0.25)]                                                # inside [0, w) x [0, h); cvRound gives w, h
    for x in (nw * cell, nw * cell + 0.5, min(nw * cell + 1, w - 1)):                            # the remainder strip
        pts += [(x, cell * 1.5), (x, nh * cell + 0.5)]
    pts += [(cell * 2.5, nh * cell), (cell * 3.5, min(nh * cell + 1, h - 1))]
    pts += pts[3:40:5]                                                                           # duplicates
    pts = _f32(pts)
    assert (pts[:, 0] >= 0).all() and (pts[:, 0] < w).all() and (pts[:, 1] >= 0).all() and (pts[:, 1] < h).all()
    return pts


def occ_cells(cell, cells_rc):
    """one point at the centre of each listed cell (row, column); its circle (radius cell / 4) stays inside the cell"""
    return _f32([(c * cell + cell * 0.5, r * cell + cell * 0.5) for r, c in cells_rc])


# ------------------------------------------------------------------------------------------------------------ the cases
def _full(w, h):
    return (0, 0, w, h)


@functools.lru_cache(maxsize=None)
def _specs():
    """name -> (builder, expect).  The builder returns (gray, cell, occupied, roi, max_quality, cap spec, calls); a cap spec is None
    (room for everything) or a function of the first call's uncapped oracle result (its n and n_primaries)."""
    S = {}

    def add(name, build, **expect):
        assert name not in S
        S[name] = (build, expect)

    # ---- every cell class on both image families; w = cell * nw + 2, so no cell is skipped by the border rule
    for cell in CELLS:
        w, h = dims(cell)
        nw, nh = grid_of(cell)
        # texture, default ROI, a few tracked points.  0.001 is too high for small cells (the texture gives them nothing): 1e-5 there
        add("tex_c%d" % cell, lambda cell=cell, w=w, h=h, nw=nw, nh=nh: (
            texture(w, h, 100 + cell), cell, occ_uniform(w, h, nw * nh // 8, cell), None, 1e-5 if cell <= 11 else 1e-3, None, 1),
            nonempty=True)
        # low entropy, full ROI, nothing tracked, every cell fills: the image border is reached (k_subpix's border path)
        add("low_c%d" % cell, lambda cell=cell, w=w, h=h: (low_entropy(w, h, 200 + cell), cell, None, _full(w, h), 1e-7, None, 1),
            nonempty=True, border=10, has_secondaries=True)
    for cell in SIZE_VARIANT_CELLS:
        for extra in (0, 1):
            w, h = dims(cell, extra)
            add("low_c%d_plus%d" % (cell, extra), lambda cell=cell, w=w, h=h: (low_entropy(w, h, 200 + cell), cell, None, _full(w, h), 1e-7, None, 1),
                nonempty=True, fewer_primaries_than="low_c%d" % cell)

    # ---- exact ties across a whole cell, and nothing at all
    for cell, period in ((16, 4), (32, 8), (6, 3)):
        w, h = dims(cell)
        add("periodic_c%d" % cell, lambda cell=cell, w=w, h=h, period=period: (periodic(w, h, period, 300 + cell), cell, None, _full(w, h), 1e-7, None, 1),
            nonempty=True, tie=True)
    # the same position is picked in every cell, so a circle that reaches into the next cell starts a chain of repairs as long as the
    # grid: these are the cases that leave the one-workgroup finisher work to do (with tracked points: under the static mask)
    for cell, period in ((5, 5), (16, 4), (17, 17), (40, 8)):
        w, h = dims(cell)
        nw, nh = grid_of(cell)
        add("chain_c%d" % cell, lambda cell=cell, w=w, h=h, period=period: (periodic(w, h, period, 310 + cell), cell, None, _full(w, h), 1e-7, None, 1),
            nonempty=True)
        add("chain_occ_c%d" % cell, lambda cell=cell, w=w, h=h, period=period, nw=nw, nh=nh: (
            periodic(w, h, period, 310 + cell), cell, occ_uniform(w, h, nw * nh // 6, 320 + cell), _full(w, h), 1e-7, None, 1), nonempty=True)
    w16, h16 = dims(16)
    add("chain_flat_c16_q0", lambda: (periodic(w16, h16, 4, 326, flat=True), 16, occ_uniform(w16, h16, 60, 327), (0, 0, w16, h16 - 3 * 16), 0.0, None, 1),
        nonempty=True)
    w8, h8 = dims(8)
    add("constant_c8", lambda: (constant(w8, h8), 8, None, _full(w8, h8), 1e-3, None, 1), empty=True, factor=0.5)
    # lambda_min is 0 everywhere and 0 >= 0: the exact arg-max path reports pixel 0 of every cell twice (the second arg-max of an all-zero
    # product is its first element again).  The ROI rejects the last three rows of cells, so the top-up rule lets 72 of those through
    add("constant_c8_q0", lambda: (constant(w8, h8), 8, occ_uniform(w8, h8, 20, 8), (0, 0, w8, h8 - 3 * 8), 0.0, None, 1),
        nonempty=True, has_secondaries=True)

    # the same threshold on an image with a flat patch among strong corners: cells that must take the exact arg-max next to cells that
    # walk their sorted list, under tracked points
    add("low_c8_q0", lambda: (low_entropy(w8, h8, 208), 8, occ_uniform(w8, h8, 40, 61), (0, 0, w8, h8 - 3 * 8), 0.0, None, 1),
        nonempty=True, has_secondaries=True)

    # ---- ROIs, on one image each of cell 8 (even) and 7 (odd)
    for cell in (8, 7):
        w, h = dims(cell)
        img = lambda cell=cell, w=w, h=h: low_entropy(w, h, 400 + cell)
        occ = lambda cell=cell, w=w, h=h: occ_uniform(w, h, 30, 400 + cell)
        add("roi_full_c%d" % cell, lambda cell=cell, w=w, h=h, img=img, occ=occ: (img(), cell, occ(), _full(w, h), 1e-7, None, 1), nonempty=True, border=10)
        add("roi_default_c%d" % cell, lambda cell=cell, img=img, occ=occ: (img(), cell, occ(), None, 1e-7, None, 1),
            nonempty=True, fewer_primaries_than="roi_full_c%d" % cell)
        add("roi_unaligned_c%d" % cell, lambda cell=cell, w=w, h=h, img=img, occ=occ: (img(), cell, occ(), (3, 5, w - 9, h - 11), 1e-7, None, 1),
            nonempty=True, fewer_primaries_than="roi_full_c%d" % cell)
        # cuts through a row and a column of cells at mid-cell: about half of their primaries fall outside, and those cells must not
        # yield a secondary either
        add("roi_cut_c%d" % cell, lambda cell=cell, w=w, h=h, img=img, occ=occ: (
            img(), cell, occ(), (0, 0, 9 * cell + cell // 2, 7 * cell + cell // 2), 1e-7, None, 1),
            nonempty=True, fewer_than="roi_full_c%d" % cell, cut_rejects_whole_cells=True)
        add("roi_empty_c%d" % cell, lambda cell=cell, h=h, img=img, occ=occ: (img(), cell, occ(), (10, 10, 0, h - 20), 1e-7, None, 1),
            empty=True, factor=0.5)

    # ---- capacities below the number of points (n and n_primaries of the uncapped run)
    for cell, base in ((8, "roi_full_c8"), (17, "tex_c17")):
        for tag, spec in (("0", lambda first: 0), ("1", lambda first: 1), ("nprim", lambda first: first["n_primaries"]),
                          ("nprim1", lambda first: first["n_primaries"] + 1), ("nm1", lambda first: first["n"] - 1)):
            add("cap_%s_c%d" % (tag, cell), lambda base=base, spec=spec: _build(base)[:5] + (spec, 1), nonempty=True, capped=True)

    # ---- occupancy
    for cell in (8, 7):
        w, h = dims(cell)
        nw, nh = grid_of(cell)
        img = lambda cell=cell, w=w, h=h: low_entropy(w, h, 500 + cell)
        add("occ_edges_c%d" % cell, lambda cell=cell, w=w, h=h, img=img: (img(), cell, occ_edges(w, h, cell), _full(w, h), 1e-7, None, 1), nonempty=True)
        add("occ_many_c%d" % cell, lambda cell=cell, w=w, h=h, nw=nw, nh=nh, img=img: (
            img(), cell, occ_uniform(w, h, nw * nh + 70, 510 + cell), _full(w, h), 1e-7, None, 1), nonempty=True, more_points_than_cells=True)
        add("occ_all_c%d" % cell, lambda cell=cell, w=w, h=h, nw=nw, nh=nh, img=img: (
            img(), cell, occ_cells(cell, [(r, c) for r in range(nh) for c in range(nw)]), _full(w, h), 1e-7, None, 1),
            empty=True, factor=1.0, no_free_cells=True)
        # the ROI covers the cells 2 .. of every side; every cell it excludes is occupied, every other cell finds its primary: the
        # top-up rule then allows no secondary (total + occupied >= cells).  Beside it: without that occupancy, secondaries
        img = lambda cell=cell, w=w, h=h: low_entropy(w, h, 500 + cell, flat=False)
        roi = (2 * cell, 2 * cell, (nw - 4) * cell, (nh - 4) * cell)
        outside = [(r, c) for r in range(nh) for c in range(nw) if not (2 <= r < nh - 2 and 2 <= c < nw - 2)]
        add("zero_sec_c%d" % cell, lambda cell=cell, img=img, roi=roi, outside=tuple(outside): (img(), cell, occ_cells(cell, outside), roi, 1e-7, None, 1),
            nonempty=True, zero_secondaries=True)
        add("zero_sec_beside_c%d" % cell, lambda cell=cell, img=img, roi=roi: (img(), cell, None, roi, 1e-7, None, 1), nonempty=True, has_secondaries=True)

    # ---- three calls that carry the threshold over, one sequence per branch of the adaptive rule
    w, h = dims(8)
    add("seq_half_c8", lambda: (texture(w, h, 108), 8, occ_uniform(w, h, 40, 61), _full(w, h), 1e-2, None, 3), nonempty=True, factor=0.5)
    add("seq_same_c8", lambda: (texture(w, h, 108), 8, occ_uniform(w, h, 40, 61), _full(w, h), SEQ_SAME_START, None, 3), nonempty=True, factor=1.0)
    add("seq_up_c8", lambda: (low_entropy(w, h, 208), 8, occ_uniform(w, h, 40, 61), _full(w, h), 1e-7, None, 3), nonempty=True, factor=1.5)
    return S


SEQ_SAME_START = 1.5e-5   # the texture at cell 8: between 33 % and 90 % of the free cells


@functools.lru_cache(maxsize=None)
def _build(name):
    g, cell, occ, roi, mq, cap, calls = _specs()[name][0]()
    g = np.ascontiguousarray(g, np.uint8)
    g.setflags(write=False)
    h, w = g.shape
    if roi is None:
        roi = (20, 20, w - 40, h - 40)
    if occ is not None:
        occ.setflags(write=False)
    return g, cell, occ, tuple(int(v) for v in roi), float(mq), cap, calls


def names():
    return tuple(_specs())


CASE_NAMES = names()
SEQUENCES = tuple(n for n in CASE_NAMES if n.startswith("seq_"))
BIG_CAP = 20000


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """the plain-C oracle's result of every call of the case, UNCAPPED (a capacity only cuts the list; the count and the threshold do
    not depend on it): a tuple of Orc.detect_grid_ex dicts.  Computed once per process and shared: callers must not change it"""
    g, cell, occ, roi, mq, _, calls = _build(name)
    out = []
    for _ in range(calls):
        r = Orc.detect_grid_ex(g, cell, occ, roi, mq, cap=BIG_CAP)
        assert r["n"] <= BIG_CAP
        out.append(r)
        mq = r["max_quality"]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(name):
    g, cell, occ, roi, mq, cap, calls = _build(name)
    if cap is not None:
        cap = int(cap(oracle_of(name)[0]))
    return Case(g, cell, occ, roi, mq, cap, calls, dict(_specs()[name][1]))


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """what the kernels are compared with: per call (pts uncapped, new threshold), from the compiled reference where it is built, else
    from the oracle (which tests/test_detect_cases.py pins to the reference on every case).  Shared: callers must not change it"""
    if not ref_available():
        return tuple((r["pts"], r["max_quality"]) for r in oracle_of(name))
    g, cell, occ, roi, mq, _, calls = _build(name)
    out = []
    for _ in range(calls):
        pts, nmq = Ref.detect_grid(g, cell, occ, roi, mq, cap=BIG_CAP)
        out.append((pts, nmq))
        mq = nmq
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------ conditions
# full-ROI cases that detect, yet put fewer than 10 points where the refinement window leaves the image:
#   periodic_c32, chain_*   every cell holds the same pixels, so every cell picks the same in-cell position, and that is not at the cell's edge
#   seq_half_c8    the texture at a threshold that has to halve: about 40 points on the whole image
BORDER_EXEMPT = ("periodic_c32", "seq_half_c8") + tuple("chain%s_c%d" % (o, c) for o in ("", "_occ") for c in (5, 16, 17, 40))


def near_border(raw, w, h):
    """how many unrefined points have a 9x9 refinement window (getRectSubPix reads one column and row more) that leaves the image: these
    take k_subpix's border path in their first iteration.  All of them lie within 5 px of the border"""
    x, y = raw[:, 0], raw[:, 1]
    return int(((x < 4) | (x >= w - 5) | (y < 4) | (y >= h - 5)).sum())


def tied_cells(gray, cell):
    """number of cells (of those the border rule lets through) whose lambda_min has at least two equal positive maxima"""
    h, w = gray.shape
    n = 0
    for r in range(h // cell):
        for c in range(w // cell):
            if not (c * cell + cell < w - 1 and r * cell + cell < h - 1):
                continue
            _, e = Orc.cell_mineig(gray, c * cell, r * cell, cell)
            m = e.max()
            n += bool(m > 0 and (e == m).sum() >= 2)
    return n


def factors(name):
    """the factor each call of the case applies to the threshold"""
    mq = case(name).max_quality
    out = []
    for r in oracle_of(name):
        out.append(r["max_quality"] / mq if mq != 0 else 1.0)
        mq = r["max_quality"]
    return out


def check_conditions(name):
    """asserts what the case is meant to be, on the oracle's result.  Called on the CPU (tests/test_detect_cases.py) and again by the GPU
    test of the same case, so that neither can pass on an empty or degenerate result."""
    c, res = case(name), oracle_of(name)
    e, first = c.expect, oracle_of(name)[0]
    h, w = c.gray.shape
    nw, nh = w // c.cell, h // c.cell
    assert first["n_cells"] == nw * nh
    if c.occupied is not None:
        assert (c.occupied[:, 0] >= 0).all() and (c.occupied[:, 0] < w).all() and (c.occupied[:, 1] >= 0).all() and (c.occupied[:, 1] < h).all()
    if e.get("nonempty"):
        assert all(r["n"] > 0 for r in res), name
    if e.get("empty"):
        assert all(r["n"] == 0 for r in res), name
    if "border" in e or (e.get("nonempty") and c.roi == (0, 0, w, h) and name not in BORDER_EXEMPT):
        # every detecting case with the full-image ROI, in every call: k_subpix's border path is compared on at least 10 points
        for r in res:
            assert near_border(r["raw"], w, h) >= e.get("border", 10), (name, near_border(r["raw"], w, h))
    if "fewer_than" in e:
        assert first["n"] < oracle_of(e["fewer_than"])[0]["n"], name
    if "fewer_primaries_than" in e:   # (the top-up rule can fill the count up again with secondaries)
        assert first["n_primaries"] < oracle_of(e["fewer_primaries_than"])[0]["n_primaries"], name
    if e.get("capped"):
        assert 0 <= c.cap < first["n"], (name, c.cap, first["n"])
    if e.get("zero_secondaries"):
        assert first["n"] == first["n_primaries"] and first["n_primaries"] + first["n_occupied_cells"] >= first["n_cells"], (name, first)
        assert first["n_secondary_cells"] > 0   # the rule cuts them, the cells did find them
    if e.get("has_secondaries"):
        assert first["n"] > first["n_primaries"], name
    if e.get("more_points_than_cells"):
        assert len(c.occupied) > first["n_cells"] > first["n_occupied_cells"]
    if e.get("no_free_cells"):
        assert first["n_occupied_cells"] == first["n_cells"]
    if "factor" in e:   # in every call of a sequence
        assert factors(name) == [e["factor"]] * c.calls, (name, factors(name))
    if e.get("tie"):
        assert tied_cells(c.gray, c.cell) >= 1, name
    if e.get("cut_rejects_whole_cells"):
        # cells the ROI's edge runs through, which found a primary inside the uncut ROI's run but nothing at all here: their primary is
        # outside the ROI, and the cell is left without looking for a secondary
        full = oracle_of("roi_full_c%d" % c.cell)[0]
        x1, y1 = c.roi[0] + c.roi[2], c.roi[1] + c.roi[3]
        cut_cells = {(r, x1 // c.cell) for r in range(y1 // c.cell + 1)} | {(y1 // c.cell, col) for col in range(x1 // c.cell + 1)}
        cells_of = lambda raw: {(int(y) // c.cell, int(x) // c.cell) for x, y in raw}
        lost = (cells_of(full["raw"]) & cut_cells) - cells_of(first["raw"])
        assert len(lost) >= 3, (name, len(lost))
