"""TEST INFRASTRUCTURE: CLAHE cases for clahe.hip -- images whose tile histograms are designed so that the clipped excess has a chosen
batch (excess / 256) and residual (excess % 256), the grid and size edges, and a numpy count of what every tile's clip sees.
test_clahe_cases.py (CPU) asserts the residuals and edges the table claims; test_gpu_clahe_cases.py runs it on the GPU against the oracle.

The redistribution (clahe.cpp:185-212) adds `batch` to every bin and one more to the bins 0, step, 2 step, ... with step = max(256 / residual, 1),
`residual` of them at most: residual 1 touches bin 0 only, 100 has step 2 (256 / 100 truncates) and stops at bin 198, 128 has step 2 and
stops at bin 254, 129 and 255 have step 1 and stop at bins 128 and 254, 0 leaves the branch out although batch > 0."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id w h clip tiles build")

# ---- designed tiles ------------------------------------------------------------------------------------------------------------------
TILE = 32                      # 3 x 2 tiles of 32 x 32: 1024 pixels each
DESIGN_TILES = (3, 2)
DESIGN_CLIP = 4.0              # clipLimit = (int) (4.0 * 1024 / 256) = 16
DESIGN_LIMIT = 16
DESIGN = ((1, 0), (0, 1), (2, 100), (0, 128), (1, 129), (2, 255))    # (batch, residual) of the tiles, row-major
RESIDUALS = (0, 1, 100, 128, 129, 255)


def _designed_tile(batch, residual, value, rng):
    """1024 pixels: `value` DESIGN_LIMIT + 256 batch + residual times (the only clipped bin), the rest spread over the other 255 values, at
    most 4 of each; shuffled"""
    n = DESIGN_LIMIT + 256 * batch + residual
    others = np.array([v for v in range(256) if v != value], np.uint8)
    rest = others[rng.permutation(255)][np.arange(TILE * TILE - n) % 255]
    t = np.concatenate([np.full(n, value, np.uint8), rest])
    return t[rng.permutation(TILE * TILE)].reshape(TILE, TILE)


def designed(values, seed):
    rng = np.random.RandomState(seed)
    tx, ty = DESIGN_TILES
    g = np.zeros((ty * TILE, tx * TILE), np.uint8)
    for k, ((b, r), v) in enumerate(zip(DESIGN, values)):
        y, x = divmod(k, tx)
        g[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE] = _designed_tile(b, r, v, rng)
    return g


def palette(w, h, seed):
    """eight heavy grey levels with a scatter of others: tiles with several clipped bins and arbitrary residuals"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 8, (h, w)) * 30 + (rng.rand(h, w) < 0.3) * rng.randint(0, 30, (h, w))
    return np.ascontiguousarray(g.astype(np.uint8))


def reflect101(p, n):
    """(BORDER_REFLECT_101 of the indices p into a length n, how many passes that took)"""
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p), 0
    count = 0
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
        count += 1
    return p, count


def tile_stats(g, clip, tiles):
    """what the clip of every tile sees (clahe.cpp:364-384, :185-212): dict of the extended size, tile size, clipLimit, how many times the
    border had to be reflected, and per tile (row-major) the clipped excess, batch and residual"""
    h, w = g.shape
    tx, ty = tiles
    ew, eh = w, h
    if not (w % tx == 0 and h % ty == 0):
        ew, eh = w + (tx - w % tx), h + (ty - h % ty)
    tw, th = ew // tx, eh // ty
    total = tw * th
    limit = 0
    if clip > 0.0:
        limit = max(int(clip * total / 256), 1)
    (xs, rx), (ys, ry) = reflect101(np.arange(ew), w), reflect101(np.arange(eh), h)
    ext = g[np.ix_(ys, xs)]
    excess = []
    for k in range(tx * ty):
        y, x = divmod(k, tx)
        hist = np.bincount(ext[y * th:(y + 1) * th, x * tw:(x + 1) * tw].ravel(), minlength=256)
        excess.append(int(np.maximum(hist - limit, 0).sum()) if limit > 0 else 0)
    excess = np.array(excess)
    return dict(ew=ew, eh=eh, tw=tw, th=th, limit=limit, raw_limit=clip * total / 256, reflections=max(rx, ry), excess=excess, batch=excess // 256,
                residual=excess % 256)


CASES = (
    Case("designed-mid", 96, 64, DESIGN_CLIP, DESIGN_TILES, lambda: designed((90, 17, 200, 128, 61, 240), 1)),
    Case("designed-ends", 96, 64, DESIGN_CLIP, DESIGN_TILES, lambda: designed((0, 255, 0, 255, 1, 254), 2)),   # the clipped bin at either end of the histogram
    # grid and size edges: w x h, clip, tiles
    Case("5x3-t4x2", 5, 3, 3.0, (4, 2), lambda: palette(5, 3, 3)),            # extended to 8 x 4: tiles of 2 x 2
    Case("7x7-t7x7", 7, 7, 0.01, (7, 7), lambda: palette(7, 7, 4)),           # one-pixel tiles; clipLimit 0.00004 clamped up to 1
    Case("33x17-t8x8", 33, 17, 3.0, (8, 8), lambda: palette(33, 17, 5)),      # extended to 40 x 24
    Case("300x10-t1x10", 300, 10, 3.0, (1, 10), lambda: palette(300, 10, 6)),  # one-row tiles
    Case("17x16-t1x1", 17, 16, 2.0, (1, 1), lambda: palette(17, 16, 7)),      # one tile: every blend has both neighbours clamped
    Case("256x1-t3x1", 256, 1, 3.0, (3, 1), lambda: palette(256, 1, 8)),      # one row, extended to 258 x 2: reflect101 of length 1
    Case("64x48-clip1000", 64, 48, 1000.0, (4, 4), lambda: palette(64, 48, 9)),   # clipLimit 750 > 192 pixels: nothing clipped
    Case("64x48-clip0", 64, 48, 0.0, (4, 4), lambda: palette(64, 48, 10)),    # no clip at all
    Case("3x2-t8x5", 3, 2, 3.0, (8, 5), lambda: palette(3, 2, 11)),           # the padding exceeds the image: reflected more than once
    Case("320x240-t7x9", 320, 240, 3.0, (7, 9), lambda: palette(320, 240, 12)),   # the largest size here, not divisible either way
)
CASE_IDS = tuple(c.id for c in CASES)
GOLDEN_IDS = CASE_IDS[:-1]                   # the reference pin records all but the largest
PITCH_IDS = ("33x17-t8x8", "300x10-t1x10")   # run again from a pitched source and into a pitched destination (palette images: 255 is free)


def case(case_id):
    return next(c for c in CASES if c.id == case_id)


@functools.lru_cache(maxsize=None)
def image(case_id):
    c = case(case_id)
    g = np.ascontiguousarray(c.build())
    assert g.shape == (c.h, c.w) and g.dtype == np.uint8
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    from oracles import orc_clahe
    c = case(case_id)
    out = orc_clahe(image(case_id), c.clip, c.tiles)
    out.setflags(write=False)
    return out
