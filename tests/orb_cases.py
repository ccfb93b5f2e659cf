"""TEST INFRASTRUCTURE: the ORB detector's cull cases -- images, a case table and a predictor of the counts that decide which branch of
orb.hip's culls a case takes.  test_orb_cases.py (CPU) asserts every case's condition from the predictor and the oracle;
test_gpu_orb_cases.py runs the same cases on the GPU against the same oracle results.

Per level l of the pyramid the detector keeps (orb.cpp:799-813, :885-960)
  n1   FAST corners at least 31 pixels inside the level,
  n2   of those, the ones with score >= the (2 n_l)-th largest (KeyPointsFilter::retainBest: ties at the cut are all kept),
  m    of those, the ones with Harris response >= the n_l-th largest (ties kept again): the level's keypoints,
where n_l is the level's share of nfeatures.  The constants below restate orb.hip's: cull_harris_body ranks in registers / LDS up to
RANK_CAP candidates and ROW_CAP rows, cull_harris_big takes the rest and orders up to SORT_CAP survivors in LDS, more through global
memory; the host returns an error above launch_bound(n_l) keypoints on a level."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from alvaar_amd import synth
from oracles import Orc

RANK_CAP = 4096   # cull_harris_body: n2 above it -> cull_harris_big
ROW_CAP = 2048    # ... and a level with more rows
SORT_CAP = 4096   # cull_harris_big: m above it -> the row-bucket order instead of the LDS rank sort
BORDER = 31       # edgeThreshold


def launch_bound(n_l):
    """the most keypoints alva_orb_collect accepts from a level (every case's levels have room for more candidates than this)"""
    return max(4 * n_l + 64, 1024)


# ---- images ------------------------------------------------------------------------------------------------------------------------
def bytes_image(w, h, seed):
    """independent random bytes: a FAST corner every ~16 pixels, float Harris responses that do not tie"""
    return np.ascontiguousarray(synth.random_rgba(w, h, seed)[..., 0])


def tiled_image(w, h, seed):
    """a 32 x 32 tile of random bytes repeated: level 0 is exactly periodic, so its Harris responses fall into tie classes with one
    member per repeat of the tile (inside the border)"""
    tile = np.random.RandomState(seed).randint(0, 256, (32, 32)).astype(np.uint8)
    return np.ascontiguousarray(np.tile(tile, ((h + 31) // 32, (w + 31) // 32))[:h, :w])


def lattice(w, h, period, offset):
    """background 40 with single pixels of 255 every `period`: every dot is a FAST corner with the same score and the same response"""
    g = np.full((h, w), 40, np.uint8)
    g[offset::period, offset::period] = 255
    return g


def smooth_image(w, h, seed):
    """the smooth texture the other ORB tests use (test_oracle_vs_ref._img)"""
    from test_oracle_vs_ref import _img
    return _img(w, h, seed)


_BUILDERS = {"bytes": bytes_image, "tiled": tiled_image, "lattice": lattice, "smooth": smooth_image}


@functools.lru_cache(maxsize=None)
def image(spec):
    """spec = (builder name, *arguments); built once, read-only"""
    g = _BUILDERS[spec[0]](*spec[1:])
    g.setflags(write=False)
    return g


# ---- predictor ---------------------------------------------------------------------------------------------------------------------
def features_per_level(nfeatures, scale, nlevels):
    """orb.cpp:799-813 in float32 (the scale factor arrives as a float, cvRound is round-half-even)"""
    f32 = np.float32
    factor = f32(1.0 / float(f32(scale)))
    nd = f32(f32(nfeatures) * (f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(int(np.rint(nd)))
        total += out[-1]
        nd = f32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


@functools.lru_cache(maxsize=None)
def level_scores(spec, scale, nlevels, thr):
    """per level (w, h, FAST scores of the corners inside the border, descending)"""
    out = []
    for lv in Orc.orb_pyramid(image(spec), scale, nlevels):
        h, w = lv.shape
        xy, sc = Orc.fast(lv, thr)
        inside = (xy[:, 0] >= BORDER) & (xy[:, 0] < w - BORDER) & (xy[:, 1] >= BORDER) & (xy[:, 1] < h - BORDER)
        out.append((w, h, np.sort(sc[inside])[::-1]))
    return out


def fast_cull_count(scores, n_l):
    """n2: how many of the (descending) scores the FAST cull keeps for a level budget n_l"""
    if n_l == 0:
        return 0
    if len(scores) <= 2 * n_l:
        return len(scores)
    return int((scores >= scores[2 * n_l - 1]).sum())


Level = namedtuple("Level", "w h n1 n2 n_l m")


def predict(spec, nfeatures, scale=1.2, nlevels=8, thr=20, kp=None):
    """per level (w, h, n1, n2, n_l, m); m is counted from the oracle's octave column (kp: its keypoints, where the caller has them)"""
    if kp is None:
        kp, _ = Orc.orb(image(spec), nfeatures, scale=scale, nlevels=nlevels, fast_thr=thr, describe=False, cap=ORACLE_CAP)
    n_l = features_per_level(nfeatures, scale, nlevels)
    octave = kp[:, 5].astype(np.int64)
    return [Level(w, h, len(sc), fast_cull_count(sc, n_l[l]), n_l[l], int((octave == l).sum()))
            for l, (w, h, sc) in enumerate(level_scores(spec, scale, nlevels, thr))]


# ---- cases -------------------------------------------------------------------------------------------------------------------------
ORACLE_CAP = 40000   # above every level's candidate count here
Case = namedtuple("Case", "id group spec nf scale nlevels thr")

TILED = ("tiled", 320, 240, 4)
BYTES = ("bytes", 320, 240, 7)
BOUND_AT = ("lattice", 320, 320, 8, 4)      # 33 x 33 = 1089 dots, 32 x 32 = 1024 of them inside the border
BOUND_OVER = ("lattice", 324, 324, 8, 4)    # 33 x 33 inside the border
SMOOTH = ("smooth", 320, 240, 9)
TALL = ("bytes", 96, 2100, 9)
SCAN_ROWS = 1024   # k_scan_rows scans this many rows at a time and carries the sum into the next chunk (tall_fast_image: 3 and 2 chunks)

# n_l of the zero_budgets cases, worked from orb.cpp:799-813 for scale 1.2 x 8 levels: n_0 = nf (1 - 1/1.2) / (1 - 1.2^-8) = 0.2172 nf,
# every next level's n is 1/1.2 of it, each rounded; the last level gets what is left of nf.  nf = 3: 0.65, 0.54, 0.45 ... -> 1, 1, 0 ...;
# nf = 4: 0.87, 0.72, 0.60, 0.503, 0.42 ... -> 1, 1, 1, 1, 0 ... and nothing is left for the last level.
ZERO_BUDGETS = {0: [0, 0, 0, 0, 0, 0, 0, 0], 1: [0, 0, 0, 0, 0, 0, 0, 1], 2: [0, 0, 0, 0, 0, 0, 0, 2], 3: [1, 1, 0, 0, 0, 0, 0, 1],
                4: [1, 1, 1, 1, 0, 0, 0, 0]}


@functools.lru_cache(maxsize=None)
def split_points():
    """split_4096's nfeatures, from the FAST scores of its image (one level, so n_l = nfeatures): label -> nfeatures"""
    (_, _, sc), = level_scores(BYTES, 1.2, 1, 20)
    n1 = len(sc)
    nf_lo = max(nf for nf in range(1, n1) if fast_cull_count(sc, nf) <= RANK_CAP)
    half = (n1 + 1) // 2
    return {"nf_lo": nf_lo, "nf_lo+1": nf_lo + 1, "sort_cap": SORT_CAP, "sort_cap+1": SORT_CAP + 1, "n1-1": n1 - 1, "n1": n1, "n1+1": n1 + 1,
            "half-1": half - 1, "half": half, "half+1": half + 1}


SPLIT_LABELS = ("nf_lo", "nf_lo+1", "sort_cap", "sort_cap+1", "n1-1", "n1", "n1+1", "half-1", "half", "half+1")
EDGE_LABELS = SPLIT_LABELS[4:]


@functools.lru_cache(maxsize=None)
def edge_points():
    """edge_small's nfeatures: n against keepN at both culls again, on an image with few enough corners for cull_harris_body"""
    (_, _, sc), = level_scores(SMOOTH, 1.2, 1, 20)
    n1 = len(sc)
    half = (n1 + 1) // 2
    return {"n1-1": n1 - 1, "n1": n1, "n1+1": n1 + 1, "half-1": half - 1, "half": half, "half+1": half + 1}


@functools.lru_cache(maxsize=None)
def cases():
    out = [Case(f"tie_small-{nf}", "tie_small", TILED, nf, 1.2, 1, 20) for nf in (1, 50, 300, 1000)]
    out += [Case(f"tie_big-{nf}", "tie_big", TILED, nf, 1.2, 1, 20) for nf in (2100, 2500)]
    out += [Case("tie_levels-2.0x2", "tie_levels", TILED, 200, 2.0, 2, 20), Case("tie_levels-1.2x8", "tie_levels", TILED, 300, 1.2, 8, 20)]
    out += [Case("bound_at", "bound_at", BOUND_AT, 1, 1.2, 1, 20), Case("bound_over", "bound_over", BOUND_OVER, 1, 1.2, 1, 20)]
    sp = split_points()
    out += [Case(f"split_4096-{label}", "split_4096", BYTES, sp[label], 1.2, 1, 20) for label in SPLIT_LABELS]
    ep = edge_points()
    out += [Case(f"edge_small-{label}", "edge_small", SMOOTH, ep[label], 1.2, 1, 20) for label in EDGE_LABELS]
    out += [Case(f"zero_budgets-{nf}", "zero_budgets", SMOOTH, nf, 1.2, 8, 20) for nf in sorted(ZERO_BUDGETS)]
    out += [Case("tall", "tall", TALL, 300, 1.2, 8, 20)]
    return tuple(out)


# ids known without the oracle (pytest.mark.parametrize wants them at collection; cases() is checked against them on the CPU)
CASE_IDS = tuple([f"tie_small-{nf}" for nf in (1, 50, 300, 1000)] + [f"tie_big-{nf}" for nf in (2100, 2500)]
                 + ["tie_levels-2.0x2", "tie_levels-1.2x8", "bound_at", "bound_over"] + [f"split_4096-{label}" for label in SPLIT_LABELS]
                 + [f"edge_small-{label}" for label in EDGE_LABELS] + [f"zero_budgets-{nf}" for nf in sorted(ZERO_BUDGETS)] + ["tall"])


def case(case_id):
    return next(c for c in cases() if c.id == case_id)


def orb_key(kp):
    """(octave, y, x) order"""
    return np.lexsort((kp[:, 0], kp[:, 1], kp[:, 5]))


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """(keypoints in (octave, y, x) order, their descriptors, predict()'s levels) of a case, computed once and read-only"""
    c = case(case_id)
    kp, desc = Orc.orb(image(c.spec), c.nf, scale=c.scale, nlevels=c.nlevels, fast_thr=c.thr, cap=ORACLE_CAP)
    i = orb_key(kp)
    kp, desc = kp[i], desc[i]
    kp.setflags(write=False)
    desc.setflags(write=False)
    return kp, desc, predict(c.spec, c.nf, c.scale, c.nlevels, c.thr, kp=kp)


def batch_cases():
    """two cameras of one geometry whose level budget exceeds SORT_CAP: (image spec, nfeatures, scale, nlevels)"""
    return [(BYTES, SORT_CAP + 1, 1.2, 1), (TILED, SORT_CAP + 1, 1.2, 1)]


@functools.lru_cache(maxsize=None)
def batch_oracle(i):
    spec, nf, scale, nlevels = batch_cases()[i]
    kp, desc = Orc.orb(image(spec), nf, scale=scale, nlevels=nlevels, fast_thr=20, cap=ORACLE_CAP)
    k = orb_key(kp)
    return kp[k], desc[k], predict(spec, nf, scale, nlevels, 20, kp=kp)


def tall_fast_image(i):
    """0: the tall image itself (96 x 2100); 1: a 64 x 1100 crop of it"""
    g = image(TALL)
    return g if i == 0 else np.ascontiguousarray(g[500:1600, 16:80])
