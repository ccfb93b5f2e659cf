"""TEST INFRASTRUCTURE: cases for describe.hip's 7 x 7 blur (alva_orb_blur) and BRIEF of supplied points (alva_describe) at the smallest
sizes the entries accept, on images that pin the rounding and the comparisons' ties, and on coordinates no image contains.
test_describe_cases.py (CPU) asserts what the table claims from the oracle; test_gpu_describe_cases.py runs it on the GPU.

A point is described iff Rect(31, 31, w - 62, h - 62) contains Point(cvRound(x), cvRound(y)): at 63 x 63 that is the one pixel (31, 31).
cvRound of a float beyond the int range (or NaN) is the x86 conversion's INT_MIN in the reference; __float2int_rn saturates on the GPU (NaN
gives 0): both land outside every Rect, and the kernel computes no address from them."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

NAN, INF = float("nan"), float("inf")


# ---- images (spec = (builder name, *arguments); built once, read-only) -------------------------------------------------------------------
def _bytes(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def _tiled(w, h, seed):
    """a 64 x 64 tile of random bytes repeated (compresses well in the recorded fixture)"""
    t = _bytes(64, 64, seed)
    return np.ascontiguousarray(np.tile(t, ((h + 63) // 64, (w + 63) // 64))[:h, :w])


def _const(w, h, v):
    return np.full((h, w), v, np.uint8)


def _checker(w, h):
    y, x = np.mgrid[:h, :w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def _halves(w, h, lo, hi):
    g = np.full((h, w), lo, np.uint8)
    g[:, w // 2:] = hi
    return g


# Six 7 x 7 patches side by side (7 rows x 42 columns), found by searching random bright patches: the blur of each patch's centre pixel
# (row 3, columns 3, 10, ..., 38 -- its window is the patch, no border) is k + 0.5 exactly in float, with k = TIE_FLOORS.  Round half to even
# gives k for the four even k and k + 1 for the two odd; truncating s + 0.5 would give k + 1 throughout.
_TIES_HEX = (
    "8ce8d0c6b794e9c2cc79bbc3d4f68ec2c07588b6ce94e36f78e8f7c2d1d4e076f0b19f78adbdfd84c2cdd0b0ceecfa97e4f9aae275efa8dae77e75c8"
    "7cfc77f188cad5aea3c7c0dea672d16c906cc3a96f90bab2828b978291a0f5c6a8fe6e70b46afd7ecd6e77ae769f95abd1c8b0a49cf6aed8d3e3c1e7"
    "a2e4f8bed1e777cae49872d7c3b98b8a69bb709bba95f1a9bae39dc3a066b5e2d3fee9717c89b2778bffc499859a679f9795e6787ee399d2b3e5ce9d"
    "7a69be9fa996c6a06497d3698ab7b9f2affa6ef89ad7ede6afc2e470899cbab095ebf8c5fbe98699a6be9b71dfa88692b6e09b836e6cd065b06ee87d"
    "b59fc369edd6b8e8bb7b87b5a18ff291b4b5ae8f74bcf5676debc5b591d266f77db3c4a47df864ce9f856988c6f4a392f7baf46689f0")
TIE_FLOORS = (178, 166, 168, 172, 175, 177)
GAUSS_TAPS = np.array([0x3d8fafb1, 0x3e06387e, 0x3e434a39, 0x3e5d4ae0, 0x3e434a39, 0x3e06387e, 0x3d8fafb1], np.uint32).view(np.float32)


def _ties():
    return np.frombuffer(bytes.fromhex(_TIES_HEX), np.uint8).reshape(7, 42).copy()


def blur_centres(g):
    """the float value the blur rounds, for the centre pixel of each 7 x 7 patch of a 7-row image: one float operation at a time, in the
    kernel's and the oracle's order"""
    k = GAUSS_TAPS
    P = g.reshape(7, -1, 7).transpose(1, 0, 2).astype(np.float32)      # [patch, y, x]
    rows = k[0] * P[:, :, 0]
    for i in range(1, 7):
        rows = rows + k[i] * P[:, :, i]
    s = k[3] * rows[:, 3]
    for j in range(1, 4):
        s = s + k[3 + j] * (rows[:, 3 + j] + rows[:, 3 - j])
    return s


_BUILDERS = {"bytes": _bytes, "tiled": _tiled, "const": _const, "checker": _checker, "halves": _halves, "ties": _ties}


@functools.lru_cache(maxsize=None)
def image(spec):
    g = np.ascontiguousarray(_BUILDERS[spec[0]](*spec[1:]))
    g.setflags(write=False)
    return g


# ---- 7 x 7 blur ------------------------------------------------------------------------------------------------------------------------
# the kernel's tile is 64 x 16 outputs with a 3-pixel halo; the entry takes width > 6 and height > 6
BLUR = {
    "7x7": ("bytes", 7, 7, 1), "8x7": ("bytes", 8, 7, 2), "7x64": ("bytes", 7, 64, 3), "64x16": ("bytes", 64, 16, 4),     # one tile exactly
    "65x17": ("bytes", 65, 17, 5), "67x7": ("bytes", 67, 7, 6),                                                              # one pixel / three into the next tile
    "zeros": ("const", 70, 20, 0), "full": ("const", 70, 20, 255), "checker": ("checker", 70, 20),                           # rounding, saturation
    "ties": ("ties",),                                                                                                       # exact halves
}
BLUR_IDS = tuple(BLUR)
BLUR_PITCHED = "65x17"


@functools.lru_cache(maxsize=None)
def blur_oracle(case_id):
    from oracles import Orc
    out = Orc.orb_blur(image(BLUR[case_id]))
    out.setflags(write=False)
    return out


# ---- BRIEF -----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id spec pts valid")     # valid: the expected flags where the table states them, else None

# the issue's hostile values and the ones next to the int range's ends; 2^32 + 512 wraps to 512 in a conversion through a 64-bit integer
HOSTILE = (NAN, INF, -INF, 3e9, -3e9, 2147483520.0, -0.0, 2147483648.0, -2147483648.0, -2147483904.0, 4294967296.0, 4294967808.0, 1e30, -1e30)
HOSTILE_SPEC = ("tiled", 576, 64, 21)              # x = 512 is describable here: 31 <= 512 < 576 - 31
HOSTILE_Y = 32.0                                   # rows 31 and 32 are


def _hostile_points():
    """every hostile value as x, as y and as both, each between two valid points"""
    rng = np.random.RandomState(22)
    rows, hostile = [], []
    for v in HOSTILE:
        for p in ((v, HOSTILE_Y), (512.0, v), (v, v)):
            rows.append((float(rng.randint(31, 545)), float(rng.randint(31, 33))))
            rows.append(p)
            hostile.append(len(rows) - 1)
    rows.append((512.0, HOSTILE_Y))
    return np.array(rows, np.float32), np.array(hostile)


def _seam_points():
    """along the seam of the two-level image (x = 50), on both sides of it, out to where the pattern no longer reaches across"""
    return np.array([(x, y) for y in (31, 40, 48) for x in (31, 36, 37, 45, 48, 49, 50, 51, 52, 55, 63, 64, 68)], np.float32)


def _spread(w, h, n, seed):
    """n points over the image and a little beyond its describable part"""
    return np.random.RandomState(seed).uniform(25, [w - 25, h - 25], (n, 2)).astype(np.float32)


SIZES = (7, 8, 9, 64, 65)        # eight keypoints per block
SIZE_SPEC = ("bytes", 120, 100, 31)
CASES = (
    Case("63x63", ("bytes", 63, 63, 11), np.array([(31, 31), (31.5, 31), (30.5, 31), (31, 30.5), (31.49, 31.49), (31, 31.5), (30.51, 30.5), (32, 31), (31, 32)], np.float32),
         (1, 0, 0, 0, 1, 0, 0, 0, 0)),                                       # 31.5 rounds to 32, 30.5 to 30: half to even
    Case("64x63", ("bytes", 64, 63, 12), np.array([(31, 31), (32, 31), (33, 31), (30, 31), (31, 32), (32.5, 31), (31.5, 31), (32, 30)], np.float32),
         (1, 1, 0, 0, 0, 1, 1, 0)),                                          # two describable pixels in one row
    Case("63x64", ("bytes", 63, 64, 13), np.array([(31, 31), (31, 32), (31, 33), (31, 30), (32, 31), (31, 32.5), (31, 31.5), (30, 32)], np.float32),
         (1, 1, 0, 0, 0, 1, 1, 0)),                                          # ... in one column
    Case("hostile", HOSTILE_SPEC, _hostile_points()[0], None),
    Case("flat", ("const", 80, 70, 128), _spread(80, 70, 40, 14), None),     # every comparison a tie: every bit 0
    Case("halves", ("halves", 100, 80, 10, 200), _seam_points(), None),
) + tuple(Case(f"n{n}", SIZE_SPEC, _spread(120, 100, n, 32), None) for n in SIZES)
CASE_IDS = tuple(c.id for c in CASES)
PITCHED = "n65"


def case(case_id):
    return next(c for c in CASES if c.id == case_id)


def hostile_rows():
    return _hostile_points()[1]


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """(desc [n, 32], valid [n]) of a case from Orc.describe, computed once and read-only"""
    from oracles import Orc
    c = case(case_id)
    d, v = Orc.describe(image(c.spec), c.pts)
    d.setflags(write=False)
    v.setflags(write=False)
    return d, v
