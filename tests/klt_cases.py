"""TEST INFRASTRUCTURE: the case table of tests/test_klt_cases.py (CPU: every row does what it aims at, oracle against the compiled
reference) and tests/test_gpu_klt_params.py (every row through every KLT entry point and wave layout, bitwise).

The other KLT tests run at one point of the parameter space (30 iterations, eps 0.01, err 30, fb 0.5, three levels of three built).
A ROW here is one set of arguments away from it and the CASES that run with it: image pair, points, priors, the depth the pyramids are
built to.  The cases of a row share its arguments, so one batched launch holds them all.

  crit    the termination criteria, clamped values beside their clamp targets                      (LK and fb-KLT)
  gate    the two thresholds of the forward-backward verdict                                       (fb-KLT)
  tie     a threshold set to one tracked point's own value, and to the float just below it         (fb-KLT)
  band    eps set to the length of one step of one point, and to its two float neighbours: |delta|^2 and eps^2 then differ by
          ~1e-7 relative, where a float comparison of the two cannot decide                        (LK and fb-KLT)
  depth   pyramids built to 0, 1, 2, 5, 7 levels against num_levels 0, 3, 7; on 200 x 152 the top level is 13 x 10 and on 64 x 48
          it is 16 x 12, smaller than a 16 x 16 tile of the searched image; and 1156 x 1156, the smallest size on which all
          eight levels that a pyramid can hold are built (the top one 10 x 10)                      (LK and fb-KLT)

Ties and bands are derived from the oracle (Orc.lk, Orc.lk_deltas), never from the code under test."""
import functools

import numpy as np

from alvaar_amd import synth
from oracles import Orc, pyr_dims

WIN = 9
DEFAULT = dict(num_levels=3, max_iters=30, eps=0.01, err_thresh=30.0, fb_dist=0.5)
LK_KEYS = ("num_levels", "max_iters", "eps")

# name: width, height, points, seed, motion of the content between the two frames
IMAGES = {"a200": (200, 152, 400, 4, (2, 1)), "b96": (96, 72, 300, 5, (2, 1)), "c64": (64, 48, 300, 6, (2, 1)), "d200": (200, 152, 400, 7, (7, -4)),
          "e1156": (1156, 1156, 400, 8, (23, -14))}
PARAM_IMAGES = ("a200", "b96", "c64")
DEPTH_IMAGES = ("d200", "c64")
BUILT = (0, 1, 2, 5, 7)
DEPTH_CASES = [(k, b) for k in DEPTH_IMAGES for b in BUILT] + [("e1156", 7)]
LEVELS = (0, 3, 7)
TIE_IMAGE = "a200"
N_TIES = 2
N_BANDS = 6
BAND_SOURCES = (("a200", 0), ("a200", 3), ("b96", 3))   # (image, num_levels) the band rows look for their steps in, two from each


@functools.lru_cache(maxsize=None)
def image(key):
    """prev, curr, pts, init: squares on black with +-5 of noise (a canvas with a narrow margin, so that the small sizes carry texture
    too), the points of test_oracle_vs_ref.klt_case: inside, on the border, outside; a quarter of them on integer positions"""
    w, h, n, seed, (dx, dy) = IMAGES[key]
    m = 32
    canvas = synth.texture_canvas(w, h, seed, margin=2 * m)
    if (dx, dy) == (2, 1):
        prev, curr = synth.frame_gray(canvas, 3, w, h, noise_seed=11), synth.frame_gray(canvas, 4, w, h, noise_seed=12)
    else:
        rng = np.random.RandomState(seed + 100)
        noisy = lambda g: np.clip(g.astype(np.int16) + rng.randint(-5, 6, g.shape), 0, 255).astype(np.uint8)
        prev, curr = noisy(canvas[m:m + h, m:m + w]), noisy(canvas[m - dy:m - dy + h, m - dx:m - dx + w])
    rng = np.random.RandomState(seed)
    pts = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1).astype(np.float32)
    pts[: n // 4] = np.round(pts[: n // 4])
    pts[0] = (0.0, 0.0)
    pts[1] = (w - 1.0, h - 1.0)
    pts[2] = (-20.0, 5.0)
    init = (pts + rng.uniform(-1.5, 1.5, pts.shape)).astype(np.float32)
    for a in (prev, curr, pts, init):
        a.setflags(write=False)
    return dict(prev=prev, curr=curr, pts=pts, init=init)


def _f32_below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def _f32_above(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


# ---- rows whose arguments are written down ---------------------------------------------------------------------------------------------
CRIT = [("iters=%d" % k, dict(max_iters=k)) for k in (-3, 0, 1, 2, 5, 100, 150)] + \
       [("eps=%g" % e, dict(eps=e)) for e in (-1.0, 0.0, 0.001, 0.03, 0.3, 3.0, 10.0, 25.0)] + \
       [("iters=100,eps=0", dict(max_iters=100, eps=0.0))]      # only the oscillation rule and the count stop this one
CLAMPED = {"iters=-3": "iters=0", "iters=150": "iters=100", "eps=-1": "eps=0", "eps=25": "eps=10"}
GATES = [("err=%g,fb=%g" % (e, f), dict(err_thresh=e, fb_dist=f))
         for e, f in ((0.0, 0.5), (1e-3, 0.5), (30.0, 0.0), (30.0, 0.01), (30.0, 0.05), (30.0, 5.0), (float("inf"), float("inf")))]
TIES = [("tie-%s-%d-%s" % (g, k, side)) for g in ("err", "fb") for k in range(N_TIES) for side in ("at", "below")]
BANDS = [("band-%d-%s" % (k, side)) for k in range(N_BANDS) for side in ("lo", "mid", "hi")]
DEPTHS = ["levels=%d" % L for L in LEVELS]

KIND = {"default": "default"}
KIND.update({n: "crit" for n, _ in CRIT})
KIND.update({n: "gate" for n, _ in GATES})
KIND.update({n: "tie" for n in TIES})
KIND.update({n: "band" for n in BANDS})
KIND.update({n: "depth" for n in DEPTHS})
ROW_NAMES = list(KIND)
LK_ROW_NAMES = [n for n in ROW_NAMES if KIND[n] in ("default", "crit", "band", "depth")]   # the others differ in the verdict alone


def _cases(name, args, keys_built):
    return [dict(name="%s/%s/built=%d" % (name, k, b), image=k, built=b, args=args, **image(k)) for k, b in keys_built]


# ---- rows derived from the oracle -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties():
    """{"err": [...], "fb": [...]}, each entry (point, threshold at which it just passes, the float below it).  The points are ones the
    default arguments accept.  err: the point's own err, as Orc.lk reports it (the verdict is !(err > thresh)).  fb: the backward pass is
    level-0 LK from the forward result with the keypoint itself as the prior; nrm as the verdict computes it (float differences, double
    square root); the threshold is the nearest float at or above it (the verdict is !(nrm > (double) thresh))."""
    I = image(TIE_IMAGE)
    fwd, _, err = Orc.lk(I["prev"], I["curr"], I["pts"], I["init"], 3)
    _, fst = Orc.fbklt(I["prev"], I["curr"], I["pts"], I["init"], 3)
    back, _, _ = Orc.lk(I["curr"], I["prev"], fwd, I["pts"], 0)
    d = (I["pts"] - back).astype(np.float32).astype(np.float64)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    acc = np.flatnonzero(fst)
    # err: the accepted points with the median and with the largest err, each value held by that point alone
    by_err = [i for i in acc[np.argsort(err[acc], kind="stable")] if (err == err[i]).sum() == 1]
    e_pts = [by_err[len(by_err) // 2], by_err[-1]]
    # fb: first a point whose nrm IS a float (one of its two differences is zero), where there is one: the gate at equality; then the median
    moved = [i for i in acc[np.argsort(nrm[acc], kind="stable")] if nrm[i] > 0 and (nrm == nrm[i]).sum() == 1]
    exact = [i for i in moved if float(np.float32(nrm[i])) == nrm[i]]
    f_pts = (exact[:1] + [moved[len(moved) // 2], moved[-1]])[:N_TIES]
    out = {"err": [(int(i), np.float32(err[i]), _f32_below(err[i])) for i in e_pts], "fb": []}
    for i in f_pts:
        at = np.float32(nrm[i])
        if float(at) < nrm[i]:
            at = _f32_above(at)
        out["fb"].append((int(i), at, _f32_below(at)))
    return out


@functools.lru_cache(maxsize=None)
def bands():
    """N_BANDS entries (image, num_levels, point, (eps below, eps, eps above)): eps = float32(|delta|) of one step the point takes on
    level 0 when LK runs with that very eps, kept only if the oracle's result for the point differs between at least two of the three."""
    found = []
    for key, levels in BAND_SOURCES:
        I = image(key)
        lk = lambda e, d=False: (Orc.lk_deltas if d else Orc.lk)(I["prev"], I["curr"], I["pts"], I["init"], levels, eps=float(e))
        _, st, _, deltas, counts = lk(DEFAULT["eps"], True)
        length = lambda dl: np.sqrt(dl[..., 0].astype(np.float64) ** 2 + dl[..., 1].astype(np.float64) ** 2)
        got = 0
        for i in np.flatnonzero(st):
            for j in range(1, int(counts[i]) - 1):
                eps = np.float32(length(deltas[i, j]))
                if not 2e-3 < eps < 0.3:
                    continue
                # eps reaches the levels above and the steps before: look the step up again in a run with eps itself
                _, _, _, d2, c2 = lk(eps, True)
                if not (np.float32(length(d2[i, :c2[i]])) == eps).any():
                    continue
                trio = (_f32_below(eps), eps, _f32_above(eps))
                res = [lk(e) for e in trio]
                bits = [(r[0][i].view(np.uint32).tolist(), int(r[1][i])) for r in res]
                if bits[0] != bits[1] or bits[1] != bits[2]:
                    found.append((key, levels, int(i), trio))
                    got += 1
                    break
            if got == N_BANDS // len(BAND_SOURCES):
                break
    assert len(found) == N_BANDS, found
    return found


@functools.lru_cache(maxsize=None)
def row(name):
    """name, kind, args (all five arguments) and the cases that run with them"""
    kind = KIND[name]
    keys, args = [(k, 3) for k in PARAM_IMAGES], dict(DEFAULT)
    if kind in ("crit", "gate"):
        args.update(dict(CRIT + GATES)[name])
    elif kind == "tie":
        _, g, k, side = name.split("-")
        _, at, below = ties()[g][int(k)]
        args["err_thresh" if g == "err" else "fb_dist"] = float(at if side == "at" else below)
    elif kind == "band":
        _, k, side = name.split("-")
        key, levels, _, trio = bands()[int(k)]
        args.update(num_levels=levels, eps=float(trio[("lo", "mid", "hi").index(side)]))
        keys = [(key, 3)] + [(x, 3) for x in PARAM_IMAGES if x != key]
    elif kind == "depth":
        args["num_levels"] = int(name.split("=")[1])
        keys = DEPTH_CASES
    return dict(name=name, kind=kind, args=args, cases=_cases(name, args, keys))


def levels_built(case):
    w, h = IMAGES[case["image"]][:2]
    return pyr_dims(w, h, WIN, case["built"])


_results = {}


def lk_result(case, which=Orc):
    """(next, status, err) of which.lk on the case, computed once"""
    a = case["args"]
    key = (which.__name__, "lk", case["image"], case["built"]) + tuple(a[k] for k in LK_KEYS)
    if key not in _results:
        _results[key] = which.lk(case["prev"], case["curr"], case["pts"], case["init"], built=case["built"], **{k: a[k] for k in LK_KEYS})
    return _results[key]


def fb_result(case, which=Orc):
    """(tracked, status) of which.fbklt on the case, computed once"""
    a = case["args"]
    key = (which.__name__, "fb", case["image"], case["built"]) + tuple(sorted(a.items()))
    if key not in _results:
        _results[key] = which.fbklt(case["prev"], case["curr"], case["pts"], case["init"], built=case["built"], **a)
    return _results[key]


def same_lk(a, b):
    ok = a[1].astype(bool)
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and \
        np.array_equal(a[2][ok].view(np.uint32), b[2][ok].view(np.uint32))


def same_fb(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
