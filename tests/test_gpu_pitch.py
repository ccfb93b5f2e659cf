"""GPU: the image entry points on pitched sub-views of larger buffers (the table of tests/pitch_cases.py; tests/test_pitch_cases.py checks
the table itself on the CPU).

Every input is a view inside a block filled with a poison value -- padded rows, rows that start at changing offsets within a 64-byte
line, a region of interest three rows down and a few steps into its row and, for the entry points whose contract has no alignment rule,
odd pitches with a start 1, 2 or 3 bytes into the row -- and the result on the view is, bit for bit, the CPU oracle's result on the packed
image (all of these stages are integer arithmetic or replay the reference's float order: no tolerance).  A kernel that took the width for
the pitch on any of its routes would read poison; every case runs with two poison values.  Outputs with a pitch (the gray image of
alva_rgba2gray, gray_out of the pyramid builders, alva_orb_blur's image) are views in poisoned blocks too, laid out differently from the
input: inside the view the oracle's bytes, outside it every byte still the poison.  Each pyramid is built over and over from two frames
in changing layouts.  The drivers (Frontend, TrackBatch) on pitched frames return what they return on packed ones.  Calls the contract
forbids -- a pitch or a pointer off its alignment, a pitch below the row, a batch of mixed geometry -- are refused on the host, before
anything is launched; no such layout is ever handed to a kernel."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import detect_cases as D
import orb_cases as oc
import pitch_cases as P
from alvaar_amd import synth
from oracles import Orc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def _put(img, layout, poison, contract):
    """the image on the device as a view inside a poisoned block: (block tensor, view tensor)"""
    import torch
    block, view, off = P.embed(np.asarray(img), layout, poison, contract)
    t = torch.from_numpy(block).cuda()
    v = torch.as_strided(t, view.shape, view.strides, off)   # (uint8: byte strides are element strides)
    assert v.data_ptr() % P.CONTRACTS[contract][1] == 0 and v.stride(0) == view.strides[0]
    return t, v


class _Out:
    """an output image as a view inside a poisoned block on the device"""

    def __init__(self, w, h, layout, poison, contract):
        import torch
        self.shape, self.poison = (h, w), poison
        self.geom = P.geometry(w, h, contract, layout)
        self.block = torch.full((self.geom.nbytes,), poison, dtype=torch.uint8, device="cuda")
        self.view = torch.as_strided(self.block, (h, w), (self.geom.pitch, 1), self.geom.off)
        assert self.view.data_ptr() % P.CONTRACTS[contract][1] == 0

    def check(self, want, what):
        """inside the view the expected bytes, everywhere else in the block still the poison"""
        blk = self.block.cpu().numpy()
        inside = P.inside_mask(self.shape, self.geom)
        assert np.array_equal(blk[inside].reshape(self.shape), want), what + ("inside",)
        assert (blk[~inside] == self.poison).all(), what + ("outside", int((blk[~inside] != self.poison).sum()))


def _cases(layouts):
    return [(layout, poison) for layout in layouts for poison in P.POISONS]


@functools.lru_cache(maxsize=None)
def _frame(w, h, seed):
    """(rgba, its gray): random bytes -- every stage here is integer, so any input is a legal one, and no two pixels are alike"""
    rgba = synth.random_rgba(w, h, seed)
    gray = Orc.rgba2gray(rgba)
    rgba.setflags(write=False)
    gray.setflags(write=False)
    return rgba, gray


@functools.lru_cache(maxsize=None)
def _pyramid_oracle(w, h, win, depth, seed):
    return Orc.build_pyramid(_frame(w, h, seed)[1], win, depth)


def _assert_levels(pyr, want, what):
    og, od = want
    assert pyr.num_levels == len(og), what
    for l in range(pyr.num_levels):
        g, d = pyr.download_level(l)
        assert np.array_equal(g, og[l]), what + (l, "gray", int((g != og[l]).sum()))
        assert np.array_equal(d, od[l]), what + (l, "deriv", int((d != od[l]).any(axis=2).sum()))


def _image_row(row):
    """a row of FAST_ROWS / BLUR_ROWS / ORB_BATCH_SPECS -> the image"""
    name, _, arg = row.partition(":")
    return oc.tall_fast_image(int(arg)) if arg else oc.image(getattr(oc, name))


# ---------------------------------------------------------------------------------------------------------------- alva_rgba2gray
@pytest.mark.parametrize("w,h", P.RGBA2GRAY_SHAPES)
def test_rgba2gray_on_views(ctx, w, h):
    e = P.ENTRY_POINTS["alva_rgba2gray"]
    rgba, gray = _frame(w, h, 1000 + w + h)
    for layout, poison in _cases(e.layouts):
        _, v = _put(rgba, layout, poison, e.contract)
        out = _Out(w, h, P.OUT_LAYOUT[layout], poison, e.out_contract)
        ctx.rgba2gray(v, out.view)
        out.check(gray, (w, h, layout, poison))
        got = ctx.rgba2gray(v)                                  # ... and into a tensor of the wrapper's own
        assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), gray), (w, h, layout, poison)


# ---------------------------------------------------------------------------------------------------------------- the pyramid builders
def _rounds(layouts):
    """(frame seed, layout, poison) in the order a pyramid is rebuilt: neighbours differ in frame AND layout, so a border or a level left
    over from the build before shows; every layout meets both poisons"""
    out = []
    for poison in P.POISONS:
        for k, layout in enumerate(layouts):
            out.append((k & 1, layout, poison))
    return out


@pytest.mark.parametrize("w,h,win,depth", list(P.PYRAMID_CASES))
def test_pyramid_from_gray_on_views(ctx, w, h, win, depth):
    import alvaar_amd
    e = P.ENTRY_POINTS["alva_pyramid_build_from_gray"]
    pyr = alvaar_amd.Pyramid(ctx, w, h, win, depth)
    assert pyr.num_levels == P.PYRAMID_CASES[(w, h, win, depth)]
    for seed, layout, poison in _rounds(e.layouts):
        _, v = _put(_frame(w, h, seed)[1], layout, poison, e.contract)
        pyr.build_from_gray(v)
        _assert_levels(pyr, _pyramid_oracle(w, h, win, depth, seed), (layout, poison))
    pyr.close()


def _build_from_rgba_on_views(ctx, pyr, w, h, win, depth, on_result=None):
    e = P.ENTRY_POINTS["alva_pyramid_build_from_rgba"]
    for with_copy in (True, False):
        for seed, layout, poison in _rounds(e.layouts):
            rgba, gray = _frame(w, h, seed)
            _, v = _put(rgba, layout, poison, e.contract)
            out = _Out(w, h, P.OUT_LAYOUT[layout], poison, e.out_contract) if with_copy else None
            pyr.build_from_rgba(v, out.view if out else None)
            what = (w, h, win, depth, layout, poison, with_copy)
            if out:
                out.check(gray, what)
            if on_result:
                on_result(pyr, out)
            _assert_levels(pyr, _pyramid_oracle(w, h, win, depth, seed), what)


@pytest.mark.parametrize("w,h,win,depth", list(P.PYRAMID_CASES))
def test_pyramid_from_rgba_on_views(ctx, w, h, win, depth):
    """the default route of a device frame: ONE launch (k_pyr_all: level0_tile and deep_tile<true> read the frame through rgba_pitch,
    halo and mirror reads included, and level0_tile stores the gray copy through its own pitch) where the pyramid has two to four
    levels, k_level0 and the per-level chain otherwise"""
    import alvaar_amd
    pyr = alvaar_amd.Pyramid(ctx, w, h, win, depth)
    assert pyr.num_levels == P.PYRAMID_CASES[(w, h, win, depth)]
    _build_from_rgba_on_views(ctx, pyr, w, h, win, depth)
    pyr.close()


def _digest_of_every_build(ctx):
    """every pyramid case built from RGBA views on whatever route this process takes, each result checked against the oracle; the digest
    of all the bytes produced"""
    import alvaar_amd
    hs = hashlib.sha256()

    def add(pyr, out):
        if out:
            hs.update(out.block.cpu().numpy().tobytes())
        for l in range(pyr.num_levels):
            for a in pyr.download_level(l):
                hs.update(a.tobytes())
    for w, h, win, depth in P.PYRAMID_CASES:
        pyr = alvaar_amd.Pyramid(ctx, w, h, win, depth)
        _build_from_rgba_on_views(ctx, pyr, w, h, win, depth, add)
        pyr.close()
    return hs.hexdigest()


def _two_launch_child():
    import alvaar_amd
    assert os.environ.get("ALVA_PYRAMID_TWO_LAUNCHES") == "1"
    print("DIGEST", _digest_of_every_build(alvaar_amd.Context(0)))


def test_pyramid_two_launch_route_on_views(ctx):
    """the same calls with ALVA_PYRAMID_TWO_LAUNCHES=1 (k_level0<true> + k_pyr_rest; read once, at the first build of a process, hence
    a child process): each result equals the oracle there too, and all the bytes together have this process's digest"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_pitch\ntest_gpu_pitch._two_launch_child()\n" % (root, os.path.join(root, "tests")))
    env = dict(os.environ, ALVA_PYRAMID_TWO_LAUNCHES="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1]
    assert "ALVA_PYRAMID_TWO_LAUNCHES" not in os.environ
    assert theirs == _digest_of_every_build(ctx)


@pytest.mark.parametrize("case,B", [(c, 2) for c in P.PYRAMID_CASES] + [(P.PYRAMID_BATCH_CASE, b) for b in P.PYRAMID_BATCHES if b != 2])
def test_pyramid_batch_on_views(ctx, case, B):
    """alva_pyramid_build_from_rgba_batch (k_level0_batch + the per-level chain): the cameras' frames in blocks of their own under one
    rgba_pitch, their gray copies under another"""
    import alvaar_amd
    from alvaar_amd import capi
    w, h, win, depth = case
    e = P.ENTRY_POINTS["alva_pyramid_build_from_rgba_batch"]
    pyrs = [alvaar_amd.Pyramid(ctx, w, h, win, depth) for _ in range(B)]
    for with_copy in (True, False):
        for k, layout, poison in _rounds(e.layouts):
            seeds = [10 * c + k for c in range(B)]
            views = [_put(_frame(w, h, s)[0], layout, poison, e.contract)[1] for s in seeds]
            outs = [_Out(w, h, P.OUT_LAYOUT[layout], poison, e.out_contract) for _ in range(B)] if with_copy else None
            capi.build_pyramids_batch(ctx, pyrs, views, [o.view for o in outs] if outs else None)
            ctx.sync()
            for c, s in enumerate(seeds):
                what = (case, B, layout, poison, with_copy, c)
                if outs:
                    outs[c].check(_frame(w, h, s)[1], what)
                _assert_levels(pyrs[c], _pyramid_oracle(w, h, win, depth, s), what)
    for p in pyrs:
        p.close()


def test_pyramid_level0_must_be_larger_than_the_window(ctx):
    """a level 0 with width <= win or height <= win would need its REFLECT_101 border reflected more than once (the oracle does that;
    store_mirrors reflects once and would leave the memset's zeros): alva_pyramid_create refuses it.  The smallest level 0 it accepts
    -- one more than the window -- is built exactly, border included"""
    import alvaar_amd
    for w, h, win in P.PYRAMID_REFUSED:
        og, _ = Orc.build_pyramid(np.arange(w * h, dtype=np.uint8).reshape(h, w), win, 0)
        assert og[0][:, 0].any() and og[0][-1].any()          # (what would have to be there: not zeros)
        with pytest.raises(alvaar_amd.AlvaError, match="bad argument"):
            alvaar_amd.Pyramid(ctx, w, h, win, 3)
    w, h, win, depth = P.PYRAMID_SMALLEST
    pyr = alvaar_amd.Pyramid(ctx, w, h, win, depth)
    for seed, layout, poison in _rounds(P.ALIGNED_LAYOUTS):
        rgba, gray = _frame(w, h, seed)
        pyr.build_from_gray(_put(gray, layout, poison, "gray4")[1])
        _assert_levels(pyr, _pyramid_oracle(w, h, win, depth, seed), ("gray", layout, poison))
        pyr.build_from_rgba(_put(_frame(w, h, seed ^ 1)[0], layout, poison, "rgba")[1])
        _assert_levels(pyr, _pyramid_oracle(w, h, win, depth, seed ^ 1), ("rgba", layout, poison))
    pyr.close()


# ---------------------------------------------------------------------------------------------------------------- grid detector
def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", P.DETECT_ROWS)
def test_detect_grid_on_views(ctx, name):
    """alva_detect_grid and alva_detect_grid_enqueue / _collect (k_eig's tile load and k_subpix read the image): the point list as uint32
    in its order, the count and the new threshold of every call of the row"""
    import torch
    D.check_conditions(name)
    c, ref = D.case(name), D.reference_of(name)
    occ = None if c.occupied is None or len(c.occupied) == 0 else torch.from_numpy(np.array(c.occupied)).cuda()
    e = P.ENTRY_POINTS["alva_detect_grid"]
    assert P.ENTRY_POINTS["alva_detect_grid_enqueue"] == e
    for layout, poison in _cases(e.layouts):
        _, g = _put(c.gray, layout, poison, e.contract)
        mq = c.max_quality
        for pts_ref, mq_ref in ref:
            n = len(pts_ref)
            cap = n + 3 if c.cap is None else c.cap
            want = pts_ref[:cap].view(np.uint32)
            what = (name, layout, poison)
            one, q1 = ctx.detect_grid(g, c.cell, occ, roi=c.roi, max_quality=mq, cap=cap)
            assert q1 == mq_ref and np.array_equal(_bits(one), want), what
            two, q2, count = ctx.detect_grid_collect(ctx.detect_grid_enqueue(g, c.cell, occ, roi=c.roi, max_quality=mq, cap=cap))
            assert q2 == mq_ref and count == n and np.array_equal(_bits(two), want), what
            mq = mq_ref


# ---------------------------------------------------------------------------------------------------------------- ORB, FAST, the blur
def _ambiguous():
    from alvaar_amd.capi import lib, check
    n = C.c_int(0)
    check(lib.alva_orb_ambiguous_rotations(C.byref(n), 1))
    return n.value


@pytest.mark.parametrize("case_id", P.ORB_ROWS)
def test_orb_on_views(ctx, case_id):
    """alva_orb_detect_and_compute reads its input in pyr_column_body (several levels) or copy_level0_body (one level): the keypoint
    records bitwise in (octave, y, x) order, no descriptor row different, no ambiguous rotation"""
    import alvaar_amd
    c = oc.case(case_id)
    rkp, rd, lv = oc.oracle(case_id)
    g = oc.image(c.spec)
    h, w = g.shape
    orb = alvaar_amd.Orb(ctx, w, h, c.nf, scale=c.scale, nlevels=c.nlevels, fast_threshold=c.thr)
    cap = max(4 * c.nf + 1024, len(rkp))
    e = P.ENTRY_POINTS["alva_orb_detect_and_compute"]
    _ambiguous()
    for layout, poison in _cases(e.layouts):
        _, v = _put(g, layout, poison, e.contract)
        kp, desc = orb.detect_and_compute(v, cap=cap)
        kp, desc = kp.cpu().numpy(), desc.cpu().numpy()
        what = (case_id, layout, poison)
        assert len(kp) == len(rkp) and len(rkp) > 0, what + (len(kp), len(rkp))
        assert np.array_equal(kp.view(np.uint32), rkp.view(np.uint32)), what
        assert (desc != rd).any(axis=1).sum() == 0, what
    assert _ambiguous() == 0
    orb.close()


@functools.lru_cache(maxsize=None)
def _orb_batch_oracle(spec_name):
    nf, scale, nlevels = P.ORB_BATCH_GEOMETRY
    kp, desc = Orc.orb(oc.image(getattr(oc, spec_name)), nf, scale=scale, nlevels=nlevels, fast_thr=20, cap=oc.ORACLE_CAP)
    k = oc.orb_key(kp)
    return kp[k], desc[k]


@pytest.mark.parametrize("B", P.ORB_BATCHES)
def test_orb_batch_on_views(ctx, B):
    """alva_orb_detect_and_compute_batch: every camera's image in a block of its own, one shared gray_pitch"""
    import alvaar_amd
    from alvaar_amd import capi
    nf, scale, nlevels = P.ORB_BATCH_GEOMETRY
    specs = [P.ORB_BATCH_SPECS[c % len(P.ORB_BATCH_SPECS)] for c in range(B)]
    cap = max(4 * nf + 1024, max(len(_orb_batch_oracle(s)[0]) for s in specs))
    orbs = [alvaar_amd.Orb(ctx, 320, 240, nf, scale=scale, nlevels=nlevels) for _ in range(B)]
    e = P.ENTRY_POINTS["alva_orb_detect_and_compute_batch"]
    _ambiguous()
    for layout, poison in _cases(e.layouts):
        views = [_put(oc.image(getattr(oc, s)), layout, poison, e.contract)[1] for s in specs]
        assert len({v.stride(0) for v in views}) == 1
        got = capi.orb_detect_and_compute_batch(ctx, orbs, views, cap)
        for c, s in enumerate(specs):
            rkp, rd = _orb_batch_oracle(s)
            kp, desc = got[c][0].cpu().numpy(), got[c][1].cpu().numpy()
            what = (B, layout, poison, c, s)
            assert len(kp) == len(rkp) and len(rkp) > 0, what
            assert np.array_equal(kp.view(np.uint32), rkp.view(np.uint32)) and (desc != rd).any(axis=1).sum() == 0, what
    assert _ambiguous() == 0
    for o in orbs:
        o.close()


@pytest.mark.parametrize("row", P.FAST_ROWS)
def test_fast_on_views(ctx, row):
    g = _image_row(row)
    rxy, rsc = Orc.fast(g, 20)
    assert len(rxy) > 0
    e = P.ENTRY_POINTS["alva_fast"]
    for layout, poison in _cases(e.layouts):
        _, v = _put(g, layout, poison, e.contract)
        xy, sc = ctx.fast(v, 20)
        assert np.array_equal(xy.cpu().numpy(), rxy) and np.array_equal(sc.cpu().numpy(), rsc), (row, layout, poison)


@pytest.mark.parametrize("row", P.BLUR_ROWS)
def test_orb_blur_on_views(ctx, row):
    g = _image_row(row)
    h, w = g.shape
    want = Orc.orb_blur(g)
    e = P.ENTRY_POINTS["alva_orb_blur"]
    for layout, poison in _cases(e.layouts):
        _, v = _put(g, layout, poison, e.contract)
        out = _Out(w, h, P.OUT_LAYOUT[layout], poison, e.out_contract)
        ctx.orb_blur(v, out.view)
        out.check(want, (row, layout, poison))


# ---------------------------------------------------------------------------------------------------------------- the drivers
N_PTS = 300


@functools.lru_cache(maxsize=None)
def _driver_inputs(seed):
    import torch
    w, h, n = P.DRIVER_SIZE
    frames = synth.stream_rgba(w, h, n, seed=seed, noise=True)
    frames.setflags(write=False)
    rng = np.random.RandomState(seed)
    pts = torch.from_numpy(rng.uniform(40, [w - 40, h - 40], (N_PTS, 2)).astype(np.float32)).cuda()
    pb = synth.make_pnp_problem(N_PTS, seed + 1, outlier_frac=0.15)
    bv, uv, wp = (torch.from_numpy(pb[k]).cuda() for k in ("bv", "uv", "wpt"))
    return dict(frames=frames, pts=pts, bv=bv, uv=uv, wp=wp, K=pb["K"])


def _run_frontend(ahead, place, fe=None):
    """three frames through a Frontend (a new one unless given); place(frame) puts a frame on the device.  Per frame (status, pose bytes,
    keypoints, results)"""
    import alvaar_amd
    w, h, n = P.DRIVER_SIZE
    I = _driver_inputs(5)
    dev = [place(I["frames"][k]) for k in range(n)]
    fe = fe or alvaar_amd.Frontend(0, w, h, N_PTS, 300)
    out = []
    for k in range(n):
        nxt = dev[k + 1] if ahead and k + 1 < n else None
        st, pose, nkp = fe.track(dev[k], I["pts"], I["bv"], I["uv"], I["wp"], I["K"], rgba_next=nxt, look_ahead=ahead)
        fe.sync()
        res = {a: b.cpu().numpy().copy() for a, b in fe.results().items() if k > 0 or a in ("keypoints", "descriptors")}
        out.append((st, pose.tobytes(), nkp, res))
    fe.close()
    return out


@functools.lru_cache(maxsize=None)
def _frontend_on_packed(ahead):
    import torch
    out = _run_frontend(ahead, lambda f: torch.from_numpy(np.array(f)).cuda())
    assert all(nkp > 50 for _, _, nkp, _ in out) and out[-1][0] >= 1 and int(out[-1][3]["status"].sum()) > N_PTS // 4   # not vacuous
    return out


def _same_frames(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[:3] == b[:3], what + (k, a[0], b[0], a[2], b[2])
        assert a[3].keys() == b[3].keys()
        for key in a[3]:
            assert a[3][key].dtype == b[3][key].dtype and a[3][key].tobytes() == b[3][key].tobytes(), what + (k, key)


@pytest.mark.parametrize("ahead", [False, True])
def test_frontend_on_views(ahead):
    """alva_frontend_track (ahead False) and alva_frontend_track_ahead with the next frame announced, which shares the pitch: status, pose
    bytes, keypoints, descriptors, tracked points and matches of every frame as on packed frames"""
    e = P.ENTRY_POINTS["alva_frontend_track_ahead" if ahead else "alva_frontend_track"]
    want = _frontend_on_packed(ahead)
    for layout, poison in _cases(e.layouts):
        got = _run_frontend(ahead, lambda f: _put(f, layout, poison, e.contract)[1])
        _same_frames(got, want, (ahead, layout, poison))


def _run_track_batch(detect, place):
    import alvaar_amd
    w, h, n = P.DRIVER_SIZE
    cams = [_driver_inputs(7), _driver_inputs(8)]
    dev = [[place(I["frames"][k]) for k in range(n)] for I in cams]
    tb = alvaar_amd.TrackBatch(0, w, h, len(cams), N_PTS, N_PTS)
    if detect:
        tb.enable_detector(300)
    tb.bind([I["pts"] for I in cams], [I["bv"] for I in cams], [I["uv"] for I in cams], [I["wp"] for I in cams])
    out = []
    for k in range(n):
        st, poses = tb.step([d[k] for d in dev], cams[0]["K"], plain=not detect)
        for i in range(len(cams)):
            res = {}
            if k > 0:
                tr, ok = tb.results(i)
                res.update(tracked=tr.cpu().numpy().copy(), status=ok.cpu().numpy().copy())
            if detect:
                res.update({a: b.cpu().numpy().copy() for a, b in tb.detections(i).items() if k > 0 or a in ("keypoints", "descriptors")})
            out.append((int(st[i]), poses[i].tobytes() if st[i] >= 1 else b"", int(tb.nkp[i]) if detect else 0, res))
    tb.close()
    return out


@functools.lru_cache(maxsize=None)
def _track_batch_on_packed(detect):
    import torch
    out = _run_track_batch(detect, lambda f: torch.from_numpy(np.array(f)).cuda())
    assert all(o[0] >= 1 for o in out[-2:]) and all(int(o[3]["status"].sum()) > N_PTS // 4 for o in out[-2:])   # not vacuous
    assert not detect or all(o[2] > 50 for o in out)
    return out


@pytest.mark.parametrize("detect", [False, True])
def test_track_batch_on_views(ctx, detect):
    """alva_track_batch_step and alva_track_batch_step_detect (with the detector lane): two cameras, every frame in a block of its own
    under one rgba_pitch"""
    e = P.ENTRY_POINTS["alva_track_batch_step_detect" if detect else "alva_track_batch_step"]
    want = _track_batch_on_packed(detect)
    for layout, poison in _cases(e.layouts):
        got = _run_track_batch(detect, lambda f: _put(f, layout, poison, e.contract)[1])
        _same_frames(got, want, (detect, layout, poison))


def test_drivers_refuse_frames_of_two_pitches_and_a_forbidden_pitch():
    """the wrappers pass ONE pitch per call: a next frame or a camera with another row stride is refused before the call, and a frame
    pitch off its rule by alva_frontend_track's argument checks (alva_pyramid_build_from_rgba's, before anything is launched); the
    same Frontend then runs the three packed frames as a fresh one does"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    w, h, n = P.DRIVER_SIZE
    I = _driver_inputs(5)
    packed = torch.from_numpy(np.array(I["frames"][0])).cuda()
    padded = _put(I["frames"][1], "pad_min", 171, "rgba")[1]
    shifted = _put(I["frames"][0], "offset", 171, "rgba")[1]
    fe = alvaar_amd.Frontend(0, w, h, N_PTS, 300)
    args = (I["pts"], I["bv"], I["uv"], I["wp"], I["K"])
    with pytest.raises(AssertionError):
        fe.track(packed, *args, rgba_next=padded)
    with pytest.raises(AssertionError):
        fe.track(padded, *args, rgba_next=packed)
    pose, st, nkp = np.zeros(7), C.c_int(-1), C.c_int(-1)
    K = I["K"]
    for ptr, pitch in ((shifted.data_ptr(), shifted.stride(0) + 4), (shifted.data_ptr() + 4, shifted.stride(0)), (shifted.data_ptr(), 4 * w - 16)):
        with pytest.raises(alvaar_amd.AlvaError, match="bad argument"):
            capi.check(capi.lib.alva_frontend_track(fe.h, ptr, pitch, I["pts"].data_ptr(), N_PTS, I["bv"].data_ptr(), I["uv"].data_ptr(),
                                                    I["wp"].data_ptr(), N_PTS, K[0], K[1], K[2], K[3], pose.ctypes.data, C.byref(st), C.byref(nkp)))
    assert st.value == -1 and nkp.value == -1 and not pose.any()
    _same_frames(_run_frontend(False, lambda f: torch.from_numpy(np.array(f)).cuda(), fe), _frontend_on_packed(False), ("after refusals",))
    tb = alvaar_amd.TrackBatch(0, w, h, 2, N_PTS, N_PTS)
    tb.bind([I["pts"]] * 2, [I["bv"]] * 2, [I["uv"]] * 2, [I["wp"]] * 2)
    with pytest.raises(AssertionError):
        tb.step([packed, padded], K)
    with pytest.raises(AssertionError):
        tb.frame_table([padded, shifted])
    tb.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_forbidden_layouts_are_refused_on_the_host(ctx):
    """every call below breaks its entry point's rule and must come back as an error from the argument checks, which run before anything
    is allocated or launched (the pointers still lie inside real allocations); the outputs stay untouched, and the same context then
    gives the oracle's result for a correct call"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    lib, AlvaError = capi.lib, alvaar_amd.AlvaError
    w, h, win, depth = 68, 33, 9, 3
    rgba, gray = _frame(w, h, 0)
    bt, rv = _put(rgba, "offset", 171, "rgba")                 # room on every side of the view for the shifted pointers below
    gt, gv = _put(gray, "offset", 171, "gray4")
    out = _Out(w, h, "offset", 84, "gray4")
    rp, gp, op = rv.data_ptr(), gv.data_ptr(), out.view.data_ptr()
    RP, GP, OP = rv.stride(0), gv.stride(0), out.view.stride(0)
    pyr, other = alvaar_amd.Pyramid(ctx, w, h, win, depth), alvaar_amd.Pyramid(ctx, w + 4, h, win, depth)
    pyr2 = alvaar_amd.Pyramid(ctx, w, h, win, depth)

    def refused(fn, *args):
        with pytest.raises(AlvaError, match="bad argument"):
            capi.check(fn(*args))

    # alva_rgba2gray: RGBA pitch not a multiple of 16 / base not 16-byte aligned / pitch below the row; the same for the gray output
    for a_rp, a_RP, a_op, a_OP in ((rp, RP + 4, op, OP), (rp, RP + 8, op, OP), (rp + 4, RP, op, OP), (rp + 8, RP, op, OP), (rp, 4 * w - 16, op, OP),
                                   (rp, RP, op, OP + 2), (rp, RP, op, OP + 1), (rp, RP, op + 1, OP), (rp, RP, op + 2, OP), (rp, RP, op, w - 4)):
        refused(lib.alva_rgba2gray, ctx.h, a_rp, a_RP, w, h, a_op, a_OP)
    # alva_pyramid_build_from_gray
    for a_gp, a_GP in ((gp, GP + 2), (gp, GP + 1), (gp + 1, GP), (gp + 2, GP), (gp, w - 4)):
        refused(lib.alva_pyramid_build_from_gray, ctx.h, pyr.h, a_gp, a_GP)
    # alva_pyramid_build_from_rgba: the frame, then gray_out
    for a_rp, a_RP, a_op, a_OP in ((rp, RP + 4, op, OP), (rp + 4, RP, op, OP), (rp + 8, RP, 0, 0), (rp, 4 * w - 16, op, OP), (rp, RP, op, OP + 2),
                                   (rp, RP, op + 2, OP), (rp, RP, op + 1, OP), (rp, RP, op, w - 4)):
        refused(lib.alva_pyramid_build_from_rgba, ctx.h, pyr.h, a_rp, a_RP, a_op, a_OP)
    # the batch: the shared pitches, one camera's pointer, a pyramid of another geometry
    arr = lambda *v: (C.c_void_p * len(v))(*v)
    good = (arr(pyr.h, pyr2.h), arr(rp, rp), RP, arr(op, op), OP)
    for k, bad in ((2, RP + 4), (2, 4 * w - 16), (4, OP + 2), (4, w - 4), (1, arr(rp, rp + 4)), (1, arr(rp + 8, rp)), (3, arr(op, op + 2)),
                   (3, arr(op + 1, op)), (0, arr(pyr.h, other.h)), (0, arr(other.h, pyr.h))):
        args = list(good)
        args[k] = bad
        refused(lib.alva_pyramid_build_from_rgba_batch, ctx.h, *args, 2)
    # the wrappers refuse tensors they could only misread: frames of one call under two pitches, a pixel that is not 4 adjacent bytes
    rv2 = _put(rgba, "pad_min", 171, "rgba")[1]
    with pytest.raises(AssertionError):
        capi.build_pyramids_batch(ctx, [pyr, pyr2], [rv, rv2])
    sparse = torch.zeros((h, w, 8), dtype=torch.uint8, device="cuda")[:, :, :4]     # pixels 8 bytes apart
    assert sparse.stride(1) == 8
    with pytest.raises(AssertionError):
        pyr.build_from_rgba(sparse)
    with pytest.raises(AssertionError):
        ctx.rgba2gray(sparse)
    # the byte-contract entry points: a pitch below the row is all they refuse
    img = oc.image(oc.SMOOTH)
    ih, iw = img.shape
    it, iv = _put(img, "offset", 171, "byte")
    ip = iv.data_ptr()
    kp = torch.full((64, 6), -7.0, dtype=torch.float32, device="cuda")
    desc = torch.full((64, 32), 0xA5, dtype=torch.uint8, device="cuda")
    xy, sc = torch.full((64, 2), -7, dtype=torch.int32, device="cuda"), torch.full((64,), -7, dtype=torch.int32, device="cuda")
    pts = torch.full((64, 2), -7.0, dtype=torch.float32, device="cuda")
    orbs = [alvaar_amd.Orb(ctx, iw, ih, 300) for _ in range(2)]
    cnt, mq, pend = C.c_int(-1), C.c_double(1e-3), capi.DetectPending()
    bout = _Out(iw, ih, "offset", 84, "byte")
    refused(lib.alva_orb_detect_and_compute, ctx.h, orbs[0].h, ip, iw - 1, kp.data_ptr(), desc.data_ptr(), 64, C.byref(cnt))
    refused(lib.alva_orb_detect_and_compute_batch, ctx.h, arr(orbs[0].h, orbs[1].h), 2, arr(ip, ip), iw - 1, arr(kp.data_ptr(), kp.data_ptr()),
            arr(desc.data_ptr(), desc.data_ptr()), 64)
    refused(lib.alva_fast, ctx.h, ip, iw - 1, iw, ih, 20, xy.data_ptr(), sc.data_ptr(), 64, C.byref(cnt))
    refused(lib.alva_orb_blur, ctx.h, ip, iw - 1, iw, ih, bout.view.data_ptr(), bout.view.stride(0))
    refused(lib.alva_orb_blur, ctx.h, ip, iv.stride(0), iw, ih, bout.view.data_ptr(), iw - 1)
    refused(lib.alva_detect_grid, ctx.h, ip, iw - 1, iw, ih, 16, None, 0, 0, 0, iw, ih, C.byref(mq), pts.data_ptr(), 64, C.byref(cnt))
    refused(lib.alva_detect_grid_enqueue, ctx.h, ip, iw - 1, iw, ih, 16, None, 0, 0, 0, iw, ih, 1e-3, pts.data_ptr(), 64, C.byref(pend))
    ctx.sync()
    # nothing was written ...
    out.check(np.full((h, w), 84, np.uint8), ("gray outputs",))
    bout.check(np.full((ih, iw), 84, np.uint8), ("blur output",))
    assert bool((kp == -7.0).all()) and bool((desc == 0xA5).all()) and bool((xy == -7).all()) and bool((sc == -7).all()) and bool((pts == -7.0).all())
    assert bool((bt == torch.from_numpy(P.embed(np.asarray(rgba), "offset", 171, "rgba")[0]).cuda()).all())
    # ... and the context, the pyramids and the detector objects work: correct calls on the same views match the oracle
    ctx.rgba2gray(rv, out.view)
    out.check(gray, ("rgba2gray after",))
    out2 = _Out(w, h, "pad_min", 84, "gray4")
    pyr.build_from_rgba(rv, out2.view)
    out2.check(gray, ("build_from_rgba after",))
    _assert_levels(pyr, _pyramid_oracle(w, h, win, depth, 0), ("build_from_rgba after",))
    pyr2.build_from_gray(gv)
    _assert_levels(pyr2, _pyramid_oracle(w, h, win, depth, 0), ("build_from_gray after",))
    capi.build_pyramids_batch(ctx, [pyr2, pyr], [rv, rv])
    ctx.sync()
    _assert_levels(pyr2, _pyramid_oracle(w, h, win, depth, 0), ("batch after",))
    rkp, rd = _orb_batch_oracle("SMOOTH")
    k1, d1 = orbs[0].detect_and_compute(iv)
    assert np.array_equal(k1.cpu().numpy().view(np.uint32), rkp.view(np.uint32)) and np.array_equal(d1.cpu().numpy(), rd)
    fxy, fsc = ctx.fast(iv, 20)
    rxy, rsc = Orc.fast(img, 20)
    assert np.array_equal(fxy.cpu().numpy(), rxy) and np.array_equal(fsc.cpu().numpy(), rsc)
    ctx.orb_blur(iv, bout.view)
    bout.check(Orc.orb_blur(img), ("blur after",))
    for o in orbs:
        o.close()
    for p in (pyr, pyr2, other):
        p.close()
