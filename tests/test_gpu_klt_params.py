"""GPU parity: pyramidal LK and forward-backward KLT away from their default arguments -- the rows of tests/klt_cases.py (termination
criteria and their clamps, the verdict's two thresholds, thresholds tied to one point's own value, eps inside the float band of the
64-lane layout's stopping test, pyramids of every depth against every num_levels) through alva_lk_track, alva_fbklt_track and the three
wave layouts of alva_fbklt_track_batch; the refusal of pyramids that do not belong together; and the LK pyramid's build kernels at other
windows and depths than 9 / 3.  The kernels replay the reference's float order: positions and err are compared as uint32, status exactly."""
from types import SimpleNamespace

import numpy as np
import pytest

import klt_cases as K
from alvaar_amd import synth
from oracles import Orc, Ref, pyr_dims, ref_available
from test_klt_cases import PYR_DEEP, PYR_DEPTHS, PYR_SIZES, PYR_WINS, pyr_frame

pytestmark = pytest.mark.gpu

FB_LAYOUTS = ("fbklt", "batch64", "batch8", "batch5")      # k_klt, k_klt_batch, k_klt_batch_q<8>, k_klt_batch_q<5>


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()        # (a copy: the table's arrays are read-only)


@pytest.fixture(scope="module")
def gpu(ctx):
    """pyramids per (image, built depth) and results per (row, layout), each made once for the module; the pyramids are freed with it"""
    import alvaar_amd
    from alvaar_amd import capi
    pyrs, results = {}, {}

    def pair(key, built):
        if (key, built) not in pyrs:
            I = K.image(key)
            h, w = I["prev"].shape
            pp, cp = alvaar_amd.Pyramid(ctx, w, h, K.WIN, built), alvaar_amd.Pyramid(ctx, w, h, K.WIN, built)
            pp.build_from_gray(_dev(I["prev"]))
            cp.build_from_gray(_dev(I["curr"]))
            assert pp.num_levels == cp.num_levels == len(pyr_dims(w, h, K.WIN, built))
            pyrs[key, built] = (pp, cp)
        return pyrs[key, built]

    def run(name, layout):
        """per case of the row: (next, status, err) for "lk", (tracked, status) for the forward-backward layouts; as numpy"""
        if (name, layout) in results:
            return results[name, layout]
        r = K.row(name)
        a, cases = r["args"], r["cases"]
        pp = [pair(c["image"], c["built"]) for c in cases]
        pts, init = [_dev(c["pts"]) for c in cases], [_dev(c["init"]) for c in cases]
        if layout == "lk":
            out = [ctx.lk_track(p[0], p[1], x, i, a["num_levels"], a["max_iters"], a["eps"]) for p, x, i in zip(pp, pts, init)]
        elif layout == "fbklt":
            out = [ctx.fbklt_track(p[0], p[1], x, i, a["num_levels"], a["err_thresh"], a["fb_dist"], a["max_iters"], a["eps"])
                   for p, x, i in zip(pp, pts, init)]
        else:
            # the cases of a row in ONE launch: three image sizes, and in the depth rows ten cameras of five pyramid depths
            tr, st = capi.fbklt_track_batch(ctx, [p[0] for p in pp], [p[1] for p in pp], pts, init, a["num_levels"], int(layout[5:]),
                                            a["err_thresh"], a["fb_dist"], a["max_iters"], a["eps"])
            ctx.sync()
            out = list(zip(tr, st))
        results[name, layout] = [tuple(t.cpu().numpy() for t in o) for o in out]
        return results[name, layout]

    yield SimpleNamespace(pair=pair, run=run)
    for pp, cp in pyrs.values():
        pp.close()
        cp.close()


def _oracles():
    return [("orc", Orc)] + ([("ref", Ref)] if ref_available() else [])


@pytest.mark.parametrize("name", K.LK_ROW_NAMES)
def test_lk_rows_bitwise(gpu, name):
    got = gpu.run(name, "lk")
    for case, g in zip(K.row(name)["cases"], got):
        for oname, O in _oracles():
            want = K.lk_result(case, O)
            assert np.array_equal(g[1], want[1]), (case["name"], oname)
            assert np.array_equal(g[0].view(np.uint32), want[0].view(np.uint32)), (case["name"], oname)
            ok = want[1].astype(bool)
            assert np.array_equal(g[2][ok].view(np.uint32), want[2][ok].view(np.uint32)), (case["name"], oname)


@pytest.mark.parametrize("layout", FB_LAYOUTS)
@pytest.mark.parametrize("name", K.ROW_NAMES)
def test_fbklt_rows_bitwise(gpu, name, layout):
    got = gpu.run(name, layout)
    for case, g in zip(K.row(name)["cases"], got):
        for oname, O in _oracles():
            want = K.fb_result(case, O)
            assert np.array_equal(g[1], want[1]), (case["name"], oname)
            assert np.array_equal(g[0].view(np.uint32), want[0].view(np.uint32)), (case["name"], oname)


@pytest.mark.parametrize("name", K.ROW_NAMES)
def test_the_four_layouts_agree(gpu, name):
    first = gpu.run(name, FB_LAYOUTS[0])
    for layout in FB_LAYOUTS[1:]:
        for case, a, b in zip(K.row(name)["cases"], first, gpu.run(name, layout)):
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (case["name"], layout)


@pytest.mark.parametrize("lanes", [64, 8, 5])
def test_batch_of_few_cameras_of_different_depth(ctx, gpu, lanes):
    """the depth rows hold ten cameras (from eight on: the camera -> XCD grid); here three of them, of three depths, on the plain grid"""
    from alvaar_amd import capi
    r = K.row("levels=7")
    cases = [c for c in r["cases"] if (c["image"], c["built"]) in (("d200", 7), ("c64", 1), ("d200", 0))]
    assert len(cases) == 3
    pp = [gpu.pair(c["image"], c["built"]) for c in cases]
    tr, st = capi.fbklt_track_batch(ctx, [p[0] for p in pp], [p[1] for p in pp], [_dev(c["pts"]) for c in cases], [_dev(c["init"]) for c in cases],
                                    7, lanes)
    ctx.sync()
    for case, t, s in zip(cases, tr, st):
        assert K.same_fb((t.cpu().numpy(), s.cpu().numpy()), K.fb_result(case)), case["name"]


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx, gpu):
    """pyramids that do not belong together -- another size, another depth, a window other than 9 -- are refused by every entry point"""
    import alvaar_amd
    from alvaar_amd import capi
    a, small, shallow = gpu.pair("a200", 3), gpu.pair("c64", 3), gpu.pair("a200", 1)
    I = K.image("a200")
    h, w = I["prev"].shape
    pts, init = _dev(I["pts"]), _dev(I["init"])
    win7 = [alvaar_amd.Pyramid(ctx, w, h, 7, 3) for _ in range(2)]
    win7[0].build_from_gray(_dev(I["prev"]))
    win7[1].build_from_gray(_dev(I["curr"]))
    assert a[0].num_levels == 4 and shallow[0].num_levels == 2 and win7[0].num_levels == 4
    for prev, curr in ((a[0], small[1]), (small[0], a[1]), (a[0], shallow[1]), (shallow[0], a[1]), (win7[0], win7[1]), (a[0], win7[1])):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.lk_track(prev, curr, pts, init, 3)
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.fbklt_track(prev, curr, pts, init, 3)
        for lanes in (64, 8, 5):
            with pytest.raises(alvaar_amd.AlvaError):     # alone, and behind a camera that is in order
                capi.fbklt_track_batch(ctx, [prev], [curr], [pts], [init], 3, lanes)
            with pytest.raises(alvaar_amd.AlvaError):
                capi.fbklt_track_batch(ctx, [a[0], prev], [a[1], curr], [pts, pts], [init, init], 3, lanes)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.lk_track(a[0], a[1], pts, init, -1)
    for p in win7:
        p.close()
    case = K.row("default")["cases"][0]
    nx, st, er = ctx.lk_track(a[0], a[1], pts, init, 3)
    assert K.same_lk((nx.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()), K.lk_result(case))
    pr, fs = ctx.fbklt_track(a[0], a[1], pts, init, 3)
    assert K.same_fb((pr.cpu().numpy(), fs.cpu().numpy()), K.fb_result(case))
    tr, bs = capi.fbklt_track_batch(ctx, [a[0]], [a[1]], [pts], [init], 3, 5)
    ctx.sync()
    assert K.same_fb((tr[0].cpu().numpy(), bs[0].cpu().numpy()), K.fb_result(case))


# ---- the pyramid's build kernels at other windows and depths ---------------------------------------------------------------------------
def _assert_levels(pyr, want, what):
    og, od = want
    assert pyr.num_levels == len(og), what
    for l in range(pyr.num_levels):
        g, d = pyr.download_level(l)
        assert np.array_equal(g, og[l]), what + (l, "gray")
        assert np.array_equal(d, od[l]), what + (l, "deriv")


def _build_every_way(ctx, w, h, win, depths):
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    frames = [pyr_frame(w, h, k) for k in range(2)]
    rgbas = [synth.gray_to_rgba(f, seed=k + 1) for k, f in enumerate(frames)]
    grays = [Orc.rgba2gray(r) for r in rgbas]
    d_frames, d_rgbas = [_dev(f) for f in frames], [_dev(r) for r in rgbas]
    for depth in depths:
        from_gray = [Orc.build_pyramid(f, win, depth) for f in frames]
        from_rgba = [Orc.build_pyramid(g, win, depth) for g in grays]
        pa, pb = alvaar_amd.Pyramid(ctx, w, h, win, depth), alvaar_amd.Pyramid(ctx, w, h, win, depth)
        assert pa.num_levels == pb.num_levels == len(pyr_dims(w, h, win, depth))
        for k in (0, 1):
            pa.build_from_gray(d_frames[k])
            _assert_levels(pa, from_gray[k], (depth, "gray", k))
        for k in (0, 1):
            pa.build_from_rgba(d_rgbas[k])
            _assert_levels(pa, from_rgba[k], (depth, "rgba", k))
        for k in (0, 1):
            copy = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            pa.build_from_rgba(d_rgbas[k], copy)
            _assert_levels(pa, from_rgba[k], (depth, "rgba+copy", k))
            assert np.array_equal(copy.cpu().numpy(), grays[k])
        for order in ((0, 1), (1, 0)):
            copies = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
            capi.build_pyramids_batch(ctx, [pa, pb], [d_rgbas[k] for k in order], copies if order[0] else None)
            for p, k, c in zip((pa, pb), order, copies):
                _assert_levels(p, from_rgba[k], (depth, "batch", k))
                assert not order[0] or np.array_equal(c.cpu().numpy(), grays[k])
        pa.close()
        pb.close()


@pytest.mark.parametrize("w,h", PYR_SIZES)
@pytest.mark.parametrize("win", PYR_WINS)
def test_pyramid_other_windows_and_depths_bit_exact(ctx, w, h, win):
    """Every build entry point -- from gray, from RGBA with and without the gray copy, the batch -- at windows 3 .. 15 and depths 0, 5, 7
    (36 x 28: the `<= win` rule cuts after one to four levels): every gray and derivative level equal to the oracle's, padding included.
    Each pyramid is built over and over, alternating between two frames, so a border left over from the frame before would show."""
    _build_every_way(ctx, w, h, win, PYR_DEPTHS)


def test_pyramid_of_eight_levels_bit_exact(ctx):
    """all the levels a pyramid can hold, at the tracker's window: 1156 x 1156 down to 10 x 10"""
    w, h, win, depth = PYR_DEEP
    assert len(pyr_dims(w, h, win, depth)) == 8
    _build_every_way(ctx, w, h, win, [depth])
