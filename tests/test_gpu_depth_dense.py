"""The dense depth stages (alva_depth_fuse, alva_depth_fill) on the GPU against their numpy restatement tests/dense_cases.py: state, src,
depth, level and info are EQUAL, bit for bit, for every case of the two tables.  Both sides do the same IEEE operations in the same order
and every other sum is an integer sum, so there is no tolerance."""
from __future__ import annotations

import numpy as np
import pytest

import dense_cases as Dn

pytestmark = pytest.mark.gpu




def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_fuse(ctx, c, **over):
    c = dict(c, **{k: v for k, v in over.items() if k in c})
    kw = dict(c["kw"], **{k: v for k, v in over.items() if k not in c})
    prev = None if c["prev"] is None else tuple(_dev(a) for a in c["prev"])
    meas = None if c["meas"] is None else tuple(_dev(a) for a in c["meas"])
    return ctx.depth_fuse(prev, c["T"], c["calib8"], c["width"], c["height"], c["step"], meas, **kw)


def _image(img, pad):
    """the image on the device, in rows of width + pad bytes; the padding holds a value no image pixel takes part in"""
    import torch
    h, w = img.shape
    buf = torch.full((h, w + pad), 171, dtype=torch.uint8, device="cuda")
    buf[:, :w] = torch.from_numpy(np.array(img)).cuda()
    return buf[:, :w]


def _gpu_fill(ctx, c, **over):
    c = dict(c, **over)
    return ctx.depth_fill(_dev(c["rho"]), _dev(c["w"]), _image(c["gray"], c["pad"]), c["step"], c["rho_ref"], c["max_level"], width=c["width"])


def _assert_fuse(got, want):
    rho, w, src, info = got
    print("gpu info", info.tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(src, want["src"])
    assert np.array_equal(w, want["w"])
    assert rho.dtype == np.float32 and np.array_equal(rho.view(np.uint32), want["rho"].view(np.uint32))
    assert np.array_equal(info, want["info"])


def _assert_fill(got, want):
    depth, level, info = got
    print("gpu info", info.tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(level, want["level"])
    assert depth.dtype == np.float32 and np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(info, want["info"])


@pytest.mark.parametrize("name", sorted(Dn.fuse_cases()))
def test_fuse_equals_the_restatement_bit_for_bit(ctx, name):
    c = Dn.fuse_cases()[name]
    got = _gpu_fuse(ctx, c)
    _assert_fuse(got, Dn.oracle_fuse(name))
    again = _gpu_fuse(ctx, c)   # the same inputs give the same bits, in whatever order the sources arrive
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", sorted(Dn.fill_cases()))
def test_fill_equals_the_restatement_bit_for_bit(ctx, name):
    c = Dn.fill_cases()[name]
    got = _gpu_fill(ctx, c)
    _assert_fill(got, Dn.oracle_fill(name))
    again = _gpu_fill(ctx, c)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_fuse_then_fill_of_the_fused_state(ctx):
    """the two stages in a row on device buffers, as the system call chains them"""
    import torch
    c = Dn.fuse_cases()["scene_10_to_40"]
    want = Dn.oracle_fuse("scene_10_to_40")
    rho, w, src, info = _gpu_fuse(ctx, c)
    import depth_cases as Dc
    img = Dc.two_depth_frame(40)[0]
    got = ctx.depth_fill(torch.from_numpy(rho).cuda(), torch.from_numpy(w).cuda(), _image(img, 0), 4, 2.0 / 1.5, 5)
    _assert_fill(got, Dn.fill(want["rho"], want["w"], img, 4, 2.0 / 1.5, 5))


def test_bad_arguments_are_rejected(ctx):
    import alvaar_amd
    c = Dn.fuse_cases()["identity_16x16"]
    for over in (dict(step=0), dict(step=17), dict(decay=-1), dict(decay=257), dict(w_max=0), dict(w_max=256), dict(rel_tol=0.0),
                 dict(rel_tol=-0.1), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(width=0), dict(height=0), dict(width=3),
                 dict(T=np.full(12, np.nan)), dict(calib8=(0.0, 58.0, 32.0, 32.0, 0, 0, 0, 0))):
        with pytest.raises(alvaar_amd.AlvaError):
            _gpu_fuse(ctx, c, **over)
    _assert_fuse(_gpu_fuse(ctx, c), Dn.oracle_fuse("identity_16x16"))   # and the context is as good as before
    f = Dn.fill_cases()["width60_step8"]
    for over in (dict(step=0), dict(step=17), dict(max_level=0), dict(max_level=9), dict(rho_ref=0.0), dict(rho_ref=-1.0),
                 dict(rho_ref=float("nan")), dict(rho_ref=float("inf"))):
        with pytest.raises(alvaar_amd.AlvaError):
            _gpu_fill(ctx, f, **over)
    _assert_fill(_gpu_fill(ctx, f), Dn.oracle_fill("width60_step8"))
