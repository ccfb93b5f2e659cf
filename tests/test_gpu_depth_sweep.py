"""The depth sweep (alva_depth_sweep) on the GPU against its numpy restatement tests/depth_cases.py: depth, conf, code, info and the
test output {kb, best, second, T} are EQUAL, bit for bit, for every case of the table.  Both sides do the same IEEE operations in the
same order and the costs are integers, so there is no tolerance."""
from __future__ import annotations

import numpy as np
import pytest

import depth_cases as Dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _device(img, pad):
    """the image on the device, in rows of width + pad bytes; the padding holds a value no image pixel takes part in"""
    import torch
    h, w = img.shape
    buf = torch.full((h, w + pad), 171, dtype=torch.uint8, device="cuda")
    buf[:, :w] = torch.from_numpy(np.array(img)).cuda()   # (a copy: the scenes are read-only arrays)
    return buf[:, :w]


def _gpu(ctx, c, **over):
    kw = dict(c["kw"], **over)
    return ctx.depth_sweep(_device(c["cur"], c["pad"]), _device(c["ref"], c["pad"]), c["calib8"], c["T"], c["rho"][0], c["rho"][1],
                           width=c["width"], want_best=True, **kw)


def _assert_equal(got, want):
    depth, conf, code, info, best = got
    print("gpu info", info.tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(code, want["code"])
    assert np.array_equal(best, want["best"])
    assert np.array_equal(conf, want["conf"])
    assert depth.dtype == np.float32 and np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(info, want["info"])


@pytest.mark.parametrize("name", sorted(Dc.cases()))
def test_case_equals_the_restatement_bit_for_bit(ctx, name):
    c = Dc.cases()[name]
    want = Dc.oracle_case(name)
    got = _gpu(ctx, c)
    _assert_equal(got, want)
    again = _gpu(ctx, c)   # the same inputs give the same bits
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_without_the_test_output_the_answer_is_the_same(ctx):
    c = Dc.cases()["dense_40_10_r2"]
    want = Dc.oracle_case("dense_40_10_r2")
    import torch
    got = ctx.depth_sweep(torch.from_numpy(np.array(c["cur"])).cuda(), torch.from_numpy(np.array(c["ref"])).cuda(),
                          c["calib8"], c["T"], *c["rho"], **c["kw"])
    assert len(got) == 4
    for a, key in zip(got, ("depth", "conf", "code", "info")):
        assert np.array_equal(a.view(np.uint8), want[key].view(np.uint8)), key


def test_bad_arguments_are_rejected(ctx):
    import alvaar_amd
    c = Dc.cases()["pitch_80"]
    for over in (dict(step=0), dict(step=17), dict(num_hyp=7), dict(num_hyp=257), dict(patch_radius=0), dict(patch_radius=5),
                 dict(min_texture=-1), dict(min_texture=256), dict(min_conf=-1), dict(min_conf=256)):
        with pytest.raises(alvaar_amd.AlvaError):
            _gpu(ctx, c, **over)
    for rho in ((0.5, 0.5), (0.5, 0.25), (0.0, 0.5), (-0.1, 0.5), (0.1, float("inf")), (float("nan"), 0.5)):
        with pytest.raises(alvaar_amd.AlvaError):
            _gpu(ctx, dict(c, rho=rho))
    with pytest.raises(alvaar_amd.AlvaError):
        _gpu(ctx, dict(c, width=62))   # width % 4
    _assert_equal(_gpu(ctx, c), Dc.oracle_case("pitch_80"))   # and the context is as good as before
