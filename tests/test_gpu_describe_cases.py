"""a6 at its edges (GPU): alva_orb_blur and alva_describe against the oracle on the tables of describe_cases.py -- the smallest sizes, the
images that pin rounding and ties, hostile coordinates between valid points, n around the eight keypoints of a block, pitched sources --
bit for bit, and against the reference's recorded outputs."""
import numpy as np
import pytest
from pathlib import Path

import describe_cases as dc

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"


def _pitched(g, left, right, pad):
    """the image as a column slice of a wider device tensor filled with `pad`: (slice, the wide tensor)"""
    import torch
    h, w = g.shape
    wide = torch.full((h, left + w + right), pad, dtype=torch.uint8, device="cuda")
    wide[:, left:left + w] = torch.from_numpy(g.copy()).cuda()
    return wide[:, left:left + w], wide


@pytest.mark.parametrize("case_id", dc.BLUR_IDS)
def test_orb_blur_matches_oracle(ctx, case_id):
    import torch
    g = dc.image(dc.BLUR[case_id])
    out = ctx.orb_blur(torch.from_numpy(g.copy()).cuda()).cpu().numpy()
    assert np.array_equal(out, dc.blur_oracle(case_id))
    if case_id == dc.BLUR_PITCHED:
        src, wide = _pitched(g, 5, 8, 255 - int(g[0, 0]))
        assert src.stride(0) == g.shape[1] + 13
        assert np.array_equal(ctx.orb_blur(src).cpu().numpy(), dc.blur_oracle(case_id))
        assert np.array_equal(wide.cpu().numpy()[:, 5:5 + g.shape[1]], g)


@pytest.mark.parametrize("case_id", dc.CASE_IDS)
def test_describe_matches_oracle(ctx, case_id):
    import torch
    c = dc.case(case_id)
    g, (od, ov) = dc.image(c.spec), dc.oracle(case_id)
    desc, valid = ctx.describe(torch.from_numpy(g.copy()).cuda(), torch.from_numpy(c.pts.copy()).cuda())
    assert np.array_equal(valid.cpu().numpy(), ov) and np.array_equal(desc.cpu().numpy(), od)
    if case_id == dc.PITCHED:
        src, _ = _pitched(g, 7, 2, 0)
        desc, valid = ctx.describe(src, torch.from_numpy(c.pts.copy()).cuda())
        assert np.array_equal(valid.cpu().numpy(), ov) and np.array_equal(desc.cpu().numpy(), od)
    if case_id == "hostile":                                     # stated outright, not only through the oracle
        bad = dc.hostile_rows()
        assert not valid.cpu().numpy()[bad].any() and not desc.cpu().numpy()[bad].any()


def test_hip_matches_golden(ctx):
    import torch
    z = np.load(G / "describe_cases.npz")
    for k in z["blur_ids"]:
        assert np.array_equal(ctx.orb_blur(torch.from_numpy(z[f"blur_g_{k}"]).cuda()).cpu().numpy(), z[f"blur_out_{k}"]), k
    for k in z["ids"]:
        desc, valid = ctx.describe(torch.from_numpy(z[f"g_{k}"]).cuda(), torch.from_numpy(z[f"pts_{k}"]).cuda())
        assert np.array_equal(valid.cpu().numpy(), z[f"valid_{k}"]) and np.array_equal(desc.cpu().numpy(), z[f"desc_{k}"]), k
