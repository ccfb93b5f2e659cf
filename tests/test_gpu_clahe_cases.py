"""f4a at its edges (GPU): alva_clahe against the oracle on the table of clahe_cases.py -- designed residuals, grid and size edges -- bit for
bit, from and into pitched buffers whose padding must stay untouched, after refused arguments, and against the reference's recorded outputs."""
import numpy as np
import pytest
from pathlib import Path

import clahe_cases as kc

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
ERR_ARG = -1


@pytest.mark.parametrize("case_id", kc.CASE_IDS)
def test_hip_matches_oracle(ctx, case_id):
    import torch
    c = kc.case(case_id)
    out = ctx.clahe(torch.from_numpy(kc.image(case_id).copy()).cuda(), c.clip, c.tiles)
    assert np.array_equal(out.cpu().numpy(), kc.oracle(case_id))


def _unused(g):
    """a byte value the image does not contain"""
    return int(np.flatnonzero(np.bincount(g.ravel(), minlength=256) == 0)[-1])


@pytest.mark.parametrize("case_id", kc.PITCH_IDS)
def test_pitched_source_and_destination(ctx, case_id):
    import torch
    from alvaar_amd.capi import lib, check
    c, g, want = kc.case(case_id), kc.image(case_id), kc.oracle(case_id)
    pad_s, pad_d = _unused(g), _unused(want)
    left, right = 3, 10                                          # the image starts 3 bytes into its rows: an unaligned base, too
    wide_s = torch.full((c.h, left + c.w + right), pad_s, dtype=torch.uint8, device="cuda")
    wide_s[:, left:left + c.w] = torch.from_numpy(g.copy()).cuda()
    src = wide_s[:, left:left + c.w]
    assert src.stride(0) == left + c.w + right and not src.is_contiguous()
    # pitched source through the wrapper (it passes stride(0)), contiguous destination
    assert np.array_equal(ctx.clahe(src, c.clip, c.tiles).cpu().numpy(), want)
    # pitched source and pitched destination through the entry point itself
    wide_d = torch.full((c.h, 5 + c.w + 6), pad_d, dtype=torch.uint8, device="cuda")
    dst = wide_d[:, 5:5 + c.w]
    check(lib.alva_clahe(ctx.h, src.data_ptr(), src.stride(0), c.w, c.h, float(c.clip), c.tiles[0], c.tiles[1], dst.data_ptr(), dst.stride(0)))
    got_s, got_d = wide_s.cpu().numpy(), wide_d.cpu().numpy()
    assert np.array_equal(got_d[:, 5:5 + c.w], want)
    assert (got_d[:, :5] == pad_d).all() and (got_d[:, 5 + c.w:] == pad_d).all()                  # the destination's padding is not written
    assert (got_s[:, :left] == pad_s).all() and (got_s[:, left + c.w:] == pad_s).all() and np.array_equal(got_s[:, left:left + c.w], g)


def test_refused_arguments_leave_the_context_usable(ctx):
    import torch
    from alvaar_amd.capi import lib
    case_id = "33x17-t8x8"
    c, g = kc.case(case_id), torch.from_numpy(kc.image(case_id).copy()).cuda()
    out = torch.zeros_like(g)
    call = lambda pitch, w, h, tx, ty, dpitch: lib.alva_clahe(ctx.h, g.data_ptr(), pitch, w, h, float(c.clip), tx, ty, out.data_ptr(), dpitch)
    assert call(c.w, c.w, c.h, 0, 8, c.w) == ERR_ARG             # tiles 0
    assert call(c.w, c.w, c.h, 8, 0, c.w) == ERR_ARG
    assert call(c.w, 0, c.h, 8, 8, c.w) == ERR_ARG               # width 0
    assert call(c.w, c.w, 0, 8, 8, c.w) == ERR_ARG
    assert call(c.w - 1, c.w, c.h, 8, 8, c.w) == ERR_ARG         # pitch < width
    assert call(c.w, c.w, c.h, 8, 8, c.w - 1) == ERR_ARG
    assert not out.any()                                         # nothing was launched
    assert call(c.w, c.w, c.h, 8, 8, c.w) == 0                   # and the same context takes a good call
    assert np.array_equal(out.cpu().numpy(), kc.oracle(case_id))


def test_hip_matches_golden(ctx):
    import torch
    z = np.load(G / "clahe_cases.npz")
    for cid in z["ids"]:
        out = ctx.clahe(torch.from_numpy(z[f"g_{cid}"]).cuda(), float(z[f"clip_{cid}"]), tuple(int(t) for t in z[f"tiles_{cid}"]))
        assert np.array_equal(out.cpu().numpy(), z[f"out_{cid}"]), cid
