"""f2a on its gates (GPU): alva_triangulate against the oracle on the table of triangulate_cases.py, bit for bit -- statuses exact, every
double and the parallax by bits, NaN where the oracle has NaN -- and against the reference's recorded outputs of the same table."""
import numpy as np
import pytest
from pathlib import Path

import triangulate_cases as tc

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"


def _run(ctx, T, group, bvl, bvr, unpxl, unpxr, max_err):
    import torch
    d = lambda a: torch.from_numpy(np.array(a)).cuda()           # (a copy: the table's arrays are read-only)
    out = ctx.triangulate(d(T), d(group), d(bvl), d(bvr), d(unpxl), d(unpxr), tc.K, max_err)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case_id", tc.CASE_IDS)
def test_hip_matches_oracle(ctx, case_id):
    c = tc.case(case_id)
    hip, orc = _run(ctx, *tc.inputs(tc.scene(c.scene)), c.max_err), tc.oracle(case_id)
    assert np.array_equal(hip["status"], orc["status"])
    for k in tc.OUT_KEYS:
        assert tc.same_bits(hip[k], orc[k]), k


def test_hip_matches_golden(ctx):
    z = np.load(G / "triangulate_cases.npz")
    for case_id in tc.GOLDEN_IDS:
        c = tc.case(case_id)
        s, want = tc.golden_case(z, case_id)
        args = (s["T"], s["group"], s["bvl"], s["bvr"], s["unpxl"], s["unpxr"])
        assert tc.close_to_reference(_run(ctx, *args, c.max_err), want, tc.restate(*args, tc.K, c.max_err), c.max_err) is None, case_id
