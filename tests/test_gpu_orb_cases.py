"""GPU: the ORB detector's two culls at the cases of orb_cases.py -- exact Harris ties at the cut, the host's bound on kept keypoints (at
it and above it), both sides of the 4096-candidate split between cull_harris_body and cull_harris_big, both sides of the 4096-survivor
split inside cull_harris_big, n against keepN at both culls (in cull_harris_big and in cull_harris_body), levels with a zero budget, and a level with more rows than the LDS row
table -- and the plain FAST entry point on images taller than one chunk of its row scan.

Every comparison is an equality with the CPU oracle (pinned to cv::ORB on these very cases by test_orb_cases.py, which also asserts
that each case reaches its branch): the same count, the keypoint records bitwise equal to the oracle's in (octave, y, x) order WITHOUT
sorting the GPU side, no descriptor row different, no ambiguous rotation; the object is run twice and the runs are byte-identical."""
import numpy as np
import pytest

import orb_cases as oc
from oracles import Orc
from test_gpu_orb import _ambiguous

pytestmark = pytest.mark.gpu


def _run_twice(ctx, case_id):
    """the case on one detector object, twice: (kp, desc) numpy of the second run, after asserting it equals the first"""
    import torch
    import alvaar_amd
    c = oc.case(case_id)
    rkp, rd, lv = oc.oracle(case_id)
    g = oc.image(c.spec)
    h, w = g.shape
    orb = alvaar_amd.Orb(ctx, w, h, c.nf, scale=c.scale, nlevels=c.nlevels, fast_threshold=c.thr)
    gray = torch.from_numpy(np.array(g)).cuda()
    cap = max(4 * c.nf + 1024, len(rkp))
    kp1, desc1 = orb.detect_and_compute(gray, cap=cap)
    kp2, desc2 = orb.detect_and_compute(gray, cap=cap)
    assert torch.equal(kp1.view(torch.int32), kp2.view(torch.int32)) and torch.equal(desc1, desc2), case_id
    orb.close()
    return kp2.cpu().numpy(), desc2.cpu().numpy()


def _check_case(ctx, case_id):
    rkp, rd, lv = oc.oracle(case_id)
    _ambiguous()
    kp, desc = _run_twice(ctx, case_id)
    assert len(kp) == len(rkp), (case_id, len(kp), len(rkp), lv)
    same = (kp.view(np.uint32) == rkp.view(np.uint32)).all(axis=1)
    assert same.all(), (case_id, int((~same).sum()), int(np.argmin(same)), lv)   # ours is already in (octave, y, x) order
    assert (desc != rd).any(axis=1).sum() == 0, case_id
    assert _ambiguous() == 0, case_id


@pytest.mark.parametrize("case_id", [i for i in oc.CASE_IDS if i != "bound_over"])
def test_case_equals_oracle(ctx, case_id):
    _check_case(ctx, case_id)
    if case_id == "bound_at":
        assert len(oc.oracle(case_id)[0]) == 1024


def test_above_the_launch_bound_is_an_error_and_nothing_else(ctx):
    """a level that keeps more than max(4 n_l + 64, 1024): the call fails with a message that names the bound; the object then still
    fails on that image and nothing else is hurt -- a detector of the right size returns bound_at's 1024 keypoints, and the context
    a correct tie_small result"""
    import torch
    import alvaar_amd
    c = oc.case("bound_over")
    g = oc.image(c.spec)
    h, w = g.shape
    m = len(oc.oracle("bound_over")[0])
    orb = alvaar_amd.Orb(ctx, w, h, c.nf, scale=c.scale, nlevels=c.nlevels, fast_threshold=c.thr)
    gray = torch.from_numpy(np.array(g)).cuda()
    for rep in range(2):
        with pytest.raises(alvaar_amd.AlvaError, match="above the launch bound"):
            orb.detect_and_compute(gray, cap=max(4 * c.nf + 1024, m))
    ctx.sync()
    _check_case(ctx, "bound_at")
    orb.close()
    _check_case(ctx, "tie_small-300")


def test_batch_of_two_above_the_sort_cap(ctx):
    """k_cull_harris_b shares the body: two cameras of one geometry with a level budget of 4097, random bytes (4097 kept: the
    row-bucket order) beside the tiled image; each equals the oracle and its own single-camera call"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    specs = oc.batch_cases()
    _, nf, scale, nlevels = specs[0]
    want = [oc.batch_oracle(i) for i in range(len(specs))]
    cap = max(4 * nf + 1024, max(len(kp) for kp, _, _ in want))
    grays = [torch.from_numpy(np.array(oc.image(spec))).cuda() for spec, *_ in specs]
    h, w = grays[0].shape
    orbs = [alvaar_amd.Orb(ctx, w, h, nf, scale=scale, nlevels=nlevels) for _ in specs]
    one = alvaar_amd.Orb(ctx, w, h, nf, scale=scale, nlevels=nlevels)
    _ambiguous()
    for rep in range(2):
        got = capi.orb_detect_and_compute_batch(ctx, orbs, grays, cap)
    for i, (rkp, rd, lv) in enumerate(want):
        kp, desc = got[i][0].cpu().numpy(), got[i][1].cpu().numpy()
        assert len(kp) == len(rkp), (i, len(kp), len(rkp), lv)
        assert np.array_equal(kp.view(np.uint32), rkp.view(np.uint32)), (i, lv)
        assert (desc != rd).any(axis=1).sum() == 0, i
        kp1, desc1 = one.detect_and_compute(grays[i], cap=cap)
        assert torch.equal(got[i][0].view(torch.int32), kp1.view(torch.int32)) and torch.equal(got[i][1], desc1), i
    assert _ambiguous() == 0
    for o in orbs + [one]:
        o.close()


@pytest.mark.parametrize("i", [0, 1])
def test_fast_on_tall_images(ctx, i):
    """alva_fast on 2100 and 1100 rows (k_scan_rows carries the running sum over two and one chunk boundaries): positions and scores
    equal the oracle's in row-major order, and with a capacity below the count the first `cap` of that order"""
    import torch
    g = oc.tall_fast_image(i)
    rxy, rsc = Orc.fast(g, 20)
    gray = torch.from_numpy(np.array(g)).cuda()
    xy, sc = ctx.fast(gray, 20)
    assert len(rxy) > 0 and np.array_equal(xy.cpu().numpy(), rxy) and np.array_equal(sc.cpu().numpy(), rsc)
    cap = len(rxy) // 2 + 1
    xy, sc = ctx.fast(gray, 20, cap=cap)
    assert np.array_equal(xy.cpu().numpy(), rxy[:cap]) and np.array_equal(sc.cpu().numpy(), rsc[:cap])
