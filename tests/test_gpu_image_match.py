"""alva_image_match on the GPU against its numpy restatement tests/image_cases.py: the pairs, their coordinates and the counts, bit for
bit.  The launches are image_cases.match_launches(): query counts 0, 1, 63, 64, 65, 255, 257, 512, frame counts 0, 1 (second = 257), 2,
257, 2048 and a device count above the capacity (and a negative one), a distance tie on two train rows, best == max_dist, best == ratio *
second exactly, two and three queries claiming one row at equal distance, and eight pictures of different sizes in one call."""
from __future__ import annotations

import numpy as np
import pytest

import image_cases as IC

pytestmark = pytest.mark.gpu

LAUNCHES = IC.match_launches()


def _gpu(ctx, launch):
    import torch
    qdesc, qxy, nq = IC.pack_images(launch["images"])
    tdesc = torch.from_numpy(launch["tdesc"]).cuda() if len(launch["tdesc"]) else torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    txy = torch.from_numpy(launch["txy"]).cuda() if len(launch["txy"]) else torch.zeros((0, 2), dtype=torch.float32, device="cuda")
    n_train = torch.tensor([launch["n_train"]], dtype=torch.int32).cuda()
    match, xy, count = ctx.image_match(torch.from_numpy(qdesc).cuda(), torch.from_numpy(qxy).cuda(), nq, tdesc, txy, n_train,
                                       max_dist=launch["max_dist"], ratio=launch["ratio"])
    ctx.sync()
    return match.cpu().numpy(), xy.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("launch", LAUNCHES, ids=[L["name"] for L in LAUNCHES])
def test_pairs_coordinates_and_counts_equal_the_restatement(ctx, launch):
    match, xy, count = _gpu(ctx, launch)
    want = IC.run_match_launch(launch)
    print(launch["name"], count.tolist(), [len(m) for m, _ in want])
    assert count.tolist() == [len(m) for m, _ in want]
    for j, (wm, wxy) in enumerate(want):
        k = len(wm)
        assert np.array_equal(match[j, :k], wm), j
        assert xy[j, :k].tobytes() == wxy.tobytes(), j
        assert not match[j, k:].any() and not xy[j, k:].any(), j   # rows past the count are not written
    if launch["expect"] is not None:
        got = {int(q): int(t) for q, t, _ in match[0, :count[0]]}
        assert got == {q: t for q, t in launch["expect"].items() if t is not None}


def test_the_result_feeds_the_homography_stage_without_a_host_wait_between(ctx):
    """the two stages queued back to back: the second reads the first's counts and coordinates on the device"""
    launch = next(L for L in LAUNCHES if L["name"] == "eight")
    import torch
    qdesc, qxy, nq = IC.pack_images(launch["images"])
    n_train = torch.tensor([launch["n_train"]], dtype=torch.int32).cuda()
    match, xy, count = ctx.image_match(torch.from_numpy(qdesc).cuda(), torch.from_numpy(qxy).cuda(), nq, torch.from_numpy(launch["tdesc"]).cuda(),
                                       torch.from_numpy(launch["txy"]).cuda(), n_train)
    whs = [(256, 192)] * len(nq)
    H, info, mask, R, t = ctx.image_homography(xy, count, whs, IC.FRAME, IC.CALIB, 64, 3.0, 20, 7)
    for j, (_, wxy) in enumerate(IC.run_match_launch(launch)):
        want = IC.homography_oracle(wxy, whs[j], IC.FRAME, IC.CALIB, 64, 3.0, 20, 7)
        assert info[j].tolist() == want["info"].tolist(), j
        assert H[j].tobytes() == want["H"].tobytes() and mask[j].tobytes() == want["mask"].tobytes(), j


def test_arguments_are_checked(ctx):
    import alvaar_amd
    import torch
    launch = LAUNCHES[0]
    qdesc, qxy, nq = IC.pack_images(launch["images"])
    args = (torch.from_numpy(qdesc).cuda(), torch.from_numpy(qxy).cuda())
    tdesc, txy = torch.from_numpy(launch["tdesc"]).cuda(), torch.from_numpy(launch["txy"]).cuda()
    n_train = torch.tensor([5], dtype=torch.int32).cuda()
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.image_match(*args, np.full(len(nq), IC.QUERY_CAP + 1), tdesc, txy, n_train)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.image_match(*args, nq, tdesc, txy, n_train, ratio=-0.5)
    big = torch.zeros((IC.TRAIN_CAP + 1, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.image_match(*args, nq, big, torch.zeros((IC.TRAIN_CAP + 1, 2), dtype=torch.float32, device="cuda"), n_train)
