"""alva_image_homography on the GPU against its numpy restatement tests/image_cases.py: H, info, the mask, R and t, bit for bit.

Both sides work in IEEE float64 in the same written order (no contraction, correctly rounded division and square root), so nothing is
toleranced: the arrays' bytes are compared, signs of zeros included.  The launches are image_cases.launches(): the sizes m = 0, 3, 4, 5,
64, 65, 512, the iteration counts around the wave and the lane stripe up to 4096, hashed words and explicit ones, the threshold edge, the
skip and tie rules, every code, 70 % clutter, and eight pictures of different sizes in one launch."""
from __future__ import annotations

import numpy as np
import pytest

import image_cases as IC

pytestmark = pytest.mark.gpu

LAUNCHES = IC.launches()


def _upload(images):
    import torch
    n = len(images)
    xy = np.full((n, IC.QUERY_CAP, 4), np.nan)   # rows past an image's count must not be read
    count = np.zeros(n, np.int32)
    for j, (pairs, _) in enumerate(images):
        count[j] = len(pairs)
        xy[j, :len(pairs)] = pairs
    return torch.from_numpy(xy).cuda(), torch.from_numpy(count).cuda()


def _same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, got.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.reshape(-1).view(np.uint8 if got.itemsize == 1 else f"u{got.itemsize}") !=
                         want.reshape(-1).view(np.uint8 if got.itemsize == 1 else f"u{got.itemsize}"))[0]
        raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[:8]}: {got.reshape(-1)[bad[:8]]} != {want.reshape(-1)[bad[:8]]}")


@pytest.mark.parametrize("launch", LAUNCHES, ids=[L["name"] for L in LAUNCHES])
def test_all_outputs_equal_the_restatement_bit_for_bit(ctx, launch):
    xy, count = _upload(launch["images"])
    H, info, mask, R, t = ctx.image_homography(xy, count, [wh for _, wh in launch["images"]], launch["frame"], launch["calib"],
                                               num_iterations=launch["iterations"], threshold_px=launch["thr"],
                                               min_inliers=launch["min_inliers"], seed=launch["seed"], rand4=launch["rand4"])
    want = IC.run_launch(launch)
    for j, w in enumerate(want):
        print(launch["name"], j, info[j].tolist(), w["info"].tolist())
        assert info[j].tolist() == w["info"].tolist(), j
        _same_bits(f"mask[{j}]", mask[j], w["mask"])
        _same_bits(f"H[{j}]", H[j], w["H"])
        _same_bits(f"R[{j}]", R[j], w["R"])
        _same_bits(f"t[{j}]", t[j], w["t"])
    for j, code in enumerate(launch["expect"] or []):
        assert code is None or info[j, 0] == code, j


def test_a_count_above_the_cap_is_clamped_and_a_negative_one_is_empty(ctx):
    import torch
    pairs = IC.planted_scene(IC.QUERY_CAP, 0.3, 5, noise_px=0.5)[0]
    xy = torch.from_numpy(np.stack([pairs, pairs])).cuda()
    count = torch.tensor([IC.QUERY_CAP + 1000, -7], dtype=torch.int32).cuda()
    H, info, mask, R, t = ctx.image_homography(xy, count, [IC.WH, IC.WH], IC.FRAME, IC.CALIB)
    want = IC.homography_oracle(pairs, IC.WH, IC.FRAME, IC.CALIB)
    assert info[0].tolist() == want["info"].tolist() and info[0][1] == IC.QUERY_CAP
    _same_bits("H", H[0], want["H"])
    _same_bits("mask", mask[0], want["mask"])
    assert info[1].tolist() == [1, 0, -1, 0, 0, 0, 0, 0] and not mask[1].any() and not H[1].any()


def test_identical_calls_give_identical_bytes_and_arguments_are_checked(ctx):
    import alvaar_amd
    launch = LAUNCHES[-1]
    xy, count = _upload(launch["images"])
    whs = [wh for _, wh in launch["images"]]
    a = ctx.image_homography(xy, count, whs, launch["frame"], launch["calib"], 300, 3.0, 12, 99)
    b = ctx.image_homography(xy, count, whs, launch["frame"], launch["calib"], 300, 3.0, 12, 99)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for bad in (dict(num_iterations=0), dict(num_iterations=4097), dict(threshold_px=-1.0)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.image_homography(xy, count, whs, launch["frame"], launch["calib"], **bad)
