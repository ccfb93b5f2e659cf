"""GPU: alva_orb_detect_and_compute_batch / alva_orb_collect_batch (the twelve _b kernels of orb.hip and k_blur7_multi) against the
CPU oracle, camera by camera.

The detector is pinned bit-exact to cv::ORB, so every comparison is an equality, the one of test_gpu_orb.py: the keypoint records in
(octave, y, x) order equal the oracle's bitwise, no descriptor row differs, no rotation was ambiguous -- and every camera's output is
also its own alva_orb_detect_and_compute's.  The camera sets are the ones the tracker's tests never build: textured frames beside
constant images (no keypoint on any level) and images with one textured corner (a few keypoints, deep levels empty), at camera counts
on both sides of alva_xcd_item's switch at 8, with the fused pyramid, with the per-level k_resize_b tail behind it (scale 2.0 x 5
levels) and with the ALVA_ORB_PYRAMID=chain launches (k_copy_level0_b), and with a capacity below what was found."""
import numpy as np
import pytest

from alvaar_amd import synth
from oracles import Orc, Ref, ref_available
from test_gpu_orb import _ambiguous
from test_oracle_vs_ref import _img, orb_key

pytestmark = pytest.mark.gpu

W, H, NF = 320, 240, 300
GEOMS = {"1.2x8": (1.2, 8), "2.0x5": (2.0, 5)}
# (kind, seed) of camera i; a batch of `count` cameras is the first `count` of them: the constant images sit at index 1 of 3, and at
# indices 1, 3 and 8 of 9
CAMERAS = [("tex", 20), ("const", 1), ("noise", 22), ("const", 2), ("corner", 27), ("tex", 25), ("noise", 26), ("corner", 28), ("const", 3)]


def _camera_image(kind, seed, w=W, h=H):
    if kind == "const":
        return np.full((h, w), 60 * seed, np.uint8)
    if kind == "corner":   # constant but for one textured 96 x 96 corner
        g = np.full((h, w), 128, np.uint8)
        g[:96, :96] = _img(96, 96, seed, noise=True)
        return g
    if kind == "bytes":    # random bytes: FAST corners even in the two rows a 96 x 64 image leaves inside the 31-pixel border
        return np.ascontiguousarray(synth.random_rgba(w, h, seed)[..., 0])
    return _img(w, h, seed, noise=kind == "noise")


def _oracle(g, nf, scale, nlevels):
    """(keypoints in (octave, y, x) order, their descriptors) of the oracle -- and of the compiled reference where it is built"""
    kp, d = Orc.orb(g, nf, scale=scale, nlevels=nlevels, fast_thr=20)
    i = orb_key(kp)
    kp, d = kp[i], d[i]
    if ref_available():
        rkp, rd = Ref.orb(g, nf, scale=scale, nlevels=nlevels, fast_thr=20)
        ri = orb_key(rkp)
        assert np.array_equal(kp.view(np.uint32), rkp[ri].view(np.uint32)) and np.array_equal(d, rd[ri])
    return kp, d


@pytest.fixture(scope="module")
def images():
    return [_camera_image(kind, seed) for kind, seed in CAMERAS]


@pytest.fixture(scope="module")
def oracle(images):
    """per geometry, per camera: the oracle's (kp, desc), computed once"""
    out = {name: [_oracle(g, NF, scale, nlevels) for g in images] for name, (scale, nlevels) in GEOMS.items()}
    for name, per_cam in out.items():
        n = {kind: [len(kp) for (k, _), (kp, _) in zip(CAMERAS, per_cam) if k == kind] for kind in ("tex", "noise", "const", "corner")}
        assert min(n["tex"] + n["noise"]) > 16 and max(n["const"]) == 0 and 0 < min(n["corner"]) and max(n["corner"]) < min(n["noise"]), (name, n)
        deepest = max(int(kp[:, 5].max()) for (k, _), (kp, _) in zip(CAMERAS, per_cam) if k == "corner")
        assert deepest < GEOMS[name][1] - 1, (name, deepest)   # the corner cameras' deep levels are empty
    return out


@pytest.fixture(scope="module")
def singles():
    """cache of every camera's own alva_orb_detect_and_compute result per (geometry, pyramid mode), filled by _single"""
    return {}


def _single(ctx, singles, images, geom, chain, i):
    """camera i through the single-camera call, on an object of its own (created under the caller's ALVA_ORB_PYRAMID)"""
    import torch
    import alvaar_amd
    if (geom, chain, i) not in singles:
        scale, nlevels = GEOMS[geom]
        orb = alvaar_amd.Orb(ctx, W, H, NF, scale=scale, nlevels=nlevels)
        singles[(geom, chain, i)] = orb.detect_and_compute(torch.from_numpy(images[i]).cuda())
        orb.close()
    return singles[(geom, chain, i)]


def _equals_oracle(got, want, where):
    kp, desc = (t.cpu().numpy() for t in got)
    rkp, rd = want
    assert len(kp) == len(rkp), (where, len(kp), len(rkp))
    assert np.array_equal(kp.view(np.uint32), rkp.view(np.uint32)), where   # ours is already in (octave, y, x) order
    assert (desc != rd).any(axis=1).sum() == 0, where


@pytest.mark.parametrize("count,chain", [(1, False), (3, False), (8, False), (9, False), (1, True), (3, True)])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_geometries_and_counts(ctx, images, oracle, singles, geom, count, chain, monkeypatch):
    """every camera of the batch equals the oracle and its own single-camera call; the second call on the same objects is the one
    compared (every buffer and counter reused).  Scale 2.0 x 5 levels leaves its deepest level to k_resize_b, chain builds level 0 with
    k_copy_level0_b and every other level with k_resize_b: the pyramid the batch built is compared byte by byte as well, and its blur."""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    if chain:
        monkeypatch.setenv("ALVA_ORB_PYRAMID", "chain")   # read at alva_orb_create
    scale, nlevels = GEOMS[geom]
    orbs = [alvaar_amd.Orb(ctx, W, H, NF, scale=scale, nlevels=nlevels) for _ in range(count)]
    grays = [torch.from_numpy(g).cuda() for g in images[:count]]
    _ambiguous()
    for rep in range(2):
        got = capi.orb_detect_and_compute_batch(ctx, orbs, grays, 4 * NF + 1024)
    for i in range(count):
        _equals_oracle(got[i], oracle[geom][i], (geom, count, chain, i))
        kp1, desc1 = _single(ctx, singles, images, geom, chain, i)
        assert torch.equal(got[i][0], kp1) and torch.equal(got[i][1], desc1), (geom, count, chain, i)
        if CAMERAS[i][0] == "const":
            assert got[i][0].shape[0] == 0
    assert _ambiguous() == 0
    for i in {0, count - 1}:
        want = Orc.orb_pyramid(images[i], scale, nlevels)
        for l, lv in enumerate(want):
            lvl = orbs[i].level(l).cpu().numpy()
            assert lvl.shape == lv.shape and np.array_equal(lvl, lv), (geom, count, chain, i, l)
            assert np.array_equal(orbs[i].level(l, blurred=True).cpu().numpy(), Orc.orb_blur(lv)), (geom, count, chain, i, "blur", l)
    for o in orbs:
        o.close()


@pytest.mark.parametrize("geom,chain,kernel", [("2.0x5", False, "k_resize_b"), ("1.2x8", True, "k_copy_level0_b"), ("1.2x8", True, "k_resize_b"),
                                               ("1.2x8", False, "k_pyramid_b")])
def test_the_geometries_launch_the_kernels_they_are_here_for(ctx, images, geom, chain, kernel, monkeypatch):
    """the library's own launch record (alva_prof_enable): which pyramid kernels a batch call of that geometry goes through"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    if chain:
        monkeypatch.setenv("ALVA_ORB_PYRAMID", "chain")
    scale, nlevels = GEOMS[geom]
    orbs = [alvaar_amd.Orb(ctx, W, H, NF, scale=scale, nlevels=nlevels) for _ in range(2)]
    grays = [torch.from_numpy(g).cuda() for g in images[:2]]
    launched = capi.kernel_times(lambda: capi.orb_detect_and_compute_batch(ctx, orbs, grays, 4 * NF + 1024), 1)
    assert kernel in launched, sorted(launched)
    assert ("k_pyramid_b" in launched) != chain and ("k_copy_level0_b" in launched) == chain, sorted(launched)
    for o in orbs:
        o.close()


def test_small_image(ctx):
    """96 x 64: only level 0 has pixels further than 31 from every border (two rows of them), every other level keeps nothing"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    w, h = 96, 64
    imgs = [_camera_image(kind, seed, w, h) for kind, seed in (("bytes", 30), ("tex", 31), ("bytes", 34))]
    want = [_oracle(g, NF, 1.2, 8) for g in imgs]
    assert [len(kp) > 0 for kp, _ in want] == [True, False, True] and all((kp[:, 5] == 0).all() for kp, _ in want)
    orbs = [alvaar_amd.Orb(ctx, w, h, NF) for _ in imgs]
    one = alvaar_amd.Orb(ctx, w, h, NF)
    grays = [torch.from_numpy(g).cuda() for g in imgs]
    _ambiguous()
    for rep in range(2):
        got = capi.orb_detect_and_compute_batch(ctx, orbs, grays, 4 * NF + 1024)
    for i, g in enumerate(grays):
        _equals_oracle(got[i], want[i], i)
        kp1, desc1 = one.detect_and_compute(g)
        assert torch.equal(got[i][0], kp1) and torch.equal(got[i][1], desc1), i
    assert _ambiguous() == 0
    for o in orbs + [one]:
        o.close()


@pytest.mark.parametrize("cap", [16, 0])
def test_capacity(ctx, images, oracle, cap):
    """a camera that finds more than cap: the first cap records and descriptors are written (the first cap of its uncapped result), the
    buffers' rows from cap on are not touched, and alva_orb_collect_batch still returns what was FOUND, as alva_orb_detect_and_compute does"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    rows, geom, count = 64, "1.2x8", 3
    orbs = [alvaar_amd.Orb(ctx, W, H, NF) for _ in range(count)]
    grays = [torch.from_numpy(g).cuda() for g in images[:count]]
    kps = [torch.full((rows, 6), -7.0, dtype=torch.float32, device="cuda") for _ in range(count)]
    descs = [torch.full((rows, 32), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(count)]
    for rep in range(2):
        capi.orb_enqueue_batch(ctx, orbs, grays, kps, descs, cap)
        counts = capi.orb_collect_batch(ctx, orbs)
    assert counts == [len(kp) for kp, _ in oracle[geom][:count]] and counts[0] > 16 and counts[1] == 0 and counts[2] > 16
    for i in range(count):
        n = min(cap, counts[i])
        kp, desc = kps[i].cpu().numpy(), descs[i].cpu().numpy()
        rkp, rd = oracle[geom][i]
        assert np.array_equal(kp[:n].view(np.uint32), rkp[:n].view(np.uint32)) and np.array_equal(desc[:n], rd[:n]), i
        assert np.array_equal(kp[n:], np.full((rows - n, 6), -7.0, np.float32)) and np.array_equal(desc[n:], np.full((rows - n, 32), 0xA5, np.uint8)), i
    for o in orbs:
        o.close()


def test_argument_errors(ctx, images):
    """each returns non-zero with a message; the checks run before the first launch"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    good = [alvaar_amd.Orb(ctx, W, H, NF) for _ in range(2)]
    other = {"another size": alvaar_amd.Orb(ctx, W, H - 40, NF), "another nlevels": alvaar_amd.Orb(ctx, W, H, NF, nlevels=7),
             "another nfeatures": alvaar_amd.Orb(ctx, W, H, 500)}
    grays = [torch.from_numpy(g).cuda() for g in images[:3]]
    kps = [torch.full((64, 6), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    descs = [torch.full((64, 32), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
    bad = {what: dict(orbs=good + [o]) for what, o in other.items()}
    bad["a NULL image"] = dict(orbs=good, grays=[grays[0], None])
    bad["count = 0"] = dict(orbs=[], grays=[], kps=[], descs=[])
    bad["gray_pitch < width"] = dict(orbs=good, gray_pitch=W - 1)
    for what, a in bad.items():
        orbs = a["orbs"]
        with pytest.raises(alvaar_amd.AlvaError, match="bad argument"):
            capi.orb_enqueue_batch(ctx, orbs, a.get("grays", grays[:len(orbs)]), a.get("kps", kps[:len(orbs)]), a.get("descs", descs[:len(orbs)]), 64,
                                   gray_pitch=a.get("gray_pitch"))
        ctx.sync()
        assert all(int((k != -7.0).sum()) == 0 for k in kps) and all(int((d != 0xA5).sum()) == 0 for d in descs), what
    for o in good + list(other.values()):
        o.close()
