"""The volume shift (alva_mesh_shift) on the GPU against its numpy restatement tests/mesh_shift_cases.py: q, w, the colour volume and the
four counts are EQUAL for every case of the table, with and without colour -- the one-voxel path (s_x odd, N = 4, 65, 81) and the
eight-voxel path (N and s_x multiples of 8) -- and the inputs are untouched.  Nothing is computed but integer counts, so there is no
tolerance.  Extraction and raycast then run on the shifted volume with the moved origin and equal their own restatements there."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc
import mesh_shift_cases as Sc
import raycast_cases as Rc

pytestmark = pytest.mark.gpu

CASES = Sc.cases()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def dev_volumes():
    """the table's volumes on the device, uploaded once; no test writes to them (the last test checks that)"""
    return {N: tuple(_dev(a) for a in v) for N, v in Sc.volumes().items()}


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("cid,N,s", CASES, ids=[c[0] for c in CASES])
def test_equals_the_restatement_byte_for_byte(ctx, dev_volumes, cid, N, s, color):
    q, w, c = dev_volumes[N]
    want_q, want_w, want_c, want_info = Sc.expected(N, s)
    out = ctx.mesh_shift(q, w, s, c if color else None)
    assert len(out) == (4 if color else 3)
    info = out[-1]
    want_info = want_info.copy()
    if not color:
        want_info[3] = 0
    print("gpu info", info.tolist(), "restatement", want_info.tolist())
    assert np.array_equal(info, want_info)
    got_q, got_w = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert got_q.dtype == np.int16 and np.array_equal(got_q, want_q)
    assert got_w.dtype == np.uint8 and np.array_equal(got_w, want_w)
    if color:
        got_c = out[2].cpu().numpy()
        assert got_c.dtype == np.uint8 and np.array_equal(got_c, want_c)


def test_both_paths_give_the_same_bytes(ctx, dev_volumes):
    """N = 32, s_x = 8: a lane moves 8 voxels when the arrays are aligned.  The same call on views one element into larger buffers --
    q 2 bytes, w 1 byte, c 4 bytes off -- has to take the one-voxel path, and gives the same bytes"""
    import torch
    N, s = 32, (8, -3, 16)
    q, w, c = dev_volumes[N]
    wide = ctx.mesh_shift(q, w, s, c)

    def off(t, k, fill=None):
        """a tensor of t's shape that begins k elements into a larger buffer: t's content, or `fill`"""
        buf = torch.full((t.numel() + k,), 0 if fill is None else fill, dtype=t.dtype, device=t.device)
        v = buf[k:].view(t.shape)
        if fill is None:
            v.copy_(t)
        return v

    qo, wo, co = off(q, 1), off(w, 1), off(c.view(-1), 4).view(c.shape)
    assert qo.data_ptr() % 16 == 2 and wo.data_ptr() % 8 == 1 and co.data_ptr() % 16 == 4
    outs = (off(q, 1, 77), off(w, 1, 77), off(c.view(-1), 4, 77).view(c.shape))
    narrow = ctx.mesh_shift(qo, wo, s, co, out=outs)
    for a, b in zip(wide[:3], narrow[:3]):
        assert torch.equal(a, b)
    want = Sc.shift(*Sc.volumes()[N], s)
    assert np.array_equal(wide[3], narrow[3]) and np.array_equal(wide[3], want[3])
    for a, b in zip(wide[:3], want[:3]):
        assert np.array_equal(a.cpu().numpy(), b)


def test_overlap_and_bad_arguments_are_refused(ctx, dev_volumes):
    import torch
    from alvaar_amd import AlvaError
    N = 8
    q, w, c = (t.clone() for t in dev_volumes[N])
    n = N * N * N
    fresh = lambda: (torch.empty_like(q), torch.empty_like(w), torch.empty_like(c))
    big_q, big_w = torch.zeros(2 * n, dtype=torch.int16, device="cuda"), torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    calls = [
        lambda: ctx.mesh_shift(q, w, (1, 0, 0), out=(q, fresh()[1])),                      # q onto itself
        lambda: ctx.mesh_shift(q, w, (1, 0, 0), out=(fresh()[0], w)),                      # w onto itself
        lambda: ctx.mesh_shift(q, w, (0, 0, 0), c, out=(fresh()[0], fresh()[1], c)),       # c onto itself
        lambda: ctx.mesh_shift(big_q[:n].view(N, N, N), w, (0, 0, 1), out=(big_q[n // 2:n // 2 + n].view(N, N, N), fresh()[1])),   # partial
        lambda: ctx.mesh_shift(q, big_w[1:n + 1].view(N, N, N), (0, 0, 1), out=(fresh()[0], big_w[n:2 * n].view(N, N, N))),        # one byte
        lambda: ctx.mesh_shift(q, w, (0, 0, 1), out=(big_q[:n].view(N, N, N), big_q[:n // 2].view(torch.uint8).view(N, N, N))),    # two outputs
        lambda: ctx.mesh_shift(q[:3, :3, :3].contiguous(), w[:3, :3, :3].contiguous(), (0, 0, 0)),                               # N = 3
    ]
    before = (q.clone(), w.clone(), c.clone())
    for k, call in enumerate(calls):
        with pytest.raises(AlvaError):
            call()
            pytest.fail(f"call {k} was accepted")
    for a, b in zip((q, w, c), before):
        assert torch.equal(a, b)
    # adjacent, not overlapping: accepted; and the context is usable after a rejected argument
    out = ctx.mesh_shift(big_q[:n].view(N, N, N), w, (1, 2, 3), out=(big_q[n:].view(N, N, N), big_w[:n].view(N, N, N)))
    want = Sc.shift(np.zeros((N, N, N), np.int16), w.cpu().numpy(), None, (1, 2, 3))
    assert np.array_equal(out[1].cpu().numpy(), want[1]) and np.array_equal(out[2], want[3])


@pytest.mark.parametrize("s", [(3, -5, 8), (-8, 16, 0)])
def test_extract_and_raycast_run_on_the_shifted_volume(ctx, s):
    """the analytic sphere at N = 32, shifted on the device; the moved origin is o + s voxel.  The extraction and the raycast (world rays)
    of the shifted device volume equal their restatements on the restated shift; the extraction also equals the unshifted one's
    vertices in the overlap (tests/test_mesh_shift_cases.py shows why, on the CPU).  Nothing bitwise is claimed against the unshifted
    raycast: the ray's clip box moves, and its samples with it"""
    N = 32
    q, w, origin, voxel = Mc.sampled(N, Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R))
    q2, w2, info = ctx.mesh_shift(_dev(q), _dev(w), s)
    rq, rw, _, rinfo = Sc.shift(q, w, None, s)
    assert np.array_equal(info, rinfo) and np.array_equal(q2.cpu().numpy(), rq) and np.array_equal(w2.cpu().numpy(), rw)
    origin2 = origin + np.asarray(s, np.float64) * voxel
    v, nrm, tri, xinfo = ctx.mesh_extract(q2, w2, origin2, voxel, 1, 1 << 16, 1 << 17)
    want = Mc.extract(rq, rw, origin2, voxel, 1, 1 << 16, 1 << 17)
    assert np.array_equal(xinfo, want["info"]) and xinfo[0] == 0 and xinfo[1] > 100
    assert np.array_equal(v.view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(nrm.view(np.uint32), want["normals"].view(np.uint32))
    assert np.array_equal(tri, want["triangles"])
    base = Mc.extract(q, w, origin, voxel, 1, 1 << 16, 1 << 17)
    p = base["cells"] - np.asarray(s)
    keep = np.all((p >= 0) & (p <= N - 2), axis=1)
    assert np.array_equal(base["vertices"][keep].view(np.uint32), v.view(np.uint32))
    rays = Rc.hashed_rays(256, 11)
    got = ctx.mesh_raycast(q2, w2, origin2, voxel, 1, _dev(rays))
    ref = Rc.raycast(rq, rw, origin2, voxel, 1, rays)
    print("raycast info", got["info"].tolist())
    assert np.array_equal(got["info"], ref["info"]) and got["info"][1] > 0
    assert np.array_equal(got["code"], ref["code"])
    for k in ("t", "point", "normal"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32))


def test_the_inputs_were_never_written(dev_volumes):
    """runs last in this module: after every case above the shared device volumes still hold the table's bytes"""
    for N, (q, w, c) in dev_volumes.items():
        hq, hw, hc = Sc.volumes()[N]
        assert np.array_equal(q.cpu().numpy(), hq) and np.array_equal(w.cpu().numpy(), hw) and np.array_equal(c.cpu().numpy(), hc)
