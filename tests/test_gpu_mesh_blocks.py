"""The block stages (alva_mesh_block_digest, alva_mesh_extract_blocks) on the GPU against their numpy restatement
tests/mesh_block_cases.py: digests, counts, ranges, info, vertices and normals (as uint32) and triangles are EQUAL, bit for bit -- for
volumes smaller than a block, of one block, with partial border blocks and of more than a thousand blocks, the three block sizes,
aligned, unaligned and negative lattices, weights on both sides of min_weight; for selections of none, one, every second and all
blocks; at the caps exactly and one below.  Refused selections are ALVA_ERR_ARG and leave the context usable; the volume is never
written.  Both sides do the same IEEE operations in the same order and every other sum is an integer sum, so there is no tolerance."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import mesh_block_cases as Bc
import mesh_cases as Mc

pytestmark = pytest.mark.gpu

BIG = 1 << 21


@functools.lru_cache(maxsize=None)
def volume(name):
    """(q, w, origin3, voxel, min_weight), read-only"""
    if name == "n4":
        q, w = Mc.hashed_volume(4, 71, -3000, 3000, 4)
        w[1:, 1:, :] = np.maximum(w[1:, 1:, :], 2)   # (enough valid voxels for a surface)
        out = (q, w, np.array([0.5, -0.25, 3.0]), 0.125, 2)
    elif name == "n8":
        out = (*Mc.sampled(8, Mc.box_dist((-0.52, -0.4, -0.33), (0.47, 0.55, 0.41))), 1)
    elif name == "n16":
        out = (*Mc.sampled(16, Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R)), 1)
    elif name == "n17":
        out = (*Mc.sampled(17, Mc.sphere_dist((-0.8, 0.7, -0.9), 0.7)), 1)   # touches the border
    elif name == "n20_hashed":
        q, w = Mc.hashed_volume(20, 61, -3000, 3000, 5)   # weights 0..5 around min_weight 3
        out = (q, w, np.array([0.3, -0.2, 0.1]), 0.07, 3)
    elif name == "n32":
        r = Mc.e2e_run()
        out = (r["q"], r["w"], r["origin3"], r["voxel"], 2)
    else:
        c = Mc.scan_case()
        out = (c["q"], c["w"], c["origin3"], c["voxel"], 1)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _cases():
    out = []
    for name in ("n4", "n8", "n16", "n17", "n20_hashed", "n32", "n65"):
        for B in Bc.BLOCKS:
            lattices = Bc.LATTICES if name != "n65" else ((3, 3, 3), (5, -13, 40))
            if name == "n4":
                lattices = ((6, 6, 6),) + Bc.LATTICES   # straddles two blocks of 8 per axis
            for lat in lattices:
                if name in ("n32", "n20_hashed") and B == 32 and lat in ((3, 3, 3), (-8, -8, -8)):
                    continue   # (nothing the other lattices do not reach)
                out.append(pytest.param(name, B, lat, id="%s-B%d-L%d_%d_%d" % (name, B, *lat)))
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_packed(got, want, what):
    print(what, "gpu info", got["info"].tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(got["info"], want["info"]), what
    assert np.array_equal(got["ranges"], want["ranges"]), what
    for f in ("vertices", "normals"):
        assert got[f].dtype == np.float32 and got[f].shape == want[f].shape, what
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f)
    assert got["triangles"].dtype == np.int32 and np.array_equal(got["triangles"], want["triangles"]), what


@pytest.mark.parametrize("name,B,lattice", _cases())
def test_stages_equal_the_restatement_bit_for_bit(ctx, name, B, lattice):
    q, w, o, vx, mw = volume(name)
    N = q.shape[0]
    dq, dw = _dev(q), _dev(w)
    keys = Bc.block_keys(N, lattice, B)
    if name == "n4" and lattice == (6, 6, 6) and B == 8:
        assert len(keys) == 8
    blocks = [Bc.block_mesh(q, w, o, vx, lattice, mw, B, key) for key in keys]
    digest, counts, nb3 = ctx.mesh_block_digest(dq, dw, lattice, mw, B)
    print("blocks", len(keys), "present", sum(b["nq"] > 0 for b in blocks))
    assert nb3.tolist() == Bc.grid(N, lattice, B)[1].tolist()
    assert digest.dtype == np.uint64 and np.array_equal(digest, np.array([b["digest"] for b in blocks], np.uint64))
    assert np.array_equal(counts, np.array([(b["nv"], b["nq"]) for b in blocks], np.int32).reshape(-1, 2))
    present = [n for n, b in enumerate(blocks) if b["nq"] > 0]
    one = present[len(present) // 2:len(present) // 2 + 1] or [len(keys) // 2]
    for what, sel in (("all", list(range(len(keys)))), ("none", []), ("one", one), ("every second", list(range(0, len(keys), 2)))):
        want = Bc.pack_blocks([blocks[n] for n in sel], N, B, BIG, BIG)
        got = ctx.mesh_extract_blocks(dq, dw, o, vx, lattice, mw, B, keys[sel].reshape(-1, 3), BIG, BIG)
        _assert_packed(got, want, what)
    # the caps: exact, one below
    full = Bc.pack_blocks(blocks, N, B, BIG, BIG)
    nv, nt = int(full["info"][1]), int(full["info"][2])
    if nt > 0:
        for what, caps in (("caps exact", (nv, nt)), ("vertices over", (nv - 1, nt)), ("triangles over", (nv, nt - 1))):
            _assert_packed(ctx.mesh_extract_blocks(dq, dw, o, vx, lattice, mw, B, keys, *caps), Bc.pack_blocks(blocks, N, B, *caps), what)
    # again: the same answer; and nothing was written into the volume
    again = ctx.mesh_block_digest(dq, dw, lattice, mw, B)
    assert np.array_equal(again[0], digest) and np.array_equal(again[1], counts)
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dw.cpu().numpy(), w)


def test_refused_selections_leave_the_context_usable(ctx):
    from alvaar_amd import capi
    q, w, o, vx, mw = volume("n17")
    dq, dw = _dev(q), _dev(w)
    lattice, B = (3, 3, 3), 8
    keys = Bc.block_keys(17, lattice, B)
    want = Bc.extract_blocks(q, w, o, vx, lattice, mw, B, keys, BIG, BIG)
    bad = [("unsorted", keys[[1, 0]]), ("unsorted in z", keys[[len(keys) - 1, 0]]), ("duplicate", keys[[2, 2]]), ("below the grid", keys[[0]] - (0, 0, 1)),
           ("beyond the grid", keys[[-1]] + (1, 0, 0)), ("more than the grid", np.concatenate([keys, keys[-1:] + (1, 0, 0)]))]
    for what, sel in bad:
        with pytest.raises(Bc.Refused):
            Bc.check_selection(17, lattice, B, sel)
        with pytest.raises(capi.StageError) as e:
            ctx.mesh_extract_blocks(dq, dw, o, vx, lattice, mw, B, sel, BIG, BIG)
        assert e.value.rc == capi.StageError.ERR_ARG, what
        _assert_packed(ctx.mesh_extract_blocks(dq, dw, o, vx, lattice, mw, B, keys, BIG, BIG), want, "after " + what)
    for args in ((lattice, mw, 12), (lattice, 0, 8), (lattice, 256, 8), (((1 << 30) + 1, 0, 0), mw, 8), ((0, -(1 << 30) - 1, 0), mw, 8)):
        with pytest.raises(capi.StageError) as e:
            ctx.mesh_block_digest(dq, dw, *args)
        assert e.value.rc == capi.StageError.ERR_ARG
    got = ctx.mesh_block_digest(dq, dw, lattice, mw, B)
    assert np.array_equal(got[0], np.array([b["digest"] for b in want["blocks"]], np.uint64))
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dw.cpu().numpy(), w)


def test_far_lattices_keep_the_bytes(ctx):
    """a lattice near the ends of its range: the keys are large, the digests, counts and meshes those of the same boxes near zero"""
    q, w, o, vx, mw = volume("n16")
    dq, dw = _dev(q), _dev(w)
    B = 16
    near = ctx.mesh_block_digest(dq, dw, (-9, 5, 0), mw, B)
    for far in ((1 << 30) - 16, -(1 << 30)):
        lattice = (far - 9, far + 5, far)   # the same remainders mod 16
        if max(abs(v) for v in lattice) > 1 << 30:
            lattice = (far + 7, far + 5, far)
            near = ctx.mesh_block_digest(dq, dw, (7, 5, 0), mw, B)
        got = ctx.mesh_block_digest(dq, dw, lattice, mw, B)
        for a, b in zip(got, near):
            assert np.array_equal(a, b)
        keys = Bc.block_keys(16, lattice, B)
        _assert_packed(ctx.mesh_extract_blocks(dq, dw, o, vx, lattice, mw, B, keys, BIG, BIG), Bc.extract_blocks(q, w, o, vx, lattice, mw, B, keys, BIG, BIG),
                       "far %d" % far)
