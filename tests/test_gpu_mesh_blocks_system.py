"""The mesh in blocks through the system surface (alva_system_mesh_blocks, alva_system_reset_mesh_blocks; AlvaAR.meshBlocks /
resetMeshBlocks) on the stream of tests/test_gpu_mesh_follow_system.py with its settings -- resolution 32, rel_extent 1, a follow block
of 2 voxels, so that unaligned lattices occur -- and once with a follow block of 8 and mesh colour.  Every call equals G1 - G6 restated
(tests/mesh_block_cases.py: BlockList) over the two stages replayed on the volume alva_system_debug_mesh_update handed back, with the
session's own offset as the lattice; welded by cell the ALL answer is mesh() of the same frame; a call on an unchanged volume reports
nothing; after meshMove by a block, state 4 appears for exactly the keys that left and no block whose box lies in both cubes is
reported; an over-cap call followed by one with room gives what a single call gives; resetMesh moves the epoch; the colours are
meshColorAt on the returned vertices; and a session that asks on every frame tracks, and answers mesh(), meshDepth, depthImage and
depthDense, bit for bit like one that never asks."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import mesh_block_cases as Bc
import mesh_cases as Mc
import mesh_shift_cases as Sc
import test_gpu_mesh_system as Ms
from test_gpu_mesh_follow_system import frames  # noqa: F401  (the stream, as a fixture)

pytestmark = pytest.mark.gpu

W, H, CELL = Ms.W, Ms.H, Ms.CELL
STEP, RES, EVERY, EXTENT = Ms.STEP, Sc.STREAM_RES, Sc.STREAM_EVERY, Sc.STREAM_EXTENT
KW = dict(resolution=RES, rel_extent=EXTENT, step=STEP)
CAPS = dict(max_blocks=4096, **Ms.CAPS)
MW, B = 2, 8
BIG = 1 << 20


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Twin:
    """the restated list beside a session, fed by the stages replayed on the test's copy of the volume"""

    def __init__(self, ctx, ar):
        self.ctx, self.ar, self.L, self.gen, self.vol = ctx, ar, Bc.BlockList(), 0, None

    def volume(self, info, offset):
        """after a debug update that integrated: the volume it handed back, where it lies and its offset"""
        self.gen += int(info["placed"])
        self.vol = dict(q=info["q"], w=info["w"], dq=_dev(info["q"]), dw=_dev(info["w"]), origin=info["origin"].copy(), voxel=info["voxel"],
                        offset=tuple(int(v) for v in offset))

    def call(self, all_=False, colors=False, block=B, min_weight=MW, **caps):
        """one meshBlocks call beside the restatement -> (the session's answer, the list of what differs)"""
        caps = dict(CAPS, **caps)
        got = self.ar.meshBlocks(min_weight=min_weight, block=block, all=all_, colors=colors, **caps)
        bad = []
        if self.vol is None:   # G1
            if got["info"]["status"] != 5 or got["info"]["blocks"] != 0 or len(got["keys"]) or got["lattice"].any():
                bad.append("no volume")
            return got, bad
        v = self.vol
        digest, counts, _ = self.ctx.mesh_block_digest(v["dq"], v["dw"], v["offset"], min_weight, block)   # G3
        info, reports = self.L.call(self.gen, min_weight, block, all_, caps["max_blocks"], caps["max_vertices"], caps["max_triangles"], RES,
                                    v["offset"], digest, counts)
        gi = got["info"]
        if [gi[k] for k in ("status", "blocks", "vertices", "triangles", "gone", "epoch", "present", "block")] != info:
            bad.append("info %s != %s" % (gi, info))
        if got["lattice"].tolist() != list(v["offset"]):
            bad.append("lattice")
        if not np.array_equal(got["geometry"]["origin"].view(np.uint64), v["origin"].view(np.uint64)) or got["geometry"]["voxel"] != v["voxel"]:
            bad.append("geometry")
        if info[0] == 3:   # G5: nothing handed out
            if len(got["keys"]) or len(got["vertices"]) or len(got["triangles"]):
                bad.append("written over a cap")
            return got, bad
        if got["keys"].tolist() != [list(r[0]) for r in reports] or got["state"].tolist() != [r[1] for r in reports]:
            bad.append("keys or states")
            return got, bad
        if got["ranges"].tolist() != [list(r[2:6]) for r in reports] or got["digest"].tolist() != [r[6] for r in reports]:
            bad.append("ranges or digests")
        sel = np.array([r[0] for r in reports if r[1] < 3], np.int32).reshape(-1, 3)   # G6
        want = self.ctx.mesh_extract_blocks(v["dq"], v["dw"], v["origin"], v["voxel"], v["offset"], min_weight, block, sel, BIG, BIG)
        if len(sel) and not np.array_equal(want["ranges"], got["ranges"][:len(sel)]):
            bad.append("the stage's ranges")
        for f in ("vertices", "normals", "triangles"):
            if got[f].shape != want[f].shape or got[f].tobytes() != want[f].tobytes():
                bad.append(f)
        if colors and len(got["vertices"]):
            rgba = self.ar.meshColorAt(got["vertices"])[0]
            if not np.array_equal(got["colors"], rgba):
                bad.append("colors")
            if not got["colors"][:, 3].any():
                bad.append("no vertex has a colour")
        return got, bad


def _session(name, **kw):
    from alvaar_amd.system import AlvaAR
    return AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True, **kw)


@pytest.fixture(scope="module")
def runs(ctx, frames):  # noqa: F811
    """the same frames through two sessions that follow with a block of 2, update on every fifth frame and answer depthImage, depthDense
    and -- after an update -- mesh() and meshDepth(): one also asks for meshBlocks on EVERY frame (ALL on every seventh), one never does"""
    out = {}
    for name in ("blocks", "never"):
        ar = _session(name, mesh_follow=Sc.STREAM_BLOCK)
        twin = _Twin(ctx, ar)
        rec, calls = [], []
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            raw = ar.depthImage(step=STEP)
            dense = ar.depthDense(step=STEP, max_level=5)
            r = [st, ar.pose7()[0].copy(), ar._pose.copy(), [a.copy() for a in raw[:3]], [a.copy() for a in dense[:4]], None]
            updated = False
            if k % EVERY == 0:
                info = ar.meshUpdate(debug=True, **KW)
                if info["status"] == 0:
                    updated = True
                    twin.volume(info, ar.meshFollowStats()["offset"])
                    mesh = ar.mesh(**Ms.CAPS)
                    depth = ar.meshDepth(step=STEP)
                    r[5] = [info["q"], info["w"], mesh[0], mesh[1], mesh[2]] + [np.asarray(a) for a in depth[:3]]
            if name == "blocks":
                got, bad = twin.call(all_=k % 7 == 0)
                calls.append(dict(frame=k, updated=updated, all=k % 7 == 0, got=got, bad=bad, offset=None if twin.vol is None else twin.vol["offset"],
                                  tracker=st))
            rec.append(r)
        out[name] = dict(rec=rec, calls=calls)
        ar.close()
    return out


def test_every_call_equals_the_restated_rule_over_the_stages(runs):
    calls = runs["blocks"]["calls"]
    for c in calls:
        assert c["bad"] == [], (c["frame"], c["bad"])
    none = [c for c in calls if c["offset"] is None]
    some = [c for c in calls if c["offset"] is not None]
    assert none and all(c["got"]["info"]["status"] == 5 for c in none) and len(some) > 60
    assert all(c["got"]["info"]["status"] == 0 and c["got"]["info"]["epoch"] == 1 for c in some)
    # (one frame's weights need not reach min_weight: the first calls may find a volume without a surface)
    first = next(c["got"] for c in some if c["got"]["info"]["present"] > 0)
    assert first["info"]["blocks"] == first["info"]["present"] and set(first["state"].tolist()) == {1}
    # unaligned lattices occurred, and blocks changed, came and went
    assert any(any(v % B for v in c["offset"]) for c in some)
    states = np.concatenate([c["got"]["state"] for c in some if not c["all"]])
    print("reports by state", np.bincount(states, minlength=5).tolist(), "calls", len(some))
    assert (states == 2).sum() > 0 and (states == 1).sum() > 0 and (states >= 3).sum() > 0 and not (states == 0).any()
    # a call on a volume that has not changed reports nothing; with ALL it reports every present block, unchanged
    quiet = [c for c in some[1:] if not c["updated"]]
    assert len(quiet) > 40
    for c in quiet:
        g = c["got"]
        if c["all"]:
            assert g["info"]["blocks"] == g["info"]["present"] and not g["state"].any(), c["frame"]
        else:
            assert g["info"]["blocks"] == 0 and len(g["vertices"]) == 0, c["frame"]


def test_the_all_answer_welded_by_cell_is_the_whole_mesh(runs):
    rec, calls = runs["blocks"]["rec"], runs["blocks"]["calls"]
    done = [c for c in calls if c["all"] and c["updated"] and c["got"]["info"]["present"] > 8]
    assert done
    c = done[-1]
    q, w, mv, mn, mt = rec[c["frame"]][5][:5]
    got = c["got"]
    whole = Mc.extract(q, w, got["geometry"]["origin"], got["geometry"]["voxel"], MW, BIG, BIG)
    assert np.array_equal(whole["vertices"].view(np.uint32), mv.view(np.uint32)) and np.array_equal(whole["triangles"], mt)   # mesh() itself
    cell_id = {tuple(x): n for n, x in enumerate(whole["cells"].tolist())}
    tri_at = {tuple(t): n for n, t in enumerate(mt.tolist())}
    seen = []
    for key, (v0, nv, t0, nt) in zip(got["keys"], got["ranges"]):
        blk = Bc.block_mesh(q, w, got["geometry"]["origin"], got["geometry"]["voxel"], c["offset"], MW, B, key)   # (for the cells)
        assert blk["nv"] == nv and 2 * blk["nq"] == nt
        ids = np.array([cell_id[tuple(x)] for x in blk["cells"].tolist()], np.int64)
        assert got["vertices"][v0:v0 + nv].tobytes() == mv[ids].tobytes() and got["normals"][v0:v0 + nv].tobytes() == mn[ids].tobytes()
        at = [tri_at[tuple(t)] for t in ids[got["triangles"][t0:t0 + nt]].tolist()]
        assert at == sorted(at)
        seen += at
    assert sorted(seen) == list(range(len(mt)))   # every triangle of mesh(), once


def test_asking_on_every_frame_changes_nothing_else(runs):
    a, b = runs["blocks"]["rec"], runs["never"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in b] and 4 in [r[0] for r in b]
    updates = 0
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
        for x, y in zip(ra[3] + ra[4], rb[3] + rb[4]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        assert (ra[5] is None) == (rb[5] is None), k
        if ra[5] is not None:
            updates += 1
            for x, y in zip(ra[5], rb[5]):   # the volume, mesh() and meshDepth()
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert updates >= 10


def _box_in_cube(key, lattice, block=B):
    l0 = block * np.asarray(key) - np.asarray(lattice) - 1
    return bool(np.all(l0 >= 0) and np.all(l0 + block + 1 < RES))


def test_move_caps_reset_and_colours(ctx, frames):  # noqa: F811
    """one session with a follow block of 8 (every lattice a multiple of the block edge: every block whole) and mesh colour"""
    from alvaar_amd.system import AlvaAR, AlvaError
    plain = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        plain.meshBlocks(colors=True)
    for bad in (dict(block=4), dict(block=12), dict(min_weight=0), dict(max_blocks=0), dict(max_vertices=0)):
        with pytest.raises(AlvaError, match="bad argument"):
            plain.meshBlocks(**bad)
    assert plain.meshBlocks()["info"]["status"] == 5
    plain.close()
    ar = _session("color", mesh_follow=8, mesh_color=True)
    twin = _Twin(ctx, ar)
    fd = Ms._Feeder(ar, frames)
    got, bad = twin.call(colors=True)
    assert bad == [] and got["info"]["status"] == 5
    # a few coloured updates, each followed by a call with colours
    # (one frame's weights need not reach min_weight: updates until the volume has a surface in more than 8 blocks, and then some)
    n_updates, present, reported = 0, 0, 0
    while present <= 8 or n_updates < 4:
        assert fd.t < 60
        fd.feed(0 if fd.t == 0 else None)
        info = ar.meshUpdate(debug=True, **KW)
        if info["status"] != 0:
            continue
        n_updates += 1
        twin.volume(info, ar.meshFollowStats()["offset"])
        got, bad = twin.call(colors=True, all_=n_updates % 3 == 0)
        assert bad == [] and got["info"]["status"] == 0 and all(v % 8 == 0 for v in twin.vol["offset"]), (n_updates, bad)
        present, reported = got["info"]["present"], reported + got["info"]["blocks"]
        again, bad = twin.call(colors=True)
        assert bad == [] and again["info"]["blocks"] == 0
    assert reported >= present
    # over each cap, then with room: the answer a single call gives (the restated list is untouched by the refused calls, as the session's)
    info = None
    while info is None or info["status"] != 0:
        fd.feed()
        info = ar.meshUpdate(debug=True, **KW)
    twin.volume(info, ar.meshFollowStats()["offset"])
    probe = copy.deepcopy(twin.L)
    digest, counts, _ = ctx.mesh_block_digest(twin.vol["dq"], twin.vol["dw"], twin.vol["offset"], MW, B)
    single = probe.call(twin.gen, MW, B, True, 4096, BIG, BIG, RES, twin.vol["offset"], digest, counts)
    n_rep, nv, nt = single[0][1:4]
    assert n_rep > 8 and nv > 0 and nt > 0
    for caps in (dict(max_blocks=n_rep - 1), dict(max_vertices=nv - 1), dict(max_triangles=nt - 1)):
        got, bad = twin.call(all_=True, colors=True, **caps)
        assert bad == [] and got["info"]["status"] == 3 and (got["info"]["blocks"], got["info"]["vertices"], got["info"]["triangles"]) == (n_rep, nv, nt)
    got, bad = twin.call(all_=True, colors=True, max_blocks=n_rep, max_vertices=nv, max_triangles=nt)
    assert bad == [] and got["info"]["status"] == 0 and got["info"]["blocks"] == n_rep
    assert [got["keys"].tolist(), got["state"].tolist(), got["ranges"].tolist()] == [[list(r[0]) for r in single[1]], [r[1] for r in single[1]],
                                                                                   [list(r[2:6]) for r in single[1]]]
    # a move by one block along x: state 4 for exactly the keys that left, nothing whose box lies in both cubes
    before = dict(twin.L.table)
    old = twin.vol
    centre = old["origin"] + old["voxel"] * RES / 2
    r = ar.meshMove(centre + np.array([8.5, 0.0, 0.0]) * old["voxel"], block=8)
    assert r["shifted"] == 1 and r["shift"].tolist() == [8, 0, 0]
    q2, w2, _, _ = Sc.shift(old["q"], old["w"], None, (8, 0, 0))
    new_offset = tuple(int(a + b) for a, b in zip(old["offset"], (8, 0, 0)))
    assert ar.meshFollowStats()["offset"].tolist() == list(new_offset)
    twin.vol = dict(q=q2, w=w2, dq=_dev(q2), dw=_dev(w2), origin=r["origin"].copy(), voxel=old["voxel"], offset=new_offset)
    got, bad = twin.call()
    assert bad == [] and got["info"]["status"] == 0 and got["info"]["epoch"] == 1
    bmin = Bc.grid(RES, new_offset, B)[0]
    left = sorted((k for k in before if k[0] < bmin[0]), key=lambda k: k[::-1])
    assert left and [tuple(k) for k, s in zip(got["keys"].tolist(), got["state"]) if s == 4] == left
    for k, s in zip(got["keys"].tolist(), got["state"]):
        assert s == 4 or not (_box_in_cube(k, old["offset"]) and _box_in_cube(k, new_offset)), (k, s)
    kept = [k for k in before if _box_in_cube(k, old["offset"]) and _box_in_cube(k, new_offset)]
    assert kept and not set(kept) & {tuple(k) for k in got["keys"].tolist()}
    # another min_weight and another block edge start over; so does resetMeshBlocks
    for kw in (dict(min_weight=MW + 1), dict(block=16)):
        epoch = twin.L.epoch
        got, bad = twin.call(**kw)
        assert bad == [] and got["info"]["epoch"] == epoch + 1 and got["info"]["blocks"] == got["info"]["present"] > 0 and set(got["state"].tolist()) == {1}
    ar.resetMeshBlocks()
    twin.L.reset()
    got, bad = twin.call(block=16)
    assert bad == [] and got["info"]["epoch"] == epoch + 2 and set(got["state"].tolist()) == {1}
    # resetMesh: no volume, then a new one -- the epoch moves
    ar.resetMesh()
    twin.vol = None
    got, bad = twin.call()
    assert bad == [] and got["info"]["status"] == 5
    info, _ = fd.until_integrated(None, limit=20, rel_extent=EXTENT)
    assert info["placed"] == 1
    info2 = None
    while info2 is None or info2["status"] != 0:
        fd.feed()
        info2 = ar.meshUpdate(debug=True, **KW)
    assert info2["placed"] == 0
    twin.gen += 1   # (the placement above)
    twin.volume(info2, ar.meshFollowStats()["offset"])
    got, bad = twin.call(block=16)
    assert bad == [] and got["info"]["epoch"] == epoch + 3 and got["info"]["blocks"] == got["info"]["present"] and set(got["state"].tolist()) <= {1}
    ar.close()
