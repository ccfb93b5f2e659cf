"""The volume raycast stages (alva_mesh_raycast, alva_mesh_raycast_pixels) on the GPU against their numpy restatement
tests/raycast_cases.py: t, the points and the normals (as uint32), the codes, the poses (as uint32), pose_ok and the info are EQUAL, bit
for bit, for every case of the table, and equal again on a second run.  Both sides do the same IEEE operations in the same order and
everything after the sample's fractions is an integer, so there is no tolerance.  The three ways to ask for the same rays -- the grid,
the list of the grid's pixels, the world rays the restatement derives from them -- give the same bits too."""
from __future__ import annotations

import numpy as np
import pytest

import raycast_cases as Rc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in Rc.cases()}
FLOATS, BYTES = ("t", "point", "normal", "pose"), ("code", "pose_ok")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _volume(c):
    return _dev(c["q"]), _dev(c["w"]), c["origin3"], c["voxel"], c["min_weight"]


def _gpu(ctx, c, uv="own"):
    if c["kind"] == "world":
        return ctx.mesh_raycast(*_volume(c), _dev(c["rays6"]), c["t_near"], c["t_far"])
    uv = c["uv"] if isinstance(uv, str) else uv
    return ctx.mesh_raycast_pixels(*_volume(c), c["T_wc12"], c["calib8"], c["width"], c["height"], c["step"], None if uv is None else _dev(uv),
                                   c["t_near"], c["t_far"])


def _differing(got, want):
    """the names of the outputs of `got` that differ from `want`'s"""
    bad = []
    for k in FLOATS:
        if k in got and not (got[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32))):
            bad.append(k)
    for k in BYTES:
        if k in got and not (got[k].dtype == np.uint8 and np.array_equal(got[k], want[k])):
            bad.append(k)
    if not np.array_equal(got["info"], want["info"]):
        bad.append("info")
    return bad


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement_bit_for_bit(ctx, name):
    c = CASES[name]
    want = Rc.expected()[name]
    got = _gpu(ctx, c)
    print("gpu info", got["info"].tolist(), "restatement", want["info"].tolist())
    assert ("pose" in got) == (c["kind"] == "pixels")
    assert _differing(got, want) == []
    assert _differing(_gpu(ctx, c), got) == []


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "pixels" and c["uv"] is None])
def test_grid_list_and_world_rays_give_the_same_bits(ctx, name):
    c = CASES[name]
    want = Rc.expected()[name]
    grid = _gpu(ctx, c)
    lst = _gpu(ctx, c, uv=Rc.grid_pixels(c["width"], c["height"], c["step"]))
    assert _differing(lst, grid) == []
    world = ctx.mesh_raycast(*_volume(c), _dev(want["rays6"]), c["t_near"], c["t_far"])
    assert _differing(world, grid) == []


def test_without_poses_and_rejected_arguments(ctx):
    from alvaar_amd import AlvaError
    c = CASES["grid_10x7"]
    q, w, o, vx, mw = _volume(c)
    bare = ctx.mesh_raycast_pixels(q, w, o, vx, mw, c["T_wc12"], c["calib8"], c["width"], c["height"], c["step"], pose=False)
    assert "pose" not in bare and _differing(bare, Rc.expected()["grid_10x7"]) == []
    rays = _dev(CASES["wall_named_rays"]["rays6"])
    bad_T = c["T_wc12"].copy()
    bad_T[3] = np.nan
    for call in (lambda: ctx.mesh_raycast(q, w, o, vx, 0, rays), lambda: ctx.mesh_raycast(q, w, o, vx, 256, rays),
                 lambda: ctx.mesh_raycast(q, w, o, -1.0, mw, rays), lambda: ctx.mesh_raycast(q, w, o, vx, mw, rays, 2.0, 1.0),
                 lambda: ctx.mesh_raycast(q, w, o, vx, mw, rays, float("-inf"), 1.0), lambda: ctx.mesh_raycast(q, w, o, vx, mw, rays, 0.0, float("nan")),
                 lambda: ctx.mesh_raycast(q, w, o, vx, mw, rays[:0]), lambda: ctx.mesh_raycast(q[:3, :3, :3].contiguous(), w[:3, :3, :3].contiguous(), o, vx, mw, rays),
                 lambda: ctx.mesh_raycast_pixels(q, w, o, vx, mw, bad_T, c["calib8"], c["width"], c["height"], c["step"]),
                 lambda: ctx.mesh_raycast_pixels(q, w, o, vx, mw, c["T_wc12"], c["calib8"], c["width"], c["height"], 17)):
        with pytest.raises(AlvaError):
            call()
    # the context is usable after a rejected argument
    assert _differing(_gpu(ctx, c), Rc.expected()["grid_10x7"]) == []
