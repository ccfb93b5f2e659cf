"""GPU parity: the grid detector (csrc/detect_grid.hip) on the cases of tests/detect_cases.py -- every cell class, image family, ROI,
capacity, occupancy set and threshold sequence -- bitwise against the compiled reference where it is built, else against the plain-C
oracle (tests/test_detect_cases.py pins that to the reference on the same cases): the point list as uint32 with its order, the count,
the new threshold with ==.  Then the one-workgroup finisher on the variants it has (no tracked points, mask in LDS, mask in global
memory, the exact arg-max), the split enqueue / collect API, the argument limits, and the re-use of the context's scratch."""
import functools

import numpy as np
import pytest

import detect_cases as D

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
LDS_LIMIT = 160 * 1024 - 1024


def _upload(c):
    import torch
    g = torch.from_numpy(np.array(c.gray)).cuda()
    occ = None if c.occupied is None or len(c.occupied) == 0 else torch.from_numpy(np.array(c.occupied)).cuda()
    return g, occ


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _run_and_compare(ctx, name):
    """every call of the case against the shared reference; returns the device results of the calls"""
    import torch
    c, ref = D.case(name), D.reference_of(name)
    g, occ = _upload(c)
    mq = c.max_quality
    got = []
    for pts_ref, mq_ref in ref:
        n = len(pts_ref)
        if c.cap is None:
            pts, nmq = ctx.detect_grid(g, c.cell, occ, roi=c.roi, max_quality=mq)
            assert pts.shape[0] == n, (name, pts.shape[0], n)
        else:
            # a capacity below the count: the count and the threshold are those of the whole list, the first `cap` points are written,
            # the rows behind them are not touched
            out = torch.full((c.cap + 4, 2), SENTINEL, dtype=torch.float32, device="cuda")
            pts, nmq, count = ctx.detect_grid_collect(ctx.detect_grid_enqueue(g, c.cell, occ, roi=c.roi, max_quality=mq, cap=c.cap, out=out))
            assert count == n and n > c.cap
            assert pts.shape[0] == c.cap
            assert bool((out[c.cap:] == SENTINEL).all())
            one, nmq1 = ctx.detect_grid(g, c.cell, occ, roi=c.roi, max_quality=mq, cap=c.cap)   # the single call, its own buffer
            assert nmq1 == mq_ref and np.array_equal(_bits(one)[:c.cap], pts_ref[:c.cap].view(np.uint32))
            pts_ref = pts_ref[:c.cap]
        assert nmq == mq_ref, (name, nmq, mq_ref)
        assert np.array_equal(_bits(pts), pts_ref.view(np.uint32)), name
        got.append((pts.clone(), nmq))
        mq = mq_ref
    return got


@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_case_bit_exact(ctx, name):
    D.check_conditions(name)
    _run_and_compare(ctx, name)


# ---------------------------------------------------------------------------------------------------------------- lambda_min
@pytest.mark.parametrize("cell", D.CELLS)
def test_lambda_min_plane_bit_exact(ctx, cell):
    """k_cell_eig's lambda_min of every cell, bitwise, at every cell size, on the texture and on the low-entropy image.  The point list
    depends on a cell's largest values only; the plane shows the rest, e.g. the order of the three double additions of the 3x3 row sums
    (cv::boxFilter's RowSum adds (c[x-1] + c[x]) + c[x+1] for ksize 3; a running sum differs in the last bit at about one pixel in 10^4)"""
    import torch
    from oracles import Orc, Ref, ref_available
    O = Ref if ref_available() else Orc
    w, h = D.dims(cell)
    nw, nh = D.grid_of(cell)
    for g in (D.texture(w, h, 100 + cell), D.low_entropy(w, h, 200 + cell)):
        ctx.detect_grid(torch.from_numpy(g).cuda(), cell, None, roi=(0, 0, w, h), max_quality=1e-5)
        got = ctx.detect_grid_debug_eig(nw * nh, cell).cpu().numpy()
        want = np.stack([O.cell_mineig(g, c * cell, r * cell, cell)[1] for r in range(nh) for c in range(nw)])   # (w = cell * nw + 2: no cell is skipped)
        assert want.max() > 0
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------- finisher
def _lds_sizes(w, h, cell):
    """the dynamic LDS of k_select as alva_detect_grid_enqueue computes it: (per-cell arrays, static mask bit-plane) in bytes"""
    n_cells = (w // cell) * (h // cell)
    return n_cells * 16 + 5 * ((n_cells + 15) & ~15) + 64, ((w + 31) // 32) * h * 4


FINISHER_CASES = ("chain_c5", "chain_c16", "chain_c17", "chain_c40", "chain_occ_c5", "chain_occ_c16", "chain_occ_c17", "chain_occ_c40",
                  "periodic_c32", "periodic_c16", "periodic_c6", "chain_flat_c16_q0", "low_c8_q0", "low_c16", "tex_c17", "tex_c40")


@pytest.mark.parametrize("rounds", ["1", "2"])
@pytest.mark.parametrize("name", FINISHER_CASES)
def test_finisher_on_every_variant(ctx, monkeypatch, name, rounds):
    """with one or two multi-CU repair rounds instead of four, the one-workgroup finisher (k_select) has the rest of the fixed-point
    iteration to do; the result must not change.  Measured with a build whose k_select returns at once: periodic_c32 (both settings,
    and the default four rounds too), low_c16, tex_c17 and tex_c40 with one round then fail, so there the finisher does the repairs;
    on the other cases of the list the rounds that ran had already reached the fixed point, and the finisher only confirms it"""
    c = D.case(name)
    h, w = c.gray.shape
    arrays, mask = _lds_sizes(w, h, c.cell)
    assert arrays + mask <= LDS_LIMIT   # with tracked points, these keep the mask in LDS
    D.check_conditions(name)
    monkeypatch.setenv("ALVA_GRID_ROUNDS", rounds)
    _run_and_compare(ctx, name)


@functools.lru_cache(maxsize=None)
def _big_case():
    """864 x 600 at cell 10 with tracked points: 5160 cells.  The finisher's per-cell arrays fit in LDS, arrays + mask do not, so the
    static mask is read from global memory inside the evaluation"""
    from oracles import Orc, Ref, ref_available
    w, h, cell = 864, 600, 10
    g = D.periodic(w, h, 10, 77)   # chains of repairs across the grid, see detect_cases' chain_* cases
    occ = D.occ_uniform(w, h, 600, 78)
    O = Ref if ref_available() else Orc
    return dict(g=g, occ=occ, cell=cell, roi=(0, 0, w, h), ref=O.detect_grid(g, cell, occ, (0, 0, w, h), 1e-7))


@pytest.mark.parametrize("rounds", ["1", "2", None])
def test_finisher_with_the_mask_in_global_memory(ctx, monkeypatch, rounds):
    """the launch variant whose static mask stays in global memory.  Known limit: on this image the repair rounds reach the fixed point
    before the finisher, so a finisher that skipped its mask read would still pass; the variant's launch and set-up are what runs"""
    import torch
    b = _big_case()
    h, w = b["g"].shape
    arrays, mask = _lds_sizes(w, h, b["cell"])
    assert arrays <= LDS_LIMIT < arrays + mask, (arrays, mask)   # else this case no longer reaches the path
    assert len(b["occ"]) > 0 and len(b["ref"][0]) > 1000
    if rounds is not None:
        monkeypatch.setenv("ALVA_GRID_ROUNDS", rounds)
    pts, q = ctx.detect_grid(torch.from_numpy(b["g"]).cuda(), b["cell"], torch.from_numpy(b["occ"]).cuda(), roi=b["roi"], max_quality=1e-7)
    assert q == b["ref"][1] and pts.shape[0] == len(b["ref"][0])
    assert np.array_equal(_bits(pts), b["ref"][0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- split API
@pytest.mark.parametrize("name", ["tex_c14", "low_c23"])
def test_enqueue_then_collect_equals_the_single_call(ctx, name):
    c, ref = D.case(name), D.reference_of(name)
    D.check_conditions(name)
    g, occ = _upload(c)
    one, q1 = ctx.detect_grid(g, c.cell, occ, roi=c.roi, max_quality=c.max_quality)
    one = one.clone()
    handle = ctx.detect_grid_enqueue(g, c.cell, occ, roi=c.roi, max_quality=c.max_quality)
    assert handle["pending"].n_cells == D.oracle_of(name)[0]["n_cells"]
    two, q2, count = ctx.detect_grid_collect(handle)
    assert q1 == q2 == ref[0][1] and count == len(ref[0][0]) == one.shape[0]
    assert np.array_equal(_bits(one), _bits(two)) and np.array_equal(_bits(two), ref[0][0].view(np.uint32))


def test_image_narrower_than_the_cell(ctx):
    """no cell at all: count 0, the threshold as it was, nothing enqueued, no error -- through both entry points"""
    import torch
    g = torch.from_numpy(D.texture(20, 20, 1)).cuda()
    pts, q = ctx.detect_grid(g, 40, roi=(0, 0, 20, 20), max_quality=0.001, cap=8)
    assert pts.shape[0] == 0 and q == 0.001
    handle = ctx.detect_grid_enqueue(g, 40, roi=(0, 0, 20, 20), max_quality=0.001, cap=8)
    assert handle["pending"].n_cells == 0 and not handle["pending"].h_cnt
    pts, q, count = ctx.detect_grid_collect(handle)
    assert count == 0 and pts.shape[0] == 0 and q == 0.001
    from oracles import Orc
    rp, rq = Orc.detect_grid(D.texture(20, 20, 1), 40, roi=(0, 0, 20, 20), max_quality=0.001)
    assert len(rp) == 0 and rq == 0.001   # (0 < 0.33 * 0 is false: the reference leaves the threshold too)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_argument_limits_are_reported(ctx):
    """cell sizes outside 4 .. 40 and a cell count whose finisher arrays exceed the LDS limit are argument errors with a message, from
    both entry points, before anything is launched; the context works afterwards"""
    import torch
    import alvaar_amd
    g = torch.from_numpy(D.texture(640, 480, 3)).cuda()
    arrays, _ = _lds_sizes(640, 480, 4)
    assert arrays > LDS_LIMIT and (640 // 4) * (480 // 4) == 19200
    for cell, word in ((3, "cell_size"), (41, "cell_size"), (4, "lds_sel")):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.detect_grid(g, cell, max_quality=0.001, cap=16)
        msg = alvaar_amd.lib.alva_last_error().decode()
        assert "bad argument" in msg and word in msg, msg
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.detect_grid_enqueue(g, cell, max_quality=0.001, cap=16)
        assert word in alvaar_amd.lib.alva_last_error().decode()
    ctx.sync()
    _run_and_compare(ctx, "tex_c14")


# ---------------------------------------------------------------------------------------------------------------- scratch re-use
@pytest.mark.parametrize("name,between", [("tex_c14", "low_c40"), ("low_c33", "occ_many_c7"), ("low_c8_q0", "tex_c40")])
def test_same_result_after_a_call_of_another_size(ctx, name, between):
    """the detector's scratch slot is laid out anew by every call: a call of another size in between must leave nothing behind"""
    a = _run_and_compare(ctx, name)
    _run_and_compare(ctx, between)
    b = _run_and_compare(ctx, name)
    assert len(a) == len(b)
    for (pa, qa), (pb, qb) in zip(a, b):
        assert qa == qb and np.array_equal(_bits(pa), _bits(pb))
