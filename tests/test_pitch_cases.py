"""CPU: the table of tests/pitch_cases.py is what tests/test_gpu_pitch.py takes it for -- every view holds its image at the stride,
start and poison margins its layout states, every (entry point, layout) pair is legal under the entry point's documented rule, every
entry point has the four aligned layouts, the pyramid sizes have the level counts the table states, and the reused detector and ORB
rows exist."""
import numpy as np
import pytest

import pitch_cases as P
from oracles import pyr_dims


def _image(w, h, contract, seed=1):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 4) if contract == "rgba" else (h, w)).astype(np.uint8)


SHAPES = ((4, 1), (260, 5), (68, 33), (98, 74), (61, 17))


@pytest.mark.parametrize("contract", list(P.CONTRACTS))
@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_views_hold_their_image_inside_poison(contract, layout):
    if layout in P.BYTE_LAYOUTS and contract != "byte":
        with pytest.raises(ValueError):
            P.geometry(8, 8, contract, layout)
        return
    px, step = P.CONTRACTS[contract]
    for w, h in SHAPES:
        if contract != "byte" and w % 4:
            continue
        for poison in P.POISONS:
            img = _image(w, h, contract)
            block, view, off = P.embed(img, layout, poison, contract)
            g = P.geometry(w, h, contract, layout)
            assert np.array_equal(view, img) and view.shape == img.shape and off == g.off
            assert view.strides[0] == g.pitch and view.strides[1:] == ((4, 1) if contract == "rgba" else (1,))
            assert view.ctypes.data - block.ctypes.data == off
            assert P.legal(contract, w, g.pitch, off), (w, h, g)
            # the margins: a whole row in front, a whole row and TAIL bytes behind, all poison; nothing but the image is not poison
            first, last = off, off + (h - 1) * g.pitch + g.row_bytes
            assert first >= g.pitch and len(block) - last >= g.pitch + P.TAIL
            inside = P.inside_mask(img.shape, g)
            assert inside.sum() == img.size and (block[~inside] == poison).all()
            assert np.array_equal(block[inside].reshape(img.shape), img)
            # what the layout's name says
            if layout == "packed":
                assert g.pitch == g.row_bytes
            elif layout == "pad_min":
                assert g.pitch == g.row_bytes + step
            elif layout == "pad_odd64":
                assert (g.pitch - step) % 64 == 0 and 0 <= g.pitch - step - g.row_bytes < 64
                assert len({(off + r * g.pitch) % 64 for r in range(4)}) == min(4, 64 // np.gcd(step, 64))   # rows start at changing offsets in a line
            elif layout == "offset":
                assert g.x0 == P.OFFSET_STEPS * step and g.rows_before == 3 and g.pitch == g.x0 + g.row_bytes + step
            else:
                assert g.x0 == int(layout[-1]) and g.pitch in (w + 1, w + 3) and (w % 2 or g.pitch % 2 == 1)
            # writing through the view changes the block, and only inside
            view[...] = 255 - img
            assert (block[~inside] == poison).all()


def test_every_pair_is_legal_and_every_entry_point_has_the_aligned_layouts():
    names = ("alva_rgba2gray", "alva_pyramid_build_from_gray", "alva_pyramid_build_from_rgba", "alva_pyramid_build_from_rgba_batch",
             "alva_detect_grid", "alva_detect_grid_enqueue", "alva_fast", "alva_orb_detect_and_compute", "alva_orb_detect_and_compute_batch",
             "alva_orb_blur", "alva_frontend_track", "alva_frontend_track_ahead", "alva_track_batch_step", "alva_track_batch_step_detect")
    assert tuple(P.ENTRY_POINTS) == names
    for name, e in P.ENTRY_POINTS.items():
        assert set(P.ALIGNED_LAYOUTS) <= set(e.layouts), name
        assert e.contract == "byte" or not set(e.layouts) & set(P.BYTE_LAYOUTS), name   # a misaligned start only where no rule forbids it
        for layout in e.layouts:
            for w, h in ((4, 1), (68, 33), (320, 240)):
                g = P.geometry(w, h, e.contract, layout)
                assert P.legal(e.contract, w, g.pitch, g.off), (name, layout, w)
                if e.out_contract:
                    o = P.geometry(w, h, e.out_contract, P.OUT_LAYOUT[layout])
                    assert P.legal(e.out_contract, w, o.pitch, o.off) and P.OUT_LAYOUT[layout] != layout, (name, layout)
    # the outputs see every layout too
    assert set(P.OUT_LAYOUT.values()) == set(P.LAYOUTS)


def test_the_header_states_the_rules_the_table_uses():
    """include/alvaar_hip.h is the contract: the RGBA and "% 4" rules, and the list of entry points without an alignment rule"""
    from pathlib import Path
    text = " ".join((Path(__file__).resolve().parent.parent / "include" / "alvaar_hip.h").read_text().split())
    for phrase in ("pitch >= 4 * width, pitch % 16 == 0, the pointer 16-byte aligned", "pitch >= width, pitch % 4 == 0, the pointer 4-byte aligned",
                   "pitch >= width and nothing else", "width > win && height > win"):
        assert phrase in text, phrase
    free = text[text.index("pitch >= width and nothing else"):text.index("An image may be a view into a larger buffer")]
    for name, e in P.ENTRY_POINTS.items():
        if e.contract == "byte":
            assert name.replace("_batch", "").replace("_enqueue", "") in free, name


def test_pyramid_sizes_have_the_stated_levels():
    for (w, h, win, depth), levels in P.PYRAMID_CASES.items():
        assert len(pyr_dims(w, h, win, depth)) == levels, (w, h, win, depth)
        assert w % 4 == 0 and w > win and h > win
    assert P.PYRAMID_BATCH_CASE in P.PYRAMID_CASES
    # which route a device frame takes (alva_pyramid_build_from_rgba): one launch for 2 .. 4 levels, level 0 + the per-level chain else
    assert sorted(P.PYRAMID_CASES.values()) == [1, 2, 4, 4, 6, 7]
    w, h, win, depth = P.PYRAMID_SMALLEST
    assert w % 4 == 0 and w > win and h == win + 1 and len(pyr_dims(w, h, win, depth)) == 1
    for w, h, win in P.PYRAMID_REFUSED:
        assert w % 4 == 0 and (w <= win or h <= win)
    # 68 x 33 and 100 x 76 cut the 64 x 16 level-0 tile on both edges
    for w, h in ((68, 33), (100, 76)):
        assert w % 64 and h % 16
    for w, h in P.RGBA2GRAY_SHAPES:
        assert w % 4 == 0
    assert {w for w, _ in P.RGBA2GRAY_SHAPES} == {4, 252, 256, 260} and {h for _, h in P.RGBA2GRAY_SHAPES} == {1, 4, 5}


def test_reused_rows_exist():
    import detect_cases as D
    import orb_cases as oc
    assert set(P.DETECT_ROWS) <= set(D.CASE_NAMES) and len(set(P.DETECT_ROWS)) == len(P.DETECT_ROWS)
    assert set(P.ORB_ROWS) <= set(oc.CASE_IDS) and "bound_over" not in P.ORB_ROWS
    assert {oc.case(i).group for i in P.ORB_ROWS} == {c.group for c in oc.cases()} - {"bound_over"}
    for row in P.FAST_ROWS + P.BLUR_ROWS + P.ORB_BATCH_SPECS:
        name, _, arg = row.partition(":")
        assert hasattr(oc, name), row
        if arg:
            assert oc.tall_fast_image(int(arg)).ndim == 2
    nf, scale, nlevels = P.ORB_BATCH_GEOMETRY
    c = oc.case("tie_levels-1.2x8")
    assert (c.nf, c.scale, c.nlevels) == (nf, scale, nlevels) and c.spec == oc.TILED
    assert {oc.image(getattr(oc, s)).shape for s in P.ORB_BATCH_SPECS} == {(240, 320)}
    # the detector rows cover a tracked-points case, a whole-image ROI, a capacity and a sequence
    assert D.case("cap_nprim_c8").cap is not None and D.case("seq_up_c8").calls == 3 and D.case("tex_c4").occupied is not None
    h, w = D.case("low_c5").gray.shape
    assert D.case("low_c5").roi == (0, 0, w, h)
    assert P.DRIVER_SIZE == (320, 240, 3)
