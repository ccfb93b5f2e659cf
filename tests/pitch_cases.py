"""TEST INFRASTRUCTURE: row pitches and sub-views for the image entry points -- the layouts, the helper that embeds an image in a larger
poisoned block, and the table of which entry point is run on which layouts and shapes.  Plain numpy; tests/test_pitch_cases.py checks the
table on the CPU, tests/test_gpu_pitch.py runs it on the GPU.

A layout places a w x h image inside a 1-D uint8 block filled with a poison value: rows `pitch` bytes apart, the first pixel `off` bytes
into the block.  The image is never the tail of its block: at least one whole row of poison and TAIL bytes follow its last row and at
least one whole row precedes it, so a kernel that reads a row at the wrong pitch, or runs past a row's end, reads poison inside the
allocation (and the comparison with the oracle fails) instead of leaving it.

Contract classes (include/alvaar_hip.h): the legal step is what a pitch and a start address must be a multiple of.
  rgba    4 bytes per pixel, pitch % 16 == 0, start 16-byte aligned (rows are read with 16-byte loads)
  gray4   1 byte per pixel, pitch % 4 == 0, start 4-byte aligned (rows are read / written with dwords)
  byte    1 byte per pixel, pitch >= width and nothing else"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

POISONS = (171, 84)     # every GPU case runs with both: a pixel can equal one poison value, not both
TAIL = 256              # bytes behind the row of poison that follows the view
CONTRACTS = {"rgba": (4, 16), "gray4": (1, 4), "byte": (1, 1)}   # bytes per pixel, legal step

ALIGNED_LAYOUTS = ("packed", "pad_min", "pad_odd64", "offset")
BYTE_LAYOUTS = ("byte_offset_1", "byte_offset_2", "byte_offset_3")   # only where the contract has no alignment rule
LAYOUTS = ALIGNED_LAYOUTS + BYTE_LAYOUTS
OFFSET_STEPS, OFFSET_ROWS = 3, 3   # `offset`: the view starts this many legal steps into its row and this many rows down

Geometry = namedtuple("Geometry", "pitch off nbytes row_bytes x0 rows_before")


def geometry(w, h, contract, layout):
    """where a w x h image of the contract class lies in its block under the layout"""
    px, step = CONTRACTS[contract]
    rb = w * px
    if layout == "packed":                       # the control: rows touch, yet the block still has poison in front and behind
        pitch, x0, rows = rb, 0, 1
    elif layout == "pad_min":                    # the smallest legal padding
        pitch, x0, rows = rb + step, 0, 1
    elif layout == "pad_odd64":                  # rows start at changing offsets within a 64-byte line
        pitch, x0, rows = (rb + 63) // 64 * 64 + step, 0, 1
    elif layout == "offset":                     # a region of interest inside a larger frame, pad_min behind it
        x0, rows = OFFSET_STEPS * step, OFFSET_ROWS
        pitch = x0 + rb + step
    elif layout in BYTE_LAYOUTS:                 # odd pitches w + 1 and w + 3, the start 1, 2 or 3 bytes into its row
        if contract != "byte":
            raise ValueError("%s is for byte-contract images only" % layout)
        x0, rows = BYTE_LAYOUTS.index(layout) + 1, 1
        pitch = w + (1 if x0 == 1 else 3)
    else:
        raise ValueError(layout)
    off = rows * pitch + x0
    return Geometry(pitch, off, (rows + h + 1) * pitch + x0 + TAIL, rb, x0, rows)


def view_of(block, shape, geom):
    """the image's (writable) view inside a block laid out by `geom`; shape (h, w) or (h, w, 4)"""
    h = shape[0]
    strides = (geom.pitch, 1) if len(shape) == 2 else (geom.pitch, 4, 1)
    assert block.dtype == np.uint8 and block.ndim == 1 and len(block) == geom.nbytes
    assert geom.off + (h - 1) * geom.pitch + geom.row_bytes <= len(block)
    return np.lib.stride_tricks.as_strided(block[geom.off:], shape=tuple(shape), strides=strides)


def inside_mask(shape, geom):
    """bool [nbytes]: True at the block's bytes that belong to the image"""
    m = np.zeros(geom.nbytes, bool)
    for r in range(shape[0]):
        m[geom.off + r * geom.pitch:geom.off + r * geom.pitch + geom.row_bytes] = True
    return m


def default_contract(img):
    return "rgba" if img.ndim == 3 else "gray4"


def embed(img, layout, poison, contract=None):
    """(block, view, off): a new uint8 block filled with `poison`, the view of a copy of `img` ((h, w) gray or (h, w, 4) RGBA) inside
    it, and the view's byte offset.  contract: "rgba" for RGBA; "gray4" (the default) or "byte" for gray."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 4))
    contract = contract or default_contract(img)
    assert (contract == "rgba") == (img.ndim == 3)
    geom = geometry(img.shape[1], img.shape[0], contract, layout)
    block = np.full(geom.nbytes, poison, np.uint8)
    view = view_of(block, img.shape, geom)
    view[...] = img
    return block, view, geom.off


def legal(contract, w, pitch, off):
    """the documented rule of the contract class for a row pitch and a start offset (from an allocation aligned to 256 bytes or more)"""
    px, step = CONTRACTS[contract]
    return pitch >= w * px and pitch % step == 0 and off % step == 0


# the output of a call gets another layout than its input: the two pitches must not be mixed up
OUT_LAYOUT = {"packed": "offset", "pad_min": "pad_odd64", "pad_odd64": "packed", "offset": "pad_min",
              "byte_offset_1": "byte_offset_3", "byte_offset_2": "byte_offset_1", "byte_offset_3": "byte_offset_2"}

# ---- the table ------------------------------------------------------------------------------------------------------------------------
Entry = namedtuple("Entry", "contract layouts out_contract")
_RGBA_IN = Entry("rgba", ALIGNED_LAYOUTS, None)
_BYTE_IN = Entry("byte", LAYOUTS, None)        # read by bytes (or by unaligned dwords inside the row): no alignment rule
ENTRY_POINTS = {
    "alva_rgba2gray": Entry("rgba", ALIGNED_LAYOUTS, "gray4"),
    "alva_pyramid_build_from_gray": Entry("gray4", ALIGNED_LAYOUTS, None),
    "alva_pyramid_build_from_rgba": Entry("rgba", ALIGNED_LAYOUTS, "gray4"),
    "alva_pyramid_build_from_rgba_batch": Entry("rgba", ALIGNED_LAYOUTS, "gray4"),
    "alva_detect_grid": _BYTE_IN,
    "alva_detect_grid_enqueue": _BYTE_IN,
    "alva_fast": _BYTE_IN,
    "alva_orb_detect_and_compute": _BYTE_IN,
    "alva_orb_detect_and_compute_batch": _BYTE_IN,
    "alva_orb_blur": Entry("byte", LAYOUTS, "byte"),
    "alva_frontend_track": _RGBA_IN,
    "alva_frontend_track_ahead": _RGBA_IN,
    "alva_track_batch_step": _RGBA_IN,
    "alva_track_batch_step_detect": _RGBA_IN,
}

# alva_rgba2gray: a workgroup is 256 pixels x 4 rows, a thread four pixels -- one thread, just under / exactly / just over one
# workgroup's width; one row, one workgroup's rows, one row more
RGBA2GRAY_SHAPES = tuple((w, h) for w in (4, 252, 256, 260) for h in (1, 4, 5))

# the pyramid builders: (w, h, win, max_level) -> the levels built.
#   68 x 33, 100 x 76 at the tracker's window: the one-launch route's 64 x 16 level-0 tile is cut on both edges, deep tiles 16 / 12 / 4
#   36 x 28 at win 3: four levels, the stop rule cuts;  64 x 48 at win 15: one level
#   200 x 152 at win 3: SIX levels (200, 100, 50, 25, 13, 7 wide; the next would be 4 x 3 and 3 <= win), the per-level chain;
#   196 x 196 at win 3: the smallest size with seven levels (196, 98, 49, 25, 13, 7, 4), the same chain one launch longer
PYRAMID_CASES = {(68, 33, 9, 3): 2, (100, 76, 9, 3): 4, (36, 28, 3, 7): 4, (200, 152, 3, 7): 6, (196, 196, 3, 7): 7, (64, 48, 15, 0): 1}
PYRAMID_BATCH_CASE = (68, 33, 9, 3)
PYRAMID_BATCHES = (2, 9)            # 9 cameras: the camera -> XCD order of the batched launches (8 and more)
PYRAMID_SMALLEST = (12, 10, 9, 0)   # the smallest level 0 alva_pyramid_create accepts at the tracker's window (width % 4 == 0)
PYRAMID_REFUSED = ((8, 8, 9), (12, 8, 9), (8, 12, 9), (12, 9, 9))   # level 0 not larger than the window in a dimension

# rows of detect_cases.py, one per class it distinguishes, each at that class's smallest image: a small cell on the texture with tracked
# points and the default ROI | the low-entropy image, whole-image ROI (k_subpix's border path), cell % 4 == 1 | four waves per cell |
# w = cell * nw + 1 | exact ties | repair chains under tracked points | lambda_min 0 everywhere | an unaligned ROI | a capacity below
# the count | occupancy on the cell edges | three calls that carry the threshold
DETECT_ROWS = ("tex_c4", "low_c5", "low_c17", "low_c7_plus1", "periodic_c6", "chain_occ_c5", "constant_c8_q0", "roi_unaligned_c7",
               "cap_nprim_c8", "occ_edges_c7", "seq_up_c8")

# rows of orb_cases.py, one per group (bound_over is the call the host refuses: it never reaches a kernel): one level (k_copy_level0) |
# more than 4096 candidates | two levels at scale 2.0 and eight at 1.2 (pyr_column_body) | the launch bound | the 4096-survivor split |
# the smooth image | zero level budgets | more rows than the LDS row table
ORB_ROWS = ("tie_small-50", "tie_big-2100", "tie_levels-2.0x2", "tie_levels-1.2x8", "bound_at", "split_4096-sort_cap+1", "edge_small-n1",
            "zero_budgets-3", "tall")
ORB_BATCH_GEOMETRY = (300, 1.2, 8)          # nfeatures, scale, nlevels of the batch's cameras (tie_levels-1.2x8's)
ORB_BATCH_SPECS = ("TILED", "BYTES", "SMOOTH")   # orb_cases' 320 x 240 images, cycled over the cameras
ORB_BATCHES = (2, 9)
FAST_ROWS = ("tall_fast_image:0", "tall_fast_image:1", "SMOOTH")    # two and one chunk boundaries of the row scan; the smooth image
BLUR_ROWS = ("tall_fast_image:1", "SMOOTH", "TILED")                # 64 wide: exactly one tile; 320 x 240

DRIVER_SIZE = (320, 240, 3)   # width, height, frames of the Frontend / TrackBatch runs
