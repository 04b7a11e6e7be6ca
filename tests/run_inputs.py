"""Painted image stacks for the run-length tests -- TEST INFRASTRUCTURE ONLY.

Bit patterns (L, H, W) for island_inputs.painted(), which turns one into an sdf_3d node whose table nodes are
the raster samples: the pattern is the exact image stack.  Each is built around one place where a run-length
walk can go wrong: the step from a row's last real pixel to the next row's first (the image rows are padded to
a multiple of 16 bytes, so with W = 17 the byte in front of a row's first is a padding zero, with W = 16 it is
the pixel itself), the seams of a walk of 64 lanes with four pixels each (63 | 64, 255 | 256), the first and
the last pixel of the stream, more rows in a chunk than one tile of the scan (4096), and rows of two full steps
and more with many starts in every step (dense, comb).  The preconditions are asserted without a GPU in
test_cpu_runs.py.
"""
import numpy as np

import island_inputs as ii
from implisolid_amd import scenes


def row_end(W):
    """five rows: rows 0 -> 1 and 3 -> 4 joined by a run across the row end (last pixel and next first pixel
    solid), row 1 -> 2 solid | empty and row 2 -> 3 empty | solid across it; layer 1 is the complement"""
    b = np.zeros((2, 5, W), bool)
    b[0, 0, W - 3:] = True
    b[0, 1, :2] = True
    b[0, 1, W - 1] = True
    b[0, 3, 0] = True
    b[0, 3, W - 1] = True
    b[0, 4, :] = True
    b[1] = ~b[0]
    return b


def boundaries():
    """300 pixels a row (two steps of 256, pitch 304).  Layer 0: row 0 solid over [64, 256): boundaries at
    63 | 64 and 255 | 256; row 1 solid over [0, 10): a boundary exactly at px = 0 behind an empty row end;
    row 2 solid over [290, 300) and row 3 over [0, 5): a run across the row end in the second step; row 4
    alternates from 250 to 262 across the step seam.  Layer 1: solid but for pixel 256 of every row"""
    b = np.zeros((2, 5, 300), bool)
    b[0, 0, 64:256] = True
    b[0, 1, 0:10] = True
    b[0, 2, 290:] = True
    b[0, 3, 0:5] = True
    b[0, 4, 250:262:2] = True
    b[1] = True
    b[1, :, 256] = False
    return b


def corners():
    """layer 0: a single solid pixel at p = 0 and another at p = W H - 1; layer 1: only the last; layer 2: only
    the first"""
    b = np.zeros((3, 9, 37), bool)
    b[0, 0, 0] = b[0, -1, -1] = True
    b[1, -1, -1] = True
    b[2, 0, 0] = True
    return b


def tall_thin():
    """17 x 129 pixels, 33 layers: 4257 rows in one chunk, more than one tile of the scan"""
    return np.random.default_rng(17).random((33, 129, 17)) < 0.5


def dense(W, ends=False):
    """two layers of three rows of W pixels (511, 512: the sdf_3d table's limit), filled at random by a half:
    about W / 4 runs of each class in every row, in every lane of both steps of the walk.  With `ends`, pixels 0,
    1 and 3 of every four of row 1 of layer 0 are solid, empty, empty and pixel 2 is random (about 3 W / 8 solid
    runs: more than 128 for W = 512), and then every row's last pixel is solid in layer 0 and empty in layer 1"""
    b = np.random.default_rng(7000 + W).random((2, 3, W)) < 0.5
    if ends:
        b[0, 1, 0::4] = True
        b[0, 1, 1::4] = False
        b[0, 1, 3::4] = False
        b[0, :, W - 1] = True
        b[1, :, W - 1] = False
    return b


# ---- the comb: a shape, rasterised at 1030 x 3 (five steps of the walk, the last of six pixels) --------------------
COMB_W, COMB_H = 1030, 3
COMB_PX = 2.0 ** -9                                   # the pixels are squares of 1 / 512: every sample is exact
COMB_RECT = [-1.0, -1.0 + COMB_W * COMB_PX, -1.5 * COMB_PX, 1.5 * COMB_PX]
COMB_Z = np.array([0.0, 0.5 * COMB_PX], np.float32)   # through the teeth's centres, and half a pixel above
COMB_SEAMS = [256, 512, 768, 1024]
# (x of the centre in pixels from the image's left edge, y of the centre in pixels from the middle row's samples,
# radius in pixels).  A pixel's sample is at its centre k + 0.5, a subsample of s = 2 at k + 0.25 and k + 0.75, the
# rows at y = -1, 0, 1 pixels.  The radii are an odd multiple of 1 / 8 or of 1 / 4 of a pixel and the centres
# multiples of 1 / 2, so no sample of any of these grids lies on a tooth's surface.  Seven teeth in each of the
# four full steps; the two widest hold three pixels of the middle row and lie half a pixel to one side, so that
# they leave the far row empty: the empty class stays in one piece.  One tooth of a radius of 3 / 4 on every seam
# (it holds the two pixels beside the seam in the middle row, and none of the rows above and below), and two of
# one pixel in the six pixels of the last step.
COMB_TEETH = [(256 * k + x, y, r) for k in range(4)
              for x, y, r in ((13.5, 0.0, 0.375), (40.0, 0.0, 0.75), (77.5, 0.5, 1.25), (121.0, 0.0, 0.75), (160.5, -0.5, 1.25),
                              (207.0, 0.0, 0.75), (236.5, 0.0, 0.375))]
COMB_TEETH += [(float(x), 0.0, 0.75) for x in COMB_SEAMS] + [(1026.5, 0.0, 0.375), (1028.5, 0.0, 0.375)]


def _union(children):
    return {"type": "Union", "matrix": list(scenes.EYE), "children": children}


# a Union takes at most 15 children (its chain of binary unions is as deep as the program's stacks allow), so the
# teeth stand in five flat Unions: one per full step, and the teeth on the seams with those of the last step
_TEETH = [{"type": "iellipsoid", "matrix": scenes.st(2 * r * COMB_PX, -1.0 + x * COMB_PX, y * COMB_PX, 0.0)} for x, y, r in COMB_TEETH]
COMB = _union([_union(_TEETH[7 * k:7 * k + 7]) for k in range(4)] + [_union(_TEETH[28:])])


def step_starts(on):
    """on bool (W,) -> the starts (on, the pixel before is not on or there is none) in each 256-pixel step"""
    on = np.asarray(on, bool)
    first = on.copy()
    first[1:] &= ~on[:-1]
    return [int(first[x0:x0 + 256].sum()) for x0 in range(0, len(on), 256)]


SIZES = [1, 15, 16, 17, 63, 64, 65, 257]


def sized(W, H):
    return ii.random_fill(0.5, W, H, 2, seed=1000 * W + H)


PAINTED = {
    "checkerboard": ii.checkerboard,
    "row_end_17": lambda: row_end(17),
    "row_end_16": lambda: row_end(16),
    "boundaries": boundaries,
    "corners": corners,
    "random_50": lambda: ii.random_fill(0.5, seed=5),
    "tall_thin": tall_thin,
    "chunked": ii.chunked,
    "dense_511": lambda: dense(511),
    "dense_512": lambda: dense(512),
    "dense_512_ends": lambda: dense(512, True),
}
