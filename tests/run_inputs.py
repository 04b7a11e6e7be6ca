"""Painted image stacks for the run-length tests -- TEST INFRASTRUCTURE ONLY.

Bit patterns (L, H, W) for island_inputs.painted(), which turns one into an sdf_3d node whose table nodes are
the raster samples: the pattern is the exact image stack.  Each is built around one place where a run-length
walk can go wrong: the step from a row's last real pixel to the next row's first (the image rows are padded to
a multiple of 16 bytes, so with W = 17 the byte in front of a row's first is a padding zero, with W = 16 it is
the pixel itself), the seams of a walk of 64 lanes with four pixels each (63 | 64, 255 | 256), the first and
the last pixel of the stream, and more rows in a chunk than one tile of the scan (4096).  The preconditions are
asserted without a GPU in test_cpu_runs.py.
"""
import numpy as np

import island_inputs as ii


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
}
