"""Painted image stacks for the island tests -- TEST INFRASTRUCTURE ONLY.

painted(bits) turns an L x H x W bit pattern into an sdf_3d node whose table nodes are the raster samples
of (rect, W, H, s = 1) and of the planes z, as test_gpu_mass.zero_node() builds one: the field at a sample
is the table entry negated, so an entry of -1 is a solid pixel and +1 an empty one, and the pattern is the
exact image stack.  The grid size is 2^-6 and the rect starts at 0: edges k / 64 and samples (k + 0.5) / 64
are exact in float32 (asserted without a GPU in test_cpu_islands.py).  Every table fits the sdf_3d limits
(2 .. 512 per axis, at most 2^22 entries); axes shorter than 2 are padded with empty entries that no
sample reads.
"""
import numpy as np

import np_sdf3d

GS = 2.0 ** -6
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def painted(bits):
    """bits (L, H, W) -> (node, rect, z float32 (L,))"""
    bits = np.asarray(bits, bool)
    L, H, W = bits.shape
    sz, sy, sx = max(L, 2), max(H, 2), max(W, 2)
    assert max(sx, sy, sz) <= 512 and sx * sy * sz <= 1 << 22
    vals = np.ones((sz, sy, sx), np.float32)
    vals[:L, :H, :W] = np.where(bits, np.float32(-1), np.float32(1))
    node = np_sdf3d.node(np_sdf3d.Table(vals.reshape(-1), (sx, sy, sz), GS, (0.5 * GS, 0.5 * GS, 0.5 * GS)), EYE)
    rect = [0.0, W * GS, 0.0, H * GS]
    z = ((np.arange(L) + 0.5) * GS).astype(np.float32)
    return node, rect, z


def checkerboard():
    y, x = np.mgrid[0:129, 0:129]
    return ((x + y) % 2 == 0)[None]


def serpentine():
    """one pixel wide over 65 x 33: every even row, joined alternately at the right and the left end"""
    W, H = 65, 33
    b = np.zeros((1, H, W), bool)
    b[0, 0::2, :] = True
    for y in range(1, H, 2):
        b[0, y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    return b


def u_shape():
    """two arms in tiles 0 and 1 that meet only in the last row (row 39, the second tile row)"""
    b = np.zeros((1, 40, 70), bool)
    b[0, :, 2] = True
    b[0, :, 67] = True
    b[0, 39, 2:68] = True
    return b


def rings():
    """square outlines at insets 1, 4, 7, ...: two empty pixels between neighbours"""
    b = np.zeros((1, 70, 70), bool)
    for i in range(1, 34, 3):
        b[0, i, i:70 - i] = b[0, 69 - i, i:70 - i] = True
        b[0, i:70 - i, i] = b[0, i:70 - i, 69 - i] = True
    return b


def diagonals():
    """pairs of diagonal neighbours: layer 0 at the tile corner (64, 32), across the 64-pixel seam only and
    across the tile-row border only; layer 1 the other diagonal at each place"""
    b = np.zeros((2, 40, 70), bool)
    for x, y in ((63, 31), (64, 32), (63, 10), (64, 11), (20, 31), (21, 32)):
        b[0, y, x] = True
    for x, y in ((64, 31), (63, 32), (64, 10), (63, 11), (21, 31), (20, 32)):
        b[1, y, x] = True
    return b


def random_fill(p, W=70, H=70, L=2, seed=3):
    return np.random.default_rng(seed).random((L, H, W)) < p


def supports():
    """four layers of 40 x 40 with designated components of layer 1: an island (below 0), one resting on a
    single pixel, one resting on half of itself, and in layer 2 one resting on all of itself"""
    b = np.zeros((4, 40, 40), bool)
    b[0, 2:10, 2:10] = True        # A
    b[0, 2:8, 30:36] = True        # P
    b[1, 20:25, 20:25] = True      # the island: nothing of layer 0 under it
    b[1, 9:15, 9:15] = True        # rests on A's pixel (9, 9) only
    b[1, 2:8, 33:39] = True        # rests on P with columns 33 .. 35: 18 of its 36 pixels
    b[2, 20:25, 20:25] = True      # rests on the island with all of itself
    b[3, 0:40:3, 0:40:3] = True    # single pixels, some over layer 2's square
    return b


def chunked():
    """twelve layers of 40 x 40 (nine raster tiles a layer): a supported square in every layer, an island on
    layers 4 and 8 (the first layers of the chunks of four), supported from the layer after, and noise"""
    b = np.zeros((12, 40, 40), bool)
    b[:, 2:12, 2:12] = True
    b[4:7, 20:26, 20:26] = True
    b[8:, 5:10, 30:35] = True
    b[:, 28:40, :] = np.random.default_rng(11).random((12, 12, 40)) < 0.5
    return b


SIZES = [1, 15, 16, 17, 63, 64, 65]


def sized(W, H):
    return random_fill(0.6, W, H, 2, seed=100 * W + H)


PAINTED = {
    "checkerboard": checkerboard,
    "serpentine": serpentine,
    "u_shape": u_shape,
    "rings": rings,
    "diagonals": diagonals,
    "random_55": lambda: random_fill(0.55),
    "random_60": lambda: random_fill(0.6, seed=4),
    "supports": supports,
    "chunked": chunked,
}
