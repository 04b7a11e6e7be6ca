"""Painted image stacks for the support-tip tests -- TEST INFRASTRUCTURE ONLY.

island_inputs.painted() turns a bit pattern into a shape whose layer images are exactly the pattern.  The stacks
below are what placing tips and finding their feet can get wrong and a distance field cannot: cells that end at and
off the lane-group, wave and block edges, cells whose deepest pixels tie, layers without any tip, and columns whose
foot lies in the tip's chunk, in the chunk before, several chunks back or on the plate.
"""
import numpy as np

import distance_inputs as di
import island_inputs as ii

painted = ii.painted
SIZES = ii.SIZES
CELLS = [1, 3, 16, 17, 64, 16384]


def sized(W, H):
    """three layers of W x H, each over a different random layer: unsupported pixels all over the image"""
    return ii.random_fill(0.6, W, H, 3, seed=100 * W + H + 3)


ISLAND_AT = (10, 9)   # (px, py) of the island's first pixel


def island_start():
    """a 4 x 4 island starts in layer 1 over an empty layer 0: its four middle pixels are equally deep"""
    b = np.zeros((2, 20, 24), bool)
    x, y = ISLAND_AT
    b[1, y:y + 4, x:x + 4] = True
    return b


def solid_over_empty():
    """every depth of layer 1 is NONE: each cell's tip is its smallest p"""
    b = np.zeros((2, 17, 33), bool)
    b[1] = True
    return b


def solid_over_solid():
    return np.ones((2, 17, 33), bool)


def plate_only():
    """one layer: it rests on the plate"""
    b = np.zeros((1, 17, 33), bool)
    b[0, 3:9, 3:20] = True
    return b


TIES = {"island_start": island_start, "solid_over_empty": solid_over_empty, "solid_over_solid": solid_over_solid,
        "plate_only": plate_only}
TIE_CELLS = [1, 3, 16, 16384]

SLAB_TOP = 2      # the slab's last layer
PATCH = 4         # the layer of a patch one empty layer above the slab
SHELF = 7         # the shelf's first layer
PILLAR_AT = (30, 30)   # (px, py) of the single voxel of layer 0


def shelf():
    """twelve layers of 40 x 40 (nine raster tiles a layer).  A slab in layers 0 .. 2, a patch over it in layer 4 (one
    empty layer between: foot = l - 2), four empty layers, then in layer 7 a shelf over the slab (foot = the slab's
    top) that runs on beside it (foot = -1), and a second piece over a single voxel of layer 0 (foot = 0).  Layer 8
    repeats the shelf (supported), layer 9 widens it, layers 10 and 11 are a smaller square over it and noise."""
    b = np.zeros((12, 40, 40), bool)
    b[0:SLAB_TOP + 1, 5:20, 5:20] = True
    b[0, PILLAR_AT[1], PILLAR_AT[0]] = True
    b[PATCH, 8:12, 8:13] = True
    b[SHELF:SHELF + 2, 5:20, 5:36] = True
    b[SHELF:SHELF + 2, 28:33, 28:33] = True
    b[SHELF + 2, 3:24, 3:38] = True
    b[10:, 6:18, 6:30] = True
    b[11, 30:40, :] = np.random.default_rng(12).random((10, 40)) < 0.4
    return b


# the shelf stack's planes repeated and out of order: entry l of z is plane SHELF_ORDER[l]
SHELF_ORDER = [0, 1, 2, 2, 7, 7, 3, 4, 0, 9, 11, 2, 8]


def shelf_reordered():
    return shelf()[SHELF_ORDER]


def painted_reordered():
    """(bits, node, rect, z): the shelf's shape sampled on its planes in SHELF_ORDER"""
    node, rect, z = painted(shelf())
    return shelf_reordered(), node, rect, z[SHELF_ORDER]


FEET = {"shelf": shelf, "shelf_reordered": shelf_reordered}
FOOT_CELLS = [1, 16]
# tile items per chunk: nine raster tiles a layer, so a layer and four layers per chunk
FOOT_CHUNKS = {"1": 1, "36": 4}

EXISTING = {
    "staircase": di.staircase,
    "supports": ii.supports,
    "random_50": lambda: ii.random_fill(0.5, L=4, seed=21),
    "random_95": lambda: ii.random_fill(0.95, L=4, seed=22),
}
EXISTING_CELLS = [1, 3, 16]
EXISTING_REACH2 = [0, 4]
