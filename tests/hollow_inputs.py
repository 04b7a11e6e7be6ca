"""Painted image stacks for the hollowing tests -- TEST INFRASTRUCTURE ONLY.

island_inputs.painted() turns a bit pattern into a shape whose layer images are exactly the pattern.  The stacks
below are what a window over the layers can get wrong and a single layer's distance field cannot: a block whose
core is known in closed form, the same block against the ends of the stack, one empty voxel whose shell is the
digital ellipsoid, stacks shorter than the reach, and the distance tests' stacks deepened to several layers.
"""
import numpy as np

import distance_inputs as di
import island_inputs as ii

painted = ii.painted
SIZES = ii.SIZES

BOX_WALL = (3, 1)            # hollow_wall2's arguments: [9, 8, 5, 0]
BOX_AT = (4, 4, 1)           # (px, py, l) of the block's first voxel
BOX_SIZE = (40, 40, 12)      # in (x, y, l)


def box():
    """a 40 x 40 x 12 block inside 48 x 48 x 14: an empty margin on every side"""
    b = np.zeros((14, 48, 48), bool)
    x, y, l = BOX_AT
    b[l:l + BOX_SIZE[2], y:y + BOX_SIZE[1], x:x + BOX_SIZE[0]] = True
    return b


def box_core(inset=3):
    """the block shrunk by `inset` voxels on every side"""
    b = np.zeros((14, 48, 48), bool)
    x, y, l = BOX_AT
    b[l + inset:l + BOX_SIZE[2] - inset, y + inset:y + BOX_SIZE[1] - inset, x + inset:x + BOX_SIZE[0] - inset] = True
    return b


def box_touching():
    """the block through all 14 layers: it touches layers 0 and 13"""
    b = np.zeros((14, 48, 48), bool)
    b[:, 4:44, 4:44] = True
    return b


HOLE = (40, 33, 4)   # (px, py, l)
HOLE_WALLS = {"isotropic": (4, 1), "anisotropic": (4, 2.5)}


def one_hole():
    """70 x 70 x 9 solid but for one middle voxel: the shell is the digital ellipsoid round it, across every tile"""
    b = np.ones((9, 70, 70), bool)
    b[HOLE[2], HOLE[1], HOLE[0]] = False
    return b


def one_class():
    """all solid, all empty, all solid again, and three more solid layers: every distance is NONE"""
    b = np.zeros((6, 17, 33), bool)
    b[0] = b[2] = b[3] = b[4] = b[5] = True
    return b


PAINTED = {
    "staircase": di.staircase,
    "random_50": lambda: ii.random_fill(0.5, L=6, seed=16),
    "random_95": lambda: ii.random_fill(0.95, L=6, seed=17),
    "one_class": one_class,
}
# per reach: a table whose every entry decides something on these stacks
WALLS = {0: [4], 1: [4, 1], 4: [5, 4, 2, 1, 0]}


def sized(W, H):
    """three dense layers of W x H"""
    return ii.random_fill(0.97, W, H, 3, seed=100 * W + H + 7)


SIZED_WALL = [1, 0]

DEPTH_REACH = 3
DEPTH_WALL = [4, 2, 1, 0]
DEPTHS = sorted({1, 2, DEPTH_REACH, DEPTH_REACH + 1, 2 * DEPTH_REACH + 1, 2 * DEPTH_REACH + 2})


def deep(n_layers):
    """n layers of 33 x 21, dense, with a column of empty voxels that moves through the layers"""
    b = np.random.default_rng(40 + n_layers).random((n_layers, 21, 33)) < 0.985
    for l in range(n_layers):
        b[l, 10, 3 + 4 * (l % 7)] = False
    return b


FAR_REACH_WALL = [3] * 6 + [1] * 3   # reach 8 over a stack of five layers


def shallow():
    return deep(5)
