"""Painted stacks for the tests of the bodies query -- TEST INFRASTRUCTURE ONLY.

Bit patterns (L, H, W), True = solid, painted through island_inputs.painted (an sdf_3d table, exact in float32;
its limits are 512 entries per axis and 2^22 in all).  What each holds is asserted without a GPU in
test_cpu_bodies.py.
"""
import itertools

import numpy as np

import island_inputs as ii
import run_inputs as ri

SIZES = ii.SIZES
LAYERS = [1, 2, 3]


def arch(bridge=4):
    """five layers of 70 x 40: one-pixel pillars at x = 2 and x = 67 (row 20) through every layer, joined only by a
    bridge along row 20 in layer `bridge` (None: no bridge)"""
    b = np.zeros((5, 40, 70), bool)
    b[:, 20, 2] = True
    b[:, 20, 67] = True
    if bridge is not None:
        b[bridge, 20, 2:68] = True
    return b


# the thirteen directions (dl, dy, dx) of the half space: with their opposites the 26 neighbours
HALF = [d for d in itertools.product((0, 1), (-1, 0, 1), (-1, 0, 1)) if d > (0, 0, 0)]
CONTACT_H = 6


def contact_pairs():
    """[(direction, voxel a, voxel b = a + direction)]: for every direction of HALF a pair in layers 3 k and 3 k + dl,
    once in rows 0 .. 1 and once in the last two rows, always on the columns 63 | 64 (both on 63 where dx = 0)"""
    out = []
    for k, (dl, dy, dx) in enumerate(HALF):
        for last in (False, True):
            if last:
                ya = CONTACT_H - 1 - max(dy, 0)
            else:
                ya = max(-dy, 0)
            xa = 64 if dx < 0 else 63
            a = (3 * k, ya, xa)
            out.append(((dl, dy, dx), a, (a[0] + dl, a[1] + dy, a[2] + dx)))
    return out


def contacts():
    """voxel pairs that touch by a face only, an edge only or a corner only, in every direction: across layers, rows,
    columns and their combinations.  Pairs are at least two steps apart in l or in y"""
    b = np.zeros((3 * len(HALF) - 1, CONTACT_H, 70), bool)
    for _, a, c in contact_pairs():
        b[a] = b[c] = True
    return b


HELIX_LAYER = [0, 1, 2, 3, 2, 1]


def helix():
    """a one-voxel path through 65 x 33 x 4: every even row 2 k is filled in one layer (0 1 2 3 2 1 0 ...), and
    between rows 2 k and 2 k + 2 the path steps one row, climbs (or descends) a layer and steps another row, at
    the right end for even k and at the left end for odd k"""
    W, H, L = 65, 33, 4
    b = np.zeros((L, H, W), bool)
    for k in range(17):
        la = HELIX_LAYER[k % 6]
        b[la, 2 * k, :] = True
        if k < 16:
            lb = HELIX_LAYER[(k + 1) % 6]
            x = W - 1 if k % 2 == 0 else 0
            b[la, 2 * k + 1, x] = b[lb, 2 * k + 1, x] = True
    return b


def cavities():
    """a solid 24 x 24 x 7 block that fills the stack, with four voids: one enclosed (A); one open to the top layer
    (B); one open to the x = 0 side (C); one (D) whose only way out is the corner contact (3, 18, 18) | (4, 19, 19)
    with a shaft (E) that is open to the top layer"""
    b = np.ones((7, 24, 24), bool)
    b[2:4, 3:6, 3:6] = False        # A
    b[4:7, 3:6, 10:13] = False      # B
    b[3, 12:14, 0:5] = False        # C
    b[2:4, 16:19, 16:19] = False    # D
    b[4:7, 19:21, 19:21] = False    # E
    return b


def floating():
    """five layers of 20 x 20: a plate-bound block; a block that starts in layer 2 and touches nothing; a part that
    starts as an island of layer 1 and joins the plate-bound block through a bar in layer 3"""
    b = np.zeros((5, 20, 20), bool)
    b[0:5, 2:6, 2:6] = True
    b[2:4, 12:15, 12:15] = True
    b[1:4, 2:6, 9:12] = True
    b[3, 3, 6:9] = True
    return b


def dense_rows():
    """130 x 3 x 3, the 3D checkerboard: alternating pixels, shifted by one from row to row and from layer to layer;
    65 runs in every row"""
    l, y, x = np.mgrid[0:3, 0:3, 0:130]
    return (x + y + l) % 2 == 0


def random_fill(p, seed):
    return np.random.default_rng(seed).random((6, 70, 70)) < p


def sized(W, H, L):
    return np.random.default_rng(10000 * L + 100 * W + H).random((L, H, W)) < 0.6


GROWING_NOISE = [2, 6, 12, 24, 40, 70, 110, 170, 260, 380]   # single pixels in rows 8 .. 19 of layer l


def growing():
    """ten layers of 64 x 24 whose run count rises from layer to layer, for a stack whose arrays outgrow their
    block from chunk to chunk (a layer per chunk).  Rows 0 .. 1: a pillar of 2 x 2 pixels through every layer,
    the stack's first run.  Rows 3 .. 5: a block in layers 0 .. 1 and, apart from it, a block in layers 7 .. 9.
    Rows 8 .. 19: single pixels on even columns, GROWING_NOISE[l] of them in layer l, every layer's a superset of
    the layer's below.  Row 22: one-pixel pillars at x = 40 and x = 60 through every layer, joined only by a bar in
    the last.  Rows 2, 6 .. 7 and 20 .. 21 are empty: the four parts touch neither each other nor the pixels"""
    L, H, W = len(GROWING_NOISE), 24, 64
    b = np.zeros((L, H, W), bool)
    b[:, 0:2, 0:2] = True
    b[0:2, 3:6, 10:15] = True
    b[7:10, 3:6, 30:35] = True
    b[:, 22, 40] = b[:, 22, 60] = True
    b[L - 1, 22, 40:61] = True
    at = (131 * np.arange(12 * 32)) % (12 * 32)   # a fixed order of the places: 131 and 384 have no common factor
    for l, n in enumerate(GROWING_NOISE):
        b[l, 8 + at[:n] // 32, 2 * (at[:n] % 32)] = True
    return b


def rounds():
    """two layers of two rows of 512 pixels for the passes that take a row's runs 64 at a time.  Layer 0: row 0 is
    solid over [0, 300); row 1 holds a pixel at every even x, 256 runs, of which the first 150 stand under row 0:
    under 6 its first two rounds of 64 runs are of row 0's body, the third holds 22 of them and 42 bodies of one
    pixel, the fourth 64 such bodies.  Layer 1: a bar over [401, 404) of row 0 that touches nothing under 6, and
    row 1 solid over [0, 290) and pixels at every fourth x behind it (292, 296, ...), over pixels of layer 0"""
    b = np.zeros((2, 2, 512), bool)
    b[0, 0, 0:300] = True
    b[0, 1, 0::2] = True
    b[1, 0, 401:404] = True
    b[1, 1, 0:290] = True
    b[1, 1, 292::4] = True
    return b


def empty():
    return np.zeros((3, 17, 65), bool)


def full():
    return np.ones((3, 17, 65), bool)


PAINTED = {
    "arch": arch,
    "arch_open": lambda: arch(None),
    "arch_bottom": lambda: arch(0),
    "contacts": contacts,
    "helix": helix,
    "cavities": cavities,
    "floating": floating,
    "dense_rows": dense_rows,
    "random_50": lambda: random_fill(0.5, 5),
    "random_60": lambda: random_fill(0.6, 6),
    "empty": empty,
    "full": full,
    "chunked": ii.chunked,
    "growing": growing,
    "rounds": rounds,
    # rows of two full steps of the walk and of two and three rounds of 64 runs, on irregular data
    "dense_511": ri.PAINTED["dense_511"],
    "dense_512": ri.PAINTED["dense_512"],
    "dense_512_ends": ri.PAINTED["dense_512_ends"],
}
