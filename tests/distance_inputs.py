"""Painted image stacks for the distance field tests -- TEST INFRASTRUCTURE ONLY.

island_inputs.painted() turns a bit pattern into a shape whose layer images are exactly the pattern; the
islands' nine stacks are taken over and the ones below added: what a distance transform can get wrong and a
labelling cannot (layers of one class, distances that cross every tile, long searches on either sign,
overhangs of a known reach).
"""
import numpy as np

import island_inputs as ii

painted = ii.painted
SIZES = ii.SIZES
sized = ii.sized


def one_class():
    """all solid, all empty, all solid again: every distance is NONE, and layer 2 stands on nothing"""
    b = np.zeros((3, 17, 33), bool)
    b[0] = b[2] = True
    return b


HOLE = (40, 33)   # (px, py)


def one_hole():
    """70 x 70 solid but for one pixel: every distance is to that pixel, across every tile"""
    b = np.ones((1, 70, 70), bool)
    b[0, HOLE[1], HOLE[0]] = False
    return b


DOT = (30, 4)


def one_pixel():
    b = np.zeros((1, 21, 37), bool)
    b[0, DOT[1], DOT[0]] = True
    return b


def disc():
    y, x = np.mgrid[0:70, 0:70]
    return ((x - 35) ** 2 + (y - 35) ** 2 <= 400)[None]


def stripes():
    """solid and empty stripes of widths 1 to 7, layer 0 along y (vertical), layer 1 along x"""
    line = np.zeros(60, bool)
    at = 0
    for w in range(1, 8):
        line[at:at + w] = True
        at += 2 * w
    b = np.zeros((2, 60, 60), bool)
    b[0] = line[None, :]
    b[1] = line[:, None]
    return b


STAIR_STEPS = [(l + 1) % 4 for l in range(12)]   # layer l overhangs layer l - 1 by this many pixels in x and in y
STAIR_REACH2 = (0, 1, 4, 8)


def staircase():
    """twelve layers of 40 x 40 (nine raster tiles a layer): a square from (5, 5) whose far corner moves out by
    STAIR_STEPS[l] pixels in x and y from layer l - 1 to l, so the corner of a step of 2 holds pixels at squared
    distances 2, 5 and 8 from the layer below and a step of 3 up to 18; the first layers of chunks of four
    (4 and 8) overhang by 1"""
    b = np.zeros((12, 40, 40), bool)
    edge = 10
    for l in range(12):
        edge += STAIR_STEPS[l] if l else 0
        b[l, 5:edge, 5:edge] = True
    return b


PAINTED = dict(ii.PAINTED)
PAINTED.update({
    "one_class": one_class,
    "one_hole": one_hole,
    "one_pixel": one_pixel,
    "disc": disc,
    "stripes": stripes,
    "random_05": lambda: ii.random_fill(0.05, seed=5),
    "random_50": lambda: ii.random_fill(0.5, seed=6),
    "random_95": lambda: ii.random_fill(0.95, seed=7),
    "staircase": staircase,
})
