"""Painted stacks for the tests of the suction-cup query -- TEST INFRASTRUCTURE ONLY.

Bit patterns (L, H, W), True = solid, painted through island_inputs.painted; layer 0 stands on the plate.  Each is
built for one way the kernels can go wrong; what each holds is asserted without a GPU in test_cpu_cups.py.
"""
import numpy as np

import body_inputs as bi

BOX = (slice(3, 17), slice(4, 18))      # the glass's outline in a 20 x 22 layer: rows 3 .. 16, columns 4 .. 17
INSIDE = (slice(4, 16), slice(5, 17))   # what its one-pixel wall encloses: 12 x 12 pixels
VENT_LAYER = 4
MERGE_LAYER = 5


def glass_up(L=8):
    """a floor in layer 0 and one-pixel walls above it, open at the last layer: a cup at every layer past the floor"""
    b = np.zeros((L, 20, 22), bool)
    b[(slice(None),) + BOX] = True
    b[(slice(1, None),) + INSIDE] = False
    return b


def glass_down():
    """a dome on the plate: walls in layers 0 .. 4, the roof in layer 5, two empty layers above"""
    b = np.zeros((8, 20, 22), bool)
    b[(slice(0, 6),) + BOX] = True
    b[(slice(0, 5),) + INSIDE] = False
    return b


def glass_down_raised():
    """the same behind an empty first plane: the dome does not stand on the plate, and its inside is open"""
    return np.concatenate((np.zeros((1, 20, 22), bool), glass_down()))


def glass_side():
    """the mouth faces +x with free space around: a floor of the box's outline in layer 0, a roof in the last layer, 6,
    and the wall at column 17 missing in between"""
    b = glass_up(7)
    b[(6,) + BOX] = True
    b[1:6, 4:16, 17] = False
    return b


def vented(v=VENT_LAYER):
    """glass_up with a one-pixel hole through the wall (row 10, column 4) at layer v"""
    b = glass_up(8)
    b[v, 10, 4] = False
    return b


def u_bend():
    """a solid block with a channel: a bend along row 10 in layers 1 .. 2, and above its ends two arms (columns 6 .. 7
    and 22 .. 23) through layers 3 .. 6, open at the last layer"""
    b = np.zeros((7, 20, 30), bool)
    b[:, 3:17, 3:27] = True
    b[1:3, 9:12, 6:24] = False
    b[3:, 9:12, 6:8] = False
    b[3:, 9:12, 22:24] = False
    return b


def merge(opened=False):
    """a solid block with two shafts, A (columns 5 .. 7) from layer 1 and B (columns 14 .. 16) from layer 2, both
    through the last layer, joined by a tunnel along row 6 in layer MERGE_LAYER.  opened: a one-pixel hole from B
    through the block's side in layer 3"""
    b = np.zeros((8, 14, 24), bool)
    b[:, 2:12, 2:22] = True
    b[1:, 5:8, 5:8] = False
    b[2:, 5:8, 14:17] = False
    b[MERGE_LAYER, 6, 8:14] = False
    if opened:
        b[3, 6, 17:22] = False
    return b


def sealed():
    """a solid block with a void in layers 2 .. 4, closed on all sides"""
    b = np.zeros((8, 16, 18), bool)
    b[:7, 2:14, 2:16] = True
    b[2:5, 5:9, 6:12] = False
    return b


SIDES = ("x0", "x1", "y0", "y1")


def frame_only(side):
    """a stack that is solid up to the frame with two voids in layers 0 .. 4.  From layer 3 on a one-pixel channel
    leads from the first void to a single frame pixel of the given side, and one from the second void to the pixel
    in front of the frame"""
    H, W = 19, 21
    b = np.ones((5, H, W), bool)
    b[:, 4:7, 8:12] = False       # the first void
    b[:, 12:15, 8:12] = False     # the second
    if side == "x0":
        b[3:, 5, 0:8] = False
        b[3:, 13, 1:8] = False
    elif side == "x1":
        b[3:, 5, 12:W] = False
        b[3:, 13, 12:W - 1] = False
    elif side == "y0":
        b[3:, 0:4, 9] = False
        b[3:, 8:12, 9] = False    # ends at row 8, far from any frame: the control stays closed
    else:
        b[3:, 7:10, 9] = False    # the first void's channel ends at row 9: closed
        b[3:, 15:H, 10] = False   # the second void's reaches row H - 1
    return b


def diagonal():
    """glass_up whose wall lacks the corner pixel (3, 4) at layer 4: the inside corner (4, 5) touches it by a corner
    only, so the glass leaks under 26 and holds under 6"""
    b = glass_up(8)
    b[4, 3, 4] = False
    return b


def framed(bits):
    """a stack with a solid row added in front of row 0 and behind the last row: its rows touch the frame at their ends only"""
    return np.pad(bits, ((0, 0), (1, 1), (0, 0)), constant_values=True)


def long_rows(W):
    """three layers of seven rows of W pixels (256: the walk's step; 257: one past it), solid but for noise in layer 2's
    row 1, a pocket in row 3 over columns 200 .. W - 2, one pixel short of the frame, and one in row 5 over columns
    100 .. W - 1, which reaches it"""
    b = np.ones((3, 7, W), bool)
    b[2, 1, 1:W - 1] = np.random.default_rng(W).random(W - 2) < 0.5
    b[:, 3, 200:W - 1] = False
    b[:, 5, 100:W] = False
    return b


def growing():
    """body_inputs.growing inverted: the single pixels are voids now, more in every layer, so the empty
    row runs outgrow their block chunk by chunk (a layer per chunk); the blocks are closed voids, the pair of pillars
    two pockets that join in the last layer, and the pillar in the corner is open"""
    return ~bi.growing()


PAINTED = {
    "glass_up": glass_up,
    "glass_down": glass_down,
    "glass_down_raised": glass_down_raised,
    "glass_side": glass_side,
    "vented": vented,
    "u_bend": u_bend,
    "merge": merge,
    "merge_open": lambda: merge(True),
    "sealed": sealed,
    "frame_only_x0": lambda: frame_only("x0"),
    "frame_only_x1": lambda: frame_only("x1"),
    "frame_only_y0": lambda: frame_only("y0"),
    "frame_only_y1": lambda: frame_only("y1"),
    "diagonal": diagonal,
    # rows of more than 64 runs
    "dense_rows": bi.dense_rows,
    "rounds": bi.rounds,
    "arch": bi.arch,
    "dense_rows_framed": lambda: framed(bi.dense_rows()),
    "rounds_framed": lambda: framed(bi.rounds()),
    "arch_inverted": lambda: ~bi.arch(),
    "long_256": lambda: long_rows(256),
    "long_257": lambda: long_rows(257),
    "all_solid": bi.full,
    "all_empty": bi.empty,
    "growing": growing,
    "chunked": lambda: ~bi.PAINTED["chunked"](),
}
# the stacks without a cup under either connectivity: their tests pin "nothing is reported"
TRIVIAL = {"glass_down_raised", "glass_side", "rounds", "arch", "all_solid", "all_empty"}
