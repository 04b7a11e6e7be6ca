"""Inputs and references of the slicer's edge tests -- TEST INFRASTRUCTURE ONLY.  No GPU.

tests/test_gpu_slice_edges.py compares implisolid_slice with np_slice.march of the field values built
here; tests/test_cpu_slice.py asserts that these inputs still hold what the GPU tests rely on (every
marching-squares case, a full tile, negative zeros, unequal axes, long item lists), so an edit that
spoils them fails without a GPU.  The field values come from np_sdf3d.evaluate (an sdf_3d table
dictates them sample by sample) or from the oracle: never from the slicing kernels.  A reference is
computed once per process and left unchanged.
"""
import json

import numpy as np

import np_sdf3d
import np_slice
from implisolid_amd import scenes
from test_gpu_parity import SCREW_TREES
from test_gpu_slice import DIFFERENCE, EGG, SHAPES, Z as Z6

f32 = np.float32
EYE = scenes.EYE
T = np_slice.T
SQUARE = [-1, 1, -1, 1]
N_SEG = np.zeros(16, np.int64)   # segments per case
for _c, _s in np_slice.SEGMENTS.items():
    N_SEG[_c] = len(_s)


class Ref:
    """One grid's sample coordinates, reference field F (L, R + 1, R + 1) and its marched slices."""

    def __init__(self, rect, R, z, F):
        self.rect, self.R, self.z = np.array(rect, f32), R, np.asarray(z, f32)
        self.xs, self.ys = np_slice.coords(rect, R)
        self.F = np.asarray(F(np_slice.points(self.xs, self.ys, self.z)), f32).reshape(len(self.z), R + 1, R + 1)
        self.seg, self.keys, self.offs = np_slice.march(self.F, self.xs, self.ys)

    def tile_counts(self, l):
        """segments per tile of layer l (tiles row-major), from the cases alone"""
        n = N_SEG[np_slice.cases(self.F[l])]
        nt = (self.R + T - 1) // T
        return np.array([[n[T * ty:T * ty + T, T * tx:T * tx + T].sum() for tx in range(nt)] for ty in range(nt)])

    def histogram(self, l):
        return np.bincount(np_slice.cases(self.F[l]).reshape(-1), minlength=16)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_field(oracle, shape, ignore_root_matrix=False):
    tree = oracle.mp5_to_nodes(json.dumps(shape), ignore_root_matrix)
    return lambda pts: oracle.eval_implicit(tree, pts)


# ---- 1. injected fields: all sixteen cases, a full tile, negative zeros -----------------------------
INJ_S = 34
INJ_Z = np.array([-0.0625, 0, 0.03125, 0.0625, 0], f32)   # three node planes, a halfway plane, a repeat
INJ_ALIGNED = {0: 0, 1: 1, 3: 2, 4: 1}                     # layer -> the table's z index on the node planes
# name -> (rect, R, aligned): on the aligned grids both steps are exactly 0.0625 and every sample of a
# node plane is a table entry; the third grid cuts the same table at general fractions
INJ_GRIDS = {"r32": ([-1, 1, -1, 1], 32, True), "r33": ([-1, 1.0625, -1, 1.0625], 33, True),
             "r40": ([-0.97, 1.0, -1.0, 0.93], 40, False)}


def injected_values():
    """(3, S, S) float32 indexed [z][y][x]: random levels with exact zeros, a checkerboard quadrant
    (every cell a saddle: 512 segments in tile (0, 0)) and a quiet quadrant."""
    rng = np.random.default_rng(11)
    vals = rng.choice(np.array([-1, -0.5, -0.25, 0, 0.25, 0.75, 1], f32), size=(3, INJ_S, INJ_S))
    j, i = np.meshgrid(np.arange(17), np.arange(17), indexing="ij")
    vals[:, :17, :17] = np.where((i + j) % 2 == 0, f32(0.5), f32(-0.75))
    vals[:, 17:, 17:] = f32(0.5)
    return vals


def injected_node():
    def make():
        vals = injected_values()
        return np_sdf3d.node(np_sdf3d.Table(vals.reshape(-1), (INJ_S, INJ_S, 3), 0.0625, (-1, -1, -0.0625)), EYE)
    return _cached("inj_node", make)


def injected_ref(grid):
    rect, R, _ = INJ_GRIDS[grid]
    node = injected_node()
    return _cached(("inj", grid), lambda: Ref(rect, R, INJ_Z, lambda p: np_sdf3d.evaluate(node, p[:, 0], p[:, 1], p[:, 2])))


# ---- 2. unequal axes ----------------------------------------------------------------------------------
UNEQUAL_RECT = [-0.35, 0.85, -0.5, 0.25]
UNEQUAL_R = 40
UNEQUAL_NAMES = ["difference", "egg", "tree_deep"]
# the egg far from the origin on a tiny rect: the coordinates' ulp is 2^-14, 1/205 of the x step
FAR_RECT = [1000, 1000.5, -1000.25, -1000]
FAR_EGG = dict(EGG, matrix=[0.5, 0, 0, 1000.25, 0, 0.25, 0, -1000.125, 0, 0, 1, 0.1875])


def unequal_ref(oracle, name):
    return _cached(("unequal", name), lambda: Ref(UNEQUAL_RECT, UNEQUAL_R, Z6, oracle_field(oracle, SHAPES[name])))


def far_ref(oracle):
    return _cached("far", lambda: Ref(FAR_RECT, UNEQUAL_R, Z6, oracle_field(oracle, FAR_EGG)))


# ---- 3. resolutions at the tile edges ---------------------------------------------------------------
# the egg's centre is (0.25, -0.125, 0.1875), its radii 1/4, 1/8, 1/2: at R = 1 the single cell has
# only its (xmax, ymax) corner inside on z = 0.1875
SMALL_RECT = [-0.05, 0.3, -0.325, -0.105]
SMALL_Z = np.array([0.1875, 0.3], f32)
SMALL_RS = [1, 2, 15, 16, 17, 31]


def small_ref(oracle, R):
    return _cached(("small", R), lambda: Ref(SMALL_RECT, R, SMALL_Z, oracle_field(oracle, EGG)))


# ---- 4. item lists longer than one scan tile (4096 items) ---------------------------------------------
# R = 17: four tiles per layer, of 16 x 16, 1 x 16, 16 x 1 and 1 x 1 cells
LONG_R = 17
LONG = {"egg": np.linspace(-0.4, 0.75, 2100).astype(f32),        # 8400 items: three scan tiles, the last partial
        "tree_deep": np.linspace(-0.9, 0.9, 1100).astype(f32)}   # 4400 items: two scan tiles


def long_ref(oracle, name):
    return _cached(("long", name), lambda: Ref(SQUARE, LONG_R, LONG[name], oracle_field(oracle, SHAPES[name])))


# ---- 5. planes of exact zeros and ignore_root_matrix --------------------------------------------------
LID = SCREW_TREES["lid"]                                          # cylinder and top_bottom_lid
BARE_LID = {"type": "top_bottom_lid", "matrix": scenes.st(1, 0, 0, 0)}
LID_R = 32
LID_Z = np.array([-0.5, 0, 0.5], f32)
MOVED_DIFFERENCE = dict(DIFFERENCE, matrix=scenes.st(0.75, 0.1, -0.05, 0.02))
ROOT_R = 40


def lid_ref(oracle, bare):
    return _cached(("lid", bare), lambda: Ref(SQUARE, LID_R, LID_Z, oracle_field(oracle, BARE_LID if bare else LID)))


def root_ref(oracle, which):
    """'eye': DIFFERENCE as it stands (root matrix EYE); 'moved': with the root matrix, flag off;
    'ignored': the oracle's own reading of the moved tree with ignore_root_matrix"""
    shape, flag = {"eye": (DIFFERENCE, False), "moved": (MOVED_DIFFERENCE, False), "ignored": (MOVED_DIFFERENCE, True)}[which]
    return _cached(("root", which), lambda: Ref(SQUARE, ROOT_R, Z6, oracle_field(oracle, shape, flag)))
