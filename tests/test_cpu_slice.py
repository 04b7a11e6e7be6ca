"""Host side of the slices of a solid (implisolid_slice_coords, implisolid_slice_loops) and the numpy
restatement tests/np_slice.py on an analytic field.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_slice   # noqa: E402
from implisolid_amd import scenes   # noqa: E402

RECT = [-1, 1, -1, 1]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_declares_the_slice_entries(impli):
    L = impli.lib()
    for name in ("implisolid_slice", "implisolid_slice_copy", "implisolid_slice_coords", "implisolid_slice_loops"):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS, name


def test_coords_equal_the_numpy_formula(impli):
    rect = [-0.7, 1.3, 0.1, 0.9]   # non-dyadic edges: the step and the products round
    xs, ys = impli.slice_coords(rect, 40)
    rx, ry = np_slice.coords(rect, 40)
    assert xs.shape == (41,) and ys.shape == (41,)
    assert np.array_equal(_u32(xs), _u32(rx)) and np.array_equal(_u32(ys), _u32(ry))
    assert xs[40] == np.float32(1.3) and ys[40] == np.float32(0.9) and (np.diff(xs) > 0).all() and (np.diff(ys) > 0).all()


@pytest.mark.parametrize("rect, R", [([1, -1, -1, 1], 8), ([-1, 1, 0, 0], 8), ([-1, np.inf, -1, 1], 8),
                                     ([np.nan, 1, -1, 1], 8), (RECT, 0), (RECT, 4097)])
def test_coords_refuse_bad_input(impli, rect, R):
    with pytest.raises(impli.ImplisolidError):
        impli.slice_coords(rect, R)


def _check_loops(impli, keys, want_order, want_offs, want_closed):
    order, offs, closed = impli.slice_loops(keys)
    ro, rf, rc = np_slice.loops(keys)
    assert order.tolist() == want_order and offs.tolist() == want_offs and closed.tolist() == want_closed
    assert ro.tolist() == want_order and rf.tolist() == want_offs and rc.tolist() == want_closed


def test_loops_two_closed_loops_interleaved(impli):
    # loop A: 10 -> 11 -> 12 -> 10 (segments 0, 2, 4); loop B: 20 -> 21 -> 20 (segments 1, 3)
    keys = [(10, 11), (20, 21), (11, 12), (21, 20), (12, 10)]
    _check_loops(impli, keys, [0, 2, 4, 1, 3], [0, 3, 5], [True, True])


def test_loops_an_open_chain_before_a_loop(impli):
    # the loop's segments come first in index order, the open chain 7 -> 8 -> 9 still leads
    keys = [(30, 31), (8, 9), (31, 30), (7, 8)]
    _check_loops(impli, keys, [3, 1, 0, 2], [0, 2, 4], [False, True])


def test_loops_single_segment_and_empty_input(impli):
    _check_loops(impli, [(4, 5)], [0], [0, 1], [False])
    _check_loops(impli, np.zeros((0, 2), np.uint32), [], [0], [])


def test_loops_refuse_a_duplicate_key(impli):
    with pytest.raises(impli.ImplisolidError):
        impli.slice_loops([(1, 2), (1, 3)])     # key 1 starts two segments
    with pytest.raises(impli.ImplisolidError):
        impli.slice_loops([(1, 3), (2, 3)])     # key 3 ends two
    assert np_slice.loops([(1, 2), (1, 3)]) is None and np_slice.loops([(1, 3), (2, 3)]) is None
    assert impli.slice_loops([(1, 2), (2, 1)])[2].tolist() == [True], "and the next call works"


@pytest.fixture(scope="module")
def sphere_slice(oracle):
    """The oracle's sphere of radius 0.5 on the plane z = 0, R = 64 in +-1, marched in numpy."""
    xs, ys = np_slice.coords(RECT, 64)
    tree = oracle.mp5_to_nodes(json.dumps({"type": "iellipsoid", "matrix": list(scenes.EYE)}))
    F = np.asarray(oracle.eval_implicit(tree, np_slice.points(xs, ys, [0.0])), np.float32).reshape(1, 65, 65)
    seg, keys, offs = np_slice.march(F, xs, ys)
    return dict(xs=xs, ys=ys, F=F, seg=seg, keys=keys, offs=offs)


def test_restatement_closes_the_sphere(impli, sphere_slice):
    seg, keys, offs = sphere_slice["seg"], sphere_slice["keys"], sphere_slice["offs"]
    assert offs.tolist() == [0, len(seg)] and len(seg) > 64
    # every key occurs exactly once as a start and once as an end
    assert len(np.unique(keys[:, 0])) == len(keys) and np.array_equal(np.sort(keys[:, 0]), np.sort(keys[:, 1]))
    order, lo, closed = impli.slice_loops(keys)
    assert lo.tolist() == [0, len(seg)] and closed.tolist() == [True]
    assert np.array_equal(keys[order[1:], 0], keys[order[:-1], 1]) and keys[order[-1], 1] == keys[order[0], 0]
    # chained segments share their endpoints bit for bit: both cells of an edge compute the same point
    assert np.array_equal(_u32(seg[order[1:], 0]), _u32(seg[order[:-1], 1]))
    # counter-clockwise (solid on the left), and the inscribed polygon's area: the chord error is of
    # order (h / r)^2 = (1/32 / 1/2)^2 = 0.4 %, far inside 2 %
    area = np_slice.shoelace(seg[order, 0])
    print("area", area, "pi / 4", np.pi / 4)
    assert area > 0 and abs(area - np.pi / 4) <= 0.02 * np.pi / 4
    ro, rf, rc = np_slice.loops(keys)
    assert np.array_equal(ro, order) and np.array_equal(rf, lo) and np.array_equal(rc, closed)


def test_saddle_cell_gives_two_segments_on_four_keys():
    xs = ys = np.array([0, 1], np.float32)
    for F, case in (([[1, -1], [-1, 1]], 5), ([[-1, 1], [1, -1]], 10)):
        F = np.array(F, np.float32)
        assert int(np_slice.cases(F)[0, 0]) == case
        seg, keys = np_slice.march_layer(F, xs, ys)
        assert seg.shape == (2, 2, 2) and len(np.unique(keys)) == 4
        # the cell's four edges: x-edges 0 and 2 W = 4, y-edges 1 and 2 + 1 = 3
        assert sorted(keys.reshape(-1).tolist()) == [0, 1, 3, 4]
        assert np.allclose(seg, np.float32(0.5) * np.round(2 * seg)), "every endpoint is an edge midpoint"
    # case 5 cuts c0 and c2 off separately: bottom -> left, then top -> right
    seg, keys = np_slice.march_layer(np.array([[1, -1], [-1, 1]], np.float32), xs, ys)
    assert keys.tolist() == [[0, 1], [4, 3]]
    assert seg.tolist() == [[[0.5, 0.0], [0.0, 0.5]], [[0.5, 1.0], [1.0, 0.5]]]
