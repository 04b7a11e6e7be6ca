"""Host side of the slices of a solid (implisolid_slice_coords, implisolid_slice_loops) and the numpy
restatement tests/np_slice.py on an analytic field, and the inputs of tests/test_gpu_slice_edges.py.
No GPU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_slice   # noqa: E402
import slice_edge_inputs as edges   # noqa: E402
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


# ---- the inputs of tests/test_gpu_slice_edges.py (tests/slice_edge_inputs.py) ---------------------------
# What the GPU tests rely on is asserted here on the references alone, so an edit that spoils an input
# fails without a GPU.


@pytest.mark.parametrize("grid, zeros, hist", [
    ("r32", 72, [246, 31, 32, 30, 19, 173, 23, 41, 28, 33, 166, 41, 33, 38, 43, 47]),
    ("r33", 79, [279, 34, 33, 35, 19, 174, 26, 46, 29, 34, 168, 43, 35, 39, 46, 49])])
def test_injected_field_holds_every_case_a_full_tile_and_negative_zeros(grid, zeros, hist):
    ref, vals = edges.injected_ref(grid), edges.injected_values()
    R = ref.R
    assert np.array_equal(_u32(np.diff(ref.xs)), _u32(np.full(R, 0.0625))) and np.array_equal(_u32(ref.xs), _u32(ref.ys))
    for l, k in edges.INJ_ALIGNED.items():
        # every sample is a table entry, negated: the test dictates the field bit for bit
        assert np.array_equal(_u32(ref.F[l]), _u32(-vals[k][:R + 1, :R + 1])), l
        h = ref.histogram(l)
        print(grid, "layer", l, "cases", h.tolist(), "segments", int(ref.offs[l + 1] - ref.offs[l]))
        assert (h >= 10).all() and h[5] >= 100 and h[10] >= 100
        tiles = ref.tile_counts(l)
        assert tiles.max() == 512 and tiles[0, 0] == 512 and tiles.sum() == ref.offs[l + 1] - ref.offs[l]
        zero = ref.F[l] == 0
        assert zero.sum() >= 60 and np.signbit(ref.F[l][zero]).all(), "an sdf_3d zero is a -0.0 sample"
    # the plane z = 0, as counted when the table was designed
    assert ref.histogram(1).tolist() == hist and ref.offs[2] - ref.offs[1] == (edges.N_SEG * hist).sum()
    assert (ref.F[1] == 0).sum() == zeros
    assert np.array_equal(_u32(ref.F[1]), _u32(ref.F[4])), "the repeated plane"
    assert np_slice.loops(ref.keys[ref.offs[1]:ref.offs[2]]) is not None
    assert not np.isnan(ref.seg).any()
    if grid == "r33":   # one-cell tiles at the border hold segments too; the corner tile is quiet
        assert ref.tile_counts(1)[0, 2] > 0 and ref.tile_counts(1)[2, 0] > 0 and ref.tile_counts(1)[2, 2] == 0


def test_injected_field_on_the_unaligned_grid():
    ref = edges.injected_ref("r40")
    assert not np.isnan(ref.seg).any() and (np.diff(ref.offs) > 500).all()
    for l in range(len(edges.INJ_Z)):
        assert (ref.histogram(l) >= 10).all()
        assert np_slice.loops(ref.keys[ref.offs[l]:ref.offs[l + 1]]) is not None
    # general fractions: most endpoints lie strictly inside their edge
    on_x_edge = ref.keys[:, 0] % 2 == 0
    assert len(np.unique(ref.seg[on_x_edge, 0, 0])) > 200


@pytest.mark.parametrize("name", edges.UNEQUAL_NAMES)
def test_unequal_axes_have_no_coordinate_in_common(oracle, name):
    ref = edges.unequal_ref(oracle, name)
    assert (ref.xs != ref.ys).all() and ref.xs[1] - ref.xs[0] != ref.ys[1] - ref.ys[0]
    print(name, "segments per layer", np.diff(ref.offs).tolist())
    assert (np.diff(ref.offs) > 0).sum() >= 3


def test_the_far_egg_has_segments(oracle):
    ref = edges.far_ref(oracle)
    print("segments per layer", np.diff(ref.offs).tolist(), "equal neighbours in xs", int((np.diff(ref.xs) == 0).sum()),
          "in ys", int((np.diff(ref.ys) == 0).sum()))
    assert (np.diff(ref.offs) > 0).sum() >= 3 and not np.isnan(ref.seg).any()
    assert (np.diff(ref.xs) >= 0).all() and (np.diff(ref.ys) >= 0).all()


@pytest.mark.parametrize("R", edges.SMALL_RS)
def test_every_small_resolution_has_a_segment(oracle, R):
    ref = edges.small_ref(oracle, R)
    print("R", R, "segments per layer", np.diff(ref.offs).tolist())
    assert (np.diff(ref.offs) > 0).all()
    if R == 1:   # only the (xmax, ymax) corner c2 is inside the egg on z = 0.1875
        assert np_slice.cases(ref.F[0]).tolist() == [[4]]


@pytest.mark.parametrize("name, items, lead, trail", [("egg", 8400, 100, 100), ("tree_deep", 4400, 50, 50)])
def test_long_item_lists_span_scan_tiles(oracle, name, items, lead, trail):
    ref = edges.long_ref(oracle, name)
    per = np.diff(ref.offs)
    tpl = ((ref.R + 15) // 16) ** 2
    assert tpl == 4 and len(per) * tpl == items and items > 4096 and items % 4096 != 0
    print(name, "segments", int(ref.offs[-1]), "empty layers in front", int(np.argmax(per > 0)), "behind", int(np.argmax(per[::-1] > 0)))
    # zero counts lead and trail; the first two scan tiles of 4096 items (1024 layers) hold segments, so
    # every later tile's offset is a non-zero sum of tile sums (the egg's third tile holds only zeros)
    assert (per[:lead] == 0).all() and (per[-trail:] == 0).all()
    assert per[:1024].sum() > 0 and per[1024:2048].sum() > 0


def test_lid_planes_are_exact_zeros(oracle):
    lid, bare = edges.lid_ref(oracle, False), edges.lid_ref(oracle, True)
    print("lid: segments per layer", np.diff(lid.offs).tolist(), "zero samples", [(f == 0).sum() for f in lid.F])
    assert sum((f == 0).sum() for f in lid.F) >= 100 and lid.offs[-1] > 0 and not np.isnan(lid.seg).any()
    # an endpoint on a zero sample sits on a grid node
    assert np.isin(lid.seg[..., 0], lid.xs).all() and np.isin(lid.seg[..., 1], lid.ys).all()
    for l in range(3):
        assert np_slice.loops(lid.keys[lid.offs[l]:lid.offs[l + 1]]) is not None
    assert (bare.F[0] == 0).all() and (bare.F[2] == 0).all() and bare.offs[1] == 0 and bare.offs[3] == bare.offs[2]
    assert (np_slice.cases(bare.F[0]) == 15).all() and (np_slice.cases(bare.F[2]) == 15).all()


def test_ignored_root_matrix_is_the_identity(oracle):
    eye, moved, ignored = (edges.root_ref(oracle, w) for w in ("eye", "moved", "ignored"))
    assert np.array_equal(_u32(eye.F), _u32(ignored.F)) and len(eye.seg) > 0
    assert eye.seg.shape != moved.seg.shape or not np.array_equal(_u32(eye.seg), _u32(moved.seg))
