"""Host side of the distance field query (implisolid_layer_distance's argument checks, offset_mask,
overhang_mask), the restatement tests/np_distance.py against hand-written expectations, and the preconditions
of the cases of test_gpu_distance.py.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_inputs as di   # noqa: E402
import np_distance   # noqa: E402
import np_islands   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np_distance.NONE
EYE = di.ii.EYE
UNIT = [-1, 1, -1, 1]

_REST = {}


def restated(name):
    """(bits, dist) of a painted stack, computed once"""
    if name not in _REST:
        bits = di.PAINTED[name]()
        _REST[name] = (bits, np_distance.field(bits))
    return _REST[name]


# ---- the restatement by hand ---------------------------------------------------------------------------------
def test_a_single_pixel_has_no_other_class():
    dist, rec = np_distance.distance(np.array([[[1]]], np.uint8), 1, 0)
    assert dist.dtype == np.int32 and dist.tolist() == [[[NONE]]] and rec.tolist() == [[1, NONE, 0, 0]]
    dist, rec = np_distance.distance(np.array([[[0]]], np.uint8), 1, 0)
    assert dist.tolist() == [[[-NONE]]] and rec.tolist() == [[0, 0, -1, 0]]


def test_one_row_of_five():
    dist, rec = np_distance.distance(np.array([[[1, 1, 1, 0, 0]]], np.uint8), 1, 0)
    assert dist.tolist() == [[[9, 4, 1, -1, -4]]] and rec.tolist() == [[3, 9, 0, 0]]
    dist, rec = np_distance.distance(np.array([[[0, 3, 0, 4, 4]]], np.uint8), 3, 0)
    assert dist.tolist() == [[[-1, 1, -1, 1, 4]]] and rec.tolist() == [[3, 4, 4, 0]]
    dist, rec = np_distance.distance(np.array([[[0, 3, 0, 4, 4]]], np.uint8), 4, 0)
    assert dist.tolist() == [[[-9, -4, -1, 1, 4]]] and rec.tolist() == [[2, 4, 4, 0]]
    dist, rec = np_distance.distance(np.array([[[0, 4, 0, 4, 0]]], np.uint8), 4, 0)
    assert dist.tolist() == [[[-1, 1, -1, 1, -1]]] and rec.tolist() == [[2, 1, 1, 0]], "the first of two widest pixels"


def test_three_by_three_with_a_centre_hole():
    bits = np.ones((1, 3, 3), np.uint8)
    bits[0, 1, 1] = 0
    dist, rec = np_distance.distance(bits, 1, 0)
    assert dist[0].tolist() == [[2, 1, 2], [1, -1, 1], [2, 1, 2]] and rec.tolist() == [[8, 2, 0, 0]]


def test_a_column_and_a_diagonal():
    bits = np.zeros((1, 4, 3), np.uint8)
    bits[0, 0, 0] = 1
    dist, _ = np_distance.distance(bits, 1, 0)
    assert dist[0].tolist() == [[1, -1, -4], [-1, -2, -5], [-4, -5, -8], [-9, -10, -13]]


def test_unsupported_by_hand():
    cov = np.array([[[1, 1, 0, 0, 0]], [[1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0]], [[0, 1, 0, 0, 0]]], np.uint8)
    dist = np_distance.field(cov >= 1)
    assert dist[0].tolist() == [[4, 1, -1, -4, -9]] and dist[2].tolist() == [[-NONE] * 5]
    for reach2, want in ((0, 3), (1, 2), (3, 2), (4, 1), (8, 1), (9, 0)):
        rec = np_distance.records(dist, reach2)
        assert rec[:, 3].tolist() == [0, want, 0, 1], reach2   # layer 3 stands on an empty layer at any reach
    assert np_distance.records(dist, NONE - 1)[:, 3].tolist() == [0, 0, 0, 1]


# ---- offset_mask, overhang_mask --------------------------------------------------------------------------------
def test_offset_mask(impli):
    assert impli.DIST_NONE == NONE
    row = np.array([[[9, 4, 1, -1, -4]]], np.int32)
    assert impli.offset_mask(row, 0).tolist() == [[[True, True, True, False, False]]]
    assert impli.offset_mask(row, 1).tolist() == [[[True, True, True, True, False]]]
    assert impli.offset_mask(row, 3).tolist() == [[[True, True, True, True, False]]]
    assert impli.offset_mask(row, 4).all()
    assert impli.offset_mask(row, -1).tolist() == [[[True, True, False, False, False]]]
    assert impli.offset_mask(row, -4).tolist() == [[[True, False, False, False, False]]]
    assert not impli.offset_mask(row, -9).any()
    ring = np.array([[2, 1, 2], [1, -1, 1], [2, 1, 2]], np.int32)
    assert impli.offset_mask(ring, 1).all() and impli.offset_mask(ring, -1).tolist() == [[True, False, True], [False] * 3, [True, False, True]]
    # a layer of one class stays what it is, whatever the radius
    assert not impli.offset_mask(np.full((2, 2), -NONE, np.int32), NONE - 1).any()
    assert impli.offset_mask(np.full((2, 2), NONE, np.int32), -(NONE - 1)).all()


def test_offset_mask_is_dilation_and_erosion_by_the_disc():
    import implisolid_amd as impli
    bits, dist = restated("random_50")
    H, W = bits.shape[1:]
    for r2 in (1, 2, 4, 5):
        r = int(np.sqrt(r2))
        grown = np.zeros_like(bits)
        kept = np.ones_like(bits)
        p = np.pad(bits, ((0, 0), (r, r), (r, r)), constant_values=False)
        q = np.pad(bits, ((0, 0), (r, r), (r, r)), constant_values=True)   # outside the image nothing is empty
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy * dy + dx * dx <= r2:
                    grown |= p[:, r + dy:r + dy + H, r + dx:r + dx + W]
                    kept &= q[:, r + dy:r + dy + H, r + dx:r + dx + W]
        assert np.array_equal(impli.offset_mask(dist, r2), grown), r2
        assert np.array_equal(impli.offset_mask(dist, -r2), kept), r2   # dist > r2: farther than sqrt(r2) from every empty pixel


def test_overhang_mask(impli):
    cov = np.array([[[1, 1, 0, 0, 0]], [[1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0]], [[0, 1, 0, 0, 0]]], np.uint8)
    dist = np_distance.field(cov >= 1)
    assert impli.overhang_mask(dist, 0).tolist() == [[[False] * 5], [[False, False, True, True, True]], [[False] * 5],
                                                    [[False, True, False, False, False]]]
    assert impli.overhang_mask(dist, 4)[1].tolist() == [[False, False, False, False, True]]
    for reach2 in (0, 1, 4, 9):
        assert impli.overhang_mask(dist, reach2).sum(axis=(1, 2)).tolist() == np_distance.records(dist, reach2)[:, 3].tolist()


# ---- the preconditions of the GPU cases -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(di.PAINTED))
def test_every_stack_fits_and_obeys_the_definition(name):
    bits, dist = restated(name)
    di.painted(bits)   # asserts the table limits
    assert dist.dtype == np.int32 and np.array_equal(dist > 0, bits) and (np.abs(dist) >= 1).all() and (np.abs(dist) <= NONE).all()
    for l in range(len(bits)):
        one = bits[l].all() or not bits[l].any()
        assert (np.abs(dist[l]) == NONE).all() if one else (np.abs(dist[l]) < NONE).all()
    # at reach 0 the unsupported pixels are the ones the islands' records do not count as resting
    offs, comps, _ = np_islands.islands(bits.astype(np.uint8), 1, 8)
    rec = np_distance.records(dist, 0)
    for l in range(1, len(bits)):
        c = comps[offs[l]:offs[l + 1]]
        assert rec[l, 3] == int((c[:, 1] - c[:, 2]).sum()), l
    assert rec[:, 0].tolist() == bits.sum(axis=(1, 2)).tolist()


def test_the_hole_s_widest_pixel_is_the_far_corner():
    bits, dist = restated("one_hole")
    rec = np_distance.records(dist, 0)
    assert rec.tolist() == [[4899, 2896, 4830, 0]]
    y, x = np.mgrid[0:70, 0:70]
    want = (x - di.HOLE[0]) ** 2 + (y - di.HOLE[1]) ** 2
    want[di.HOLE[1], di.HOLE[0]] = -1
    assert np.array_equal(dist[0], want)
    assert (dist[0] > 32 * 32).any(), "distances cross whole tiles"


def test_the_single_pixel_and_the_one_class_layers():
    bits, dist = restated("one_pixel")
    y, x = np.mgrid[0:21, 0:37]
    want = -((x - di.DOT[0]) ** 2 + (y - di.DOT[1]) ** 2)
    want[di.DOT[1], di.DOT[0]] = 1
    assert np.array_equal(dist[0], want) and np_distance.records(dist, 0).tolist() == [[1, 1, di.DOT[1] * 37 + di.DOT[0], 0]]
    bits, dist = restated("one_class")
    assert np_distance.records(dist, 4).tolist() == [[561, NONE, 0, 0], [0, 0, -1, 0], [561, NONE, 0, 561]]


def test_the_disc_s_widest_pixel_is_its_centre():
    bits, dist = restated("disc")
    rec = np_distance.records(dist, 0)[0]
    assert rec[2] == 35 * 70 + 35 and rec[1] == 401, "the nearest empty pixels lie at (20, 1) from the centre, not along an axis"


def test_the_stripes_have_their_half_widths():
    bits, dist = restated("stripes")
    assert np.array_equal(dist[1], dist[0].T)
    line = dist[0][0]
    assert (dist[0] == line[None, :]).all()
    at = 0
    for w in range(1, 8):
        half = (w + 1) // 2
        assert line[at:at + w].max() == half * half, w
        if w < 7:   # an empty stripe between two solid ones
            assert line[at + w:at + 2 * w].min() == -half * half, w
        at += 2 * w
    assert line[-1] == -(60 - 49) ** 2, "the last, empty stripe runs to the border: only its solid side counts"


def test_the_random_fills_search_far_on_both_signs():
    assert restated("random_05")[1].min() <= -16 and restated("random_95")[1].max() >= 16
    d = restated("random_50")[1]
    assert d.max() >= 2 and d.min() <= -2


def test_the_staircase_tells_the_reaches_apart():
    bits, dist = restated("staircase")
    rows = [np_distance.records(dist, r2)[:, 3].tolist() for r2 in di.STAIR_REACH2]
    print(rows)
    for i in range(len(rows)):
        for j in range(i):
            assert rows[i] != rows[j], (di.STAIR_REACH2[i], di.STAIR_REACH2[j])
    assert all(rows[0][l] > 0 for l in (4, 8)), "the first layers of the chunks of four overhang"
    assert sorted(set(di.STAIR_STEPS[1:])) == [0, 1, 2, 3] and bits[11].sum() < 35 * 35
    edge = 10 + sum(di.STAIR_STEPS[1:3])   # layer 2 follows a step of 3: its corner pixel is at 3^2 + 3^2
    assert dist[1][edge - 1, edge - 1] == -18 and bits[2][edge - 1, edge - 1]


def test_the_sized_fills_hold_both_classes():
    for W in di.SIZES:
        for H in di.SIZES:
            bits = di.sized(W, H)
            assert bits.any() and not bits.all(), (W, H)


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declares_the_distance_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name in ("implisolid_layer_distance", "implisolid_debug_layer_distance_ms"):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("int %s(" % name) in header, name
    for word in ("reach2", "widest_at", "unsupported", "NONE = 2^30", "IMPLISOLID_DISTANCE_CHUNK"):
        assert word in header, word
    assert impli.DIST_DTYPE.names == np_distance.FIELDS and impli.DIST_DTYPE.itemsize == 32


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
REFUSALS = [
    (dict(threshold=0), "implisolid_layer_distance: threshold must be in [1, supersample^2]"),
    (dict(threshold=5), "implisolid_layer_distance: threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), "implisolid_layer_distance: threshold must be in [1, supersample^2]"),
    (dict(reach2=-1), "implisolid_layer_distance: reach2 must be in [0, 2^30)"),
    (dict(reach2=1 << 30), "implisolid_layer_distance: reach2 must be in [0, 2^30)"),
    (dict(reach2=1 << 40), "implisolid_layer_distance: reach2 must be in [0, 2^30)"),
    (dict(n=0), "implisolid_layer_distance: n_layers must be in [1, 65536]"),
    (dict(n=65537), "implisolid_layer_distance: n_layers must be in [1, 65536]"),
    (dict(z=[0.0, np.nan]), "implisolid_layer_distance: every z must be finite"),
    (dict(W=0), "implisolid_layer_distance: width and height must be in [1, 16384]"),
    (dict(H=16385), "implisolid_layer_distance: width and height must be in [1, 16384]"),
    (dict(s=3), "implisolid_layer_distance: supersample must be 1, 2 or 4"),
    (dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
    (dict(shape=None), "implisolid_layer_distance: bad arguments"),
    (dict(rec=None), "implisolid_layer_distance: bad arguments"),
    # the request is validated before the shape is compiled
    (dict(shape=b"{", reach2=-5), "implisolid_layer_distance: reach2 must be in [0, 2^30)"),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = np.array(kw.get("rect", UNIT), np.float32)
    rec = np.full(4 * max(n, 2), 77, np.int64)
    rc = L.implisolid_layer_distance(kw.get("shape", SPHERE), 0, rect.ctypes.data_as(fp), kw.get("W", 8), kw.get("H", 8), kw.get("s", 2),
                                     z.ctypes.data_as(fp), n, kw.get("threshold", 1), kw.get("reach2", 0), None,
                                     None if "rec" in kw else rec.ctypes.data_as(lp), None)
    assert (rec == 77).all(), "a refused call writes nothing"
    return rc


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_bad_input_is_refused_before_a_device(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(reach2=-1), dict(reach2=1 << 30), dict(reach2=1 << 70),
                                dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_distance(**a)
    assert str(e.value)
    with pytest.raises(ValueError):
        impli.layer_distance(json.loads(SPHERE), [0, 1, 2], 8, 8, [0.0])


def test_the_timer_answers_without_a_call(impli):
    assert len(impli.layer_distance_kernel_ms(False)) == 3
