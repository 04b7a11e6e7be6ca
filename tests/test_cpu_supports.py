"""Host side of the support-tip query (implisolid_layer_supports' argument checks in their order, supports_decode),
the restatement tests/np_supports.py against hand-written expectations, and the preconditions of the cases of
test_gpu_supports.py, computed from the restatement alone.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_distance   # noqa: E402
import np_supports   # noqa: E402
import support_inputs as si   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = si.ii.EYE
UNIT = [-1, 1, -1, 1]
NONE = np_supports.NONE

_BITS = {}
_REST = {}


def stack(name):
    """(bits, dist) of a stack of support_inputs, computed once; sized stacks are named (W, H)"""
    if name not in _BITS:
        if isinstance(name, tuple):
            bits = si.sized(*name)
        else:
            bits = (si.TIES.get(name) or si.FEET.get(name) or si.EXISTING[name])()
        _BITS[name] = (bits, np_distance.field(bits))
    return _BITS[name]


def restated(name, reach2, cell):
    """(bits, tips, tip_offsets, records, U) of a stack, computed once per reach and cell"""
    key = (name, reach2, cell)
    if key not in _REST:
        bits, dist = stack(name)
        _REST[key] = (bits,) + np_supports.supports(bits.astype(np.uint8), 1, reach2, cell, dist)
    return _REST[key]


# ---- the restatement by hand ---------------------------------------------------------------------------------
def test_a_square_over_nothing_by_hand():
    cov = np.zeros((3, 5, 6), np.uint8)
    cov[0, 4, 5] = 1
    cov[2, 1:4, 1:4] = 1
    tips, offs, recs, U = np_supports.supports(cov, 1, 0, 16384)
    # one cell: the square's middle (2, 2) at squared distance 4 from the nearest empty pixel; nothing under it
    assert tips.tolist() == [[2 * 6 + 2, 4, -1, 9]] and offs.tolist() == [0, 0, 0, 1] and recs.tolist() == [[0, 0], [0, 0], [9, 1]]
    assert U.sum() == 9 and U[2, 1:4, 1:4].all()
    tips, offs, recs, U = np_supports.supports(cov, 1, 0, 2)
    # cells of 2 x 2, three a row: the square meets cells 0, 1, 3, 4; the rim pixels tie at 1 and the smallest p wins
    assert offs.tolist() == [0, 0, 0, 4] and recs[2].tolist() == [9, 4]
    assert tips.tolist() == [[7, 1, -1, 1], [8, 1, -1, 2], [13, 1, -1, 2], [14, 4, -1, 4]]


def test_feet_by_hand():
    cov = np.zeros((5, 1, 4), np.uint8)
    cov[0, 0, 0] = cov[1, 0, 0] = 1     # column 0: solid in 0 and 1, empty in 2 and 3
    cov[2, 0, 1] = 1                    # column 1: solid in 2, empty in 3
    cov[0, 0, 3] = cov[1, 0, 3] = cov[2, 0, 3] = cov[3, 0, 3] = 1   # column 3 is solid up to 3: supported in 4
    cov[4, 0, :] = 1
    tips, offs, recs, U = np_supports.supports(cov, 1, 0, 1)
    assert offs.tolist() == [0, 0, 0, 1, 1, 4] and recs[4].tolist() == [3, 3]
    assert tips[0].tolist() == [1, 1, -1, 1], "layer 2's pixel over nothing"
    assert tips[1:].tolist() == [[0, NONE, 1, 1], [1, NONE, 2, 1], [2, NONE, -1, 1]], "an all-solid layer: depth NONE"
    assert (tips[:, 2] <= np.repeat(np.arange(5), np.diff(offs)) - 2).all()


def test_reach_makes_near_pixels_supported():
    cov = np.zeros((2, 1, 8), np.uint8)
    cov[0, 0, 0:3] = 1
    cov[1, 0, 0:7] = 1   # overhangs by 4: the empty pixels 3 .. 6 of layer 0 lie at squared distances 1, 4, 9, 16
    assert [np_supports.supports(cov, 1, r2, 16384)[2][1, 0] for r2 in (0, 1, 4, 9, 16)] == [4, 3, 2, 1, 0]
    tips = np_supports.supports(cov, 1, 4, 16384)[0]
    assert tips.tolist() == [[5, 4, -1, 2]], "pixels 5 and 6 are left; 5 lies deeper (squared distance 4 to pixel 7)"


def test_a_threshold_above_one():
    cov = np.zeros((2, 2, 2), np.uint8)
    cov[0] = 2
    cov[1] = 3
    assert len(np_supports.supports(cov, 2, 0, 1)[0]) == 0
    tips, offs, recs, U = np_supports.supports(cov, 3, 0, 1)
    assert tips[:, 0].tolist() == [0, 1, 2, 3] and (tips[:, 2] == -1).all(), "a coverage of 2 below is neither support nor foot"


# ---- supports_decode ---------------------------------------------------------------------------------------------
def test_supports_decode(impli):
    tips = np.zeros(4, impli.SUPPORT_DTYPE)
    tips["p"] = [0, 41, 7, 79]
    l, py, px = impli.supports_decode(tips, [0, 0, 2, 2, 4], 40)
    assert l.tolist() == [1, 1, 3, 3] and py.tolist() == [0, 1, 0, 1] and px.tolist() == [0, 1, 7, 39] and l.dtype == np.int64
    l, py, px = impli.supports_decode(np_supports.as_rows(tips), [0, 4], 8)
    assert l.tolist() == [0] * 4 and py.tolist() == [0, 5, 0, 9] and px.tolist() == [0, 1, 7, 7]
    l, py, px = impli.supports_decode(tips[:0], [0, 0], 8)
    assert len(l) == len(py) == len(px) == 0
    for offs in ([0, 3], [1, 4], [0, 3, 2, 4], []):
        with pytest.raises(ValueError):
            impli.supports_decode(tips, offs, 40)
    with pytest.raises(ValueError):
        impli.supports_decode(tips, [0, 4], 0)


# ---- the ABI -----------------------------------------------------------------------------------------------------
def test_abi_declares_the_support_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name, res in (("implisolid_layer_supports", "int64_t"), ("implisolid_layer_supports_copy", "int"),
                      ("implisolid_debug_layer_supports_ms", "int")):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("%s %s(" % (res, name)) in header, name
    for word in ("cell", "tip_offsets", "foot", "load", "depth", "IMPLISOLID_SUPPORTS_CHUNK", "12 bytes per cell"):
        assert word in header, word
    assert impli.SUPPORT_DTYPE.names == np_supports.FIELDS and impli.SUPPORT_DTYPE.itemsize == 16
    assert impli.SUPPORT_REC_DTYPE.names == np_supports.REC_FIELDS and impli.SUPPORT_REC_DTYPE.itemsize == 16


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
WHO = "implisolid_layer_supports: "
# in the order of the checks: each entry's message wins over every later entry's
ORDER = [
    ("null shape", dict(shape=None), WHO + "bad arguments"),
    ("0 layers", dict(n=0), WHO + "n_layers must be in [1, 65536]"),
    ("nan z", dict(z=[0.0, np.nan]), WHO + "every z must be finite"),
    ("height 16385", dict(H=16385), WHO + "width and height must be in [1, 16384]"),
    ("supersample 3", dict(s=3), WHO + "supersample must be 1, 2 or 4"),
    ("threshold 5", dict(threshold=5), WHO + "threshold must be in [1, supersample^2]"),
    ("reach2 -1", dict(reach2=-1), WHO + "reach2 must be in [0, 2^30)"),
    ("cell 0", dict(cell=0), WHO + "cell must be in [1, 16384]"),
    ("no offsets", dict(offs=None), WHO + "tip_offsets and layer_rec are required"),
    ("reversed rect", dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    ("truncated shape", dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
]
ALONE = [
    (dict(rect=None), WHO + "bad arguments"),
    (dict(z=None), WHO + "bad arguments"),
    (dict(n=65537), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[np.inf, 0.0]), WHO + "every z must be finite"),
    (dict(W=0), WHO + "width and height must be in [1, 16384]"),
    (dict(s=0), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0), WHO + "threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), WHO + "threshold must be in [1, supersample^2]"),
    (dict(reach2=1 << 30), WHO + "reach2 must be in [0, 2^30)"),
    (dict(cell=-1), WHO + "cell must be in [1, 16384]"),
    (dict(cell=16385), WHO + "cell must be in [1, 16384]"),
    (dict(rec=None), WHO + "tip_offsets and layer_rec are required"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = None if "z" in kw and kw["z"] is None else np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = None if "rect" in kw and kw["rect"] is None else np.array(kw.get("rect", UNIT), np.float32)
    offs = np.full(max(n, 2) + 1, 77, np.int64)
    rec = np.full(2 * max(n, 2), 77, np.int64)
    stats = np.full(8, 77, np.int64)
    rc = L.implisolid_layer_supports(kw.get("shape", SPHERE), 0, None if rect is None else rect.ctypes.data_as(fp), kw.get("W", 8),
                                     kw.get("H", 8), kw.get("s", 2), None if z is None else z.ctypes.data_as(fp), n, kw.get("threshold", 1),
                                     kw.get("reach2", 0), kw.get("cell", 4), None if "offs" in kw else offs.ctypes.data_as(lp),
                                     None if "rec" in kw else rec.ctypes.data_as(lp), stats.ctypes.data_as(lp))
    assert (offs == 77).all() and (rec == 77).all() and (stats == 77).all(), "a refused call writes nothing"
    return rc


@pytest.mark.parametrize("kw, message", [(kw, m) for _, kw, m in ORDER] + ALONE)
def test_bad_input_is_refused_before_a_device(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    tips = np.full(4, 77, np.int32)
    assert L.implisolid_layer_supports_copy(tips.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1 and (tips == 77).all()
    assert impli.last_error().startswith("implisolid_layer_supports_copy: no tips to copy")
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("first", range(len(ORDER) - 1))
def test_the_refusals_come_in_order(impli, first):
    L = impli.lib()
    name, kw, message = ORDER[first]
    for later, kw2, _ in ORDER[first + 1:]:
        both = dict(kw2)
        both.update(kw)
        if set(kw) & set(kw2):
            continue   # both mistakes in one argument: one of them cannot be made
        assert _call(L, both) == -1 and impli.last_error() == message, (name, later)


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(reach2=-1), dict(reach2=1 << 30), dict(reach2=1 << 70),
                                dict(cell=0), dict(cell=16385), dict(cell=-3), dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1], cell=4)
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_supports(**a)
    assert str(e.value)


def test_the_timer_answers_without_a_call(impli):
    assert len(impli.layer_supports_kernel_ms(False)) == 4


# ---- the preconditions of the GPU cases ----------------------------------------------------------------------------
def test_the_sized_stacks_have_tips_in_partial_and_whole_cells():
    assert si.CELLS == [1, 3, 16, 17, 64, 16384] and si.SIZES == [1, 15, 16, 17, 63, 64, 65]
    with_tips = 0
    for W in si.SIZES:
        for H in si.SIZES:
            bits, dist = stack((W, H))
            assert bits.shape == (3, H, W)
            U = np_supports.unsupported(dist, 0)
            assert not U[0].any()
            if W * H >= 15:
                assert U[1].any() and U[2].any(), (W, H)
                with_tips += 1
                # an unsupported pixel in the last, partial cell of a row or column wherever there is one
                for cell in (3, 16, 17, 64) if min(W, H) >= 15 else ():
                    if W % cell and W > cell:
                        assert U[:, :, W - W % cell:].any(), (W, H, cell)
                    if H % cell and H > cell:
                        assert U[:, H - H % cell:, :].any(), (W, H, cell)
    assert with_tips == 48
    # one cell for the whole image and a cell that is a pixel, on the largest size
    bits, tips, offs, recs, U = restated((65, 65), 0, 16384)
    assert recs[:, 1].tolist() == [0, 1, 1]
    bits, tips1, offs1, recs1, U = restated((65, 65), 0, 1)
    assert recs1[:, 1].tolist() == recs1[:, 0].tolist() == U.sum(axis=(1, 2)).tolist() and (tips1[:, 3] == 1).all()
    assert np.array_equal(np.flatnonzero(U[1].reshape(-1)), tips1[offs1[1]:offs1[2], 0])
    # a cell side that is no multiple of 4 puts cell edges inside a lane's four pixels: such cells hold tips
    bits, tips17, offs17, recs17, U = restated((65, 65), 0, 17)
    assert len(tips17) == 2 * 16, "every one of the 4 x 4 cells of both layers"


def test_the_tie_cases_really_tie():
    bits, dist = stack("island_start")
    x, y = si.ISLAND_AT
    inner = dist[1, y:y + 4, x:x + 4]
    assert inner.max() == 4 and (inner == 4).sum() == 4 and (dist[0] == -NONE).all()
    bits, tips, offs, recs, U = restated("island_start", 0, 16384)
    assert tips.tolist() == [[(y + 1) * 24 + x + 1, 4, -1, 16]], "the smallest p of the four"
    bits, tips3, offs3, recs3, U = restated("island_start", 0, 3)
    # the island lies over cells of 3 x 3 from (9, 9): x 10 .. 13 -> cells 3, 4; y 9 .. 12 -> cells 3, 4
    assert len(tips3) == 4 and tips3[:, 3].tolist() == [6, 6, 2, 2] and tips3[0].tolist() == [(y + 1) * 24 + x + 1, 4, -1, 6]
    assert tips3[1, 1] == 4 and tips3[2, 1] == 1 and tips3[3, 1] == 1

    for cell in si.TIE_CELLS:
        bits, tips, offs, recs, U = restated("solid_over_empty", 5, cell)
        ncx, ncy = -(-33 // cell), -(-17 // cell)
        assert len(tips) == ncx * ncy and (tips[:, 1] == NONE).all() and (tips[:, 2] == -1).all() and tips[:, 3].sum() == 33 * 17
        want = [cy * cell * 33 + cx * cell for cy in range(ncy) for cx in range(ncx)]
        assert tips[:, 0].tolist() == want, "each cell's first pixel"
        assert len(restated("solid_over_solid", 0, cell)[1]) == 0 and restated("solid_over_solid", 0, cell)[3].tolist() == [[0, 0]] * 2
        assert len(restated("plate_only", 0, cell)[1]) == 0 and stack("plate_only")[0].any()


def test_the_foot_cases_hold_every_kind_of_foot():
    for name in sorted(si.FEET):
        bits, tips, offs, recs, U = restated(name, 0, 1)
        layer = np.repeat(np.arange(len(bits)), np.diff(offs))
        feet = tips[:, 2]
        assert (feet >= 0).any() and (feet == -1).any() and (feet <= layer - 2).all(), name
        assert (feet == 0).any(), "a voxel of layer 0 is a foot"
        assert ((feet >= 0) & (feet == layer - 2)).any(), "a foot right under the empty layer"
        assert (layer - feet >= 5)[feet >= 0].any(), "a foot several layers down"
        # with a layer per chunk every foot lies two chunks back at least, some of them five
        assert sorted(si.FOOT_CHUNKS.values()) == [1, 4]
        back4 = layer[feet >= 0] // 4 - feet[feet >= 0] // 4
        assert (back4 == 0).any() and (back4 == 1).any(), "four layers a chunk: a foot in the tip's own chunk and one in the chunk before"
        for cell in si.FOOT_CELLS:
            assert len(restated(name, 0, cell)[1]) > 0
    bits, tips, offs, recs, U = restated("shelf", 0, 1)
    l, py, px = np.repeat(np.arange(12), np.diff(offs)), tips[:, 0] // 40, tips[:, 0] % 40
    over_slab = (l == si.SHELF) & (py >= 5) & (py < 20) & (px >= 5) & (px < 20)
    beside = (l == si.SHELF) & (py >= 5) & (py < 20) & (px >= 20) & (px < 36)
    over_patch = over_slab & (py >= 8) & (py < 12) & (px >= 8) & (px < 13)
    assert over_slab.sum() == 225 and (tips[over_slab & ~over_patch, 2] == si.SLAB_TOP).all() and beside.sum() == 15 * 16 and (tips[beside, 2] == -1).all()
    assert over_patch.sum() == 20 and (tips[over_patch, 2] == si.PATCH).all(), "the patch is the higher foot"
    pillar = (l == si.SHELF) & (py == si.PILLAR_AT[1]) & (px == si.PILLAR_AT[0])
    assert pillar.sum() == 1 and tips[pillar, 2].tolist() == [0]
    assert (tips[l == si.PATCH, 2] == si.SLAB_TOP).all() and (l == si.PATCH).sum() == 20
    assert recs[si.SHELF + 1].tolist() == [0, 0], "the repeated shelf is supported"
    # the reordered planes: a repeated plane is supported by its twin, and plane 0 after plane 4 hangs in the air
    assert len(si.SHELF_ORDER) > len(set(si.SHELF_ORDER)) and si.SHELF_ORDER != sorted(si.SHELF_ORDER)
    recs = restated("shelf_reordered", 0, 1)[3]
    assert recs[3].tolist() == [0, 0] and recs[5].tolist() == [0, 0] and recs[4, 0] > 0 and recs[8, 0] > 0


@pytest.mark.parametrize("name", sorted(si.EXISTING))
def test_the_existing_stacks_have_tips(name):
    for reach2 in si.EXISTING_REACH2:
        for cell in si.EXISTING_CELLS:
            bits, tips, offs, recs, U = restated(name, reach2, cell)
            # "has tips": every case but the dense stack at reach 2, where every pixel has a solid one within reach below
            assert len(tips) > 0 or (name, reach2) == ("random_95", 4), (name, reach2, cell)
            assert recs[0].tolist() == [0, 0] and tips[:, 3].sum() == U.sum() == recs[:, 0].sum(), (name, reach2, cell)
            assert (np.diff(offs) == recs[:, 1]).all()
    # the reach decides something
    assert restated(name, 0, 1)[3][:, 0].sum() > restated(name, 4, 1)[3][:, 0].sum()
