"""Host side of the suction-cup query (implisolid_layer_cups' argument checks, implisolid_layer_cups_copy, cups_decode,
cup_areas), the restatement tests/np_cups.py on hand-made stacks, and the preconditions of the cases of
test_gpu_cups.py, so that none of them is vacuous.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_inputs as bi   # noqa: E402
import cup_inputs as cu   # noqa: E402
import island_inputs as ii   # noqa: E402
import np_bodies   # noqa: E402
import np_cups   # noqa: E402
import test_cpu_bodies as cb   # noqa: E402  (the sizing rule of the stack-wide arrays; its tests are not collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = ii.EYE
UNIT = [-1, 1, -1, 1]

_REST = {}


def restated(name, connectivity):
    """(bits, cup_offsets, records, run_offsets, runs, decode, empty row runs) of a painted stack, computed once"""
    key = (name, connectivity)
    if key not in _REST:
        bits = cu.PAINTED[name]()
        _REST[key] = (bits,) + np_cups.cups(bits.astype(np.uint8), 1, connectivity)
    return _REST[key]


def per_layer(name, connectivity):
    return np.diff(restated(name, connectivity)[1]).tolist()


# ---- the restatement --------------------------------------------------------------------------------------------
def test_the_restatement_on_a_hand_made_stack():
    # 5 x 5, two layers: a ring around the centre pixel in layer 0; in layer 1 the ring lacks (2, 1), so the centre drains
    ring = np.zeros((5, 5), bool)
    ring[1:4, 1:4] = True
    ring[2, 2] = False
    open_ = ring.copy()
    open_[2, 1] = False
    offs, rec, roffs, runs, dec, n = np_cups.cups(np.stack([ring, open_]).astype(np.uint8), 1, 6)
    assert offs.tolist() == [0, 1, 1] and rec.tolist() == [[12, 1, 2, 2, 2, 2, 12]]
    assert roffs.tolist() == [0, 1, 1] and runs.tolist() == [[12, 1, 0]] and dec[0, 2, 2] == 0 and (dec >= 0).sum() == 1
    assert n == (1 + 2 + 3 + 2 + 1) + (1 + 2 + 2 + 2 + 1), "the empty row runs of both layers"
    # the other order: the pocket is open from the first layer on, and stays so
    offs, rec, roffs, runs, dec, n = np_cups.cups(np.stack([open_, ring]).astype(np.uint8), 1, 6)
    assert offs.tolist() == [0, 0, 0] and len(rec) == 0 and len(runs) == 0, "the order given is the print order"
    # two rings side by side that share one pocket through a tunnel in layer 0: one record in layer 1, two regions
    b = np.ones((2, 5, 9), bool)
    b[0, 2, 2:7] = False
    b[1, 2, 2] = b[1, 2, 6] = False
    offs, rec, roffs, runs, dec, n = np_cups.cups(b.astype(np.uint8), 1, 6)
    assert rec.tolist() == [[20, 5, 2, 2, 6, 2, 20], [20, 2, 2, 2, 6, 2, 20]] and runs.tolist() == [[20, 5, 0], [20, 1, 1], [24, 1, 1]]
    assert offs.tolist() == [0, 1, 2] and roffs.tolist() == [0, 1, 3]


def test_every_painted_stack_fits_the_table_limits():
    for name, make in cu.PAINTED.items():
        bits = make()
        node, rect, z = ii.painted(bits)
        assert len(z) == bits.shape[0] and bits.size <= 70 * 70 * 12, name


# ---- the painted stacks are what they say --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cu.PAINTED))
def test_every_non_trivial_case_has_a_cup(name):
    counts = [sum(per_layer(name, conn)) for conn in (6, 26)]
    if name in cu.TRIVIAL:
        assert counts == [0, 0], name
    else:
        assert max(counts) > 0, name
    for conn in (6, 26):
        bits, offs, rec, roffs, runs, dec, n = restated(name, conn)
        assert rec[:, 1].sum() == runs[:, 1].sum() == (dec >= 0).sum() and not (dec >= 0)[bits].any()
        assert len(runs) <= n and all((np.diff(rec[offs[l]:offs[l + 1], 0]) > 0).all() for l in range(len(offs) - 1))


def test_the_glass_mouth_up_is_a_cup_at_every_layer_past_its_floor_and_no_enclosed_void():
    for conn in (6, 26):
        bits, offs, rec, roffs, runs, dec, n = restated("glass_up", conn)
        assert per_layer("glass_up", conn) == [0] + [1] * 7
        assert (rec[:, 1] == 144).all() and (rec[:, 6] == 1 * 440 + 4 * 22 + 5).all() and (rec[:, 0] == 4 * 22 + 5).all()
        r = np_bodies.bodies(bits.astype(np.uint8), 1, 0, conn)[1]
        L, H, W = bits.shape
        voids = r[(r[:, 2] > 0) & (r[:, 3] > 0) & (r[:, 4] > 0) & (r[:, 5] < W - 1) & (r[:, 6] < H - 1) & (r[:, 7] < L - 1)]
        assert len(voids) == 0, "layer_bodies' enclosed_voids has nothing to say about it"


def test_the_dome_is_cupped_only_on_the_plate():
    for conn in (6, 26):
        assert per_layer("glass_down", conn) == [1] * 5 + [0] * 3, "the plate is closed"
        assert (restated("glass_down", conn)[2][:, 6] == 4 * 22 + 5).all(), "the pocket begins in layer 0"
        assert per_layer("glass_down_raised", conn) == [0] * 9, "an empty first plane opens everything that touches it"
        assert per_layer("glass_side", conn) == [0] * 7


def test_the_vent_ends_the_cup_at_its_layer():
    v = cu.VENT_LAYER
    for conn in (6, 26):
        assert per_layer("vented", conn) == [0] + [1] * (v - 1) + [0] * (8 - v)
        assert per_layer("glass_up", conn)[v] == 1, "without the hole layer v is still cupped"
        # the outer space is unaffected: the only empty voxels outside a cup are the same in both stacks but for the hole
        d_v, d_g = restated("vented", conn)[5], restated("glass_up", conn)[5]
        assert np.array_equal(d_v[:v] >= 0, d_g[:v] >= 0)


def test_the_u_bend_is_one_record_a_layer_over_two_regions():
    for conn in (6, 26):
        bits, offs, rec, roffs, runs, dec, n = restated("u_bend", conn)
        assert per_layer("u_bend", conn) == [0] + [1] * 6
        assert rec[2:, 1].tolist() == [12] * 4 and rec[2:, [2, 3, 4, 5]].tolist() == [[6, 9, 23, 11]] * 4, "the box spans both arms"
        assert not (dec[3, 9:12, 8:22] >= 0).any() and (dec[3, 9:12, 6:8] == 2).all() and (dec[3, 9:12, 22:24] == 2).all()
        assert len(set(rec[:, 6].tolist())) == 1


def test_the_two_pockets_merge_at_the_tunnel():
    m = cu.MERGE_LAYER
    for conn in (6, 26):
        bits, offs, rec, roffs, runs, dec, n = restated("merge", conn)
        H, W = bits.shape[1:]
        A, B = (1 * H + 5) * W + 5, (2 * H + 5) * W + 14
        assert per_layer("merge", conn) == [0, 1, 2, 2, 2, 1, 1, 1]
        assert all(rec[offs[l]:offs[l + 1], 6].tolist() == [A, B] for l in range(2, m)), "two keys before the tunnel"
        assert all(rec[offs[l]:offs[l + 1], 6].tolist() == [A] for l in range(m, 8)), "the smaller one from the tunnel on"
        assert rec[offs[m + 1], 1] == 18 and rec[offs[m + 1], [2, 4]].tolist() == [5, 16]
        assert per_layer("merge_open", conn) == [0, 1, 2, 1, 1, 0, 0, 0], "B opens in layer 3, and takes A with it at the tunnel"


def test_the_sealed_void_is_cupped_over_its_own_layers_only():
    for conn in (6, 26):
        assert per_layer("sealed", conn) == [0, 0, 1, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("side", cu.SIDES)
def test_one_frame_pixel_opens_a_pocket(side):
    bits = cu.frame_only(side)
    L, H, W = bits.shape
    out = ~bits[3] & np_cups.frame(H, W)
    assert out.sum() == 1, "a single frame pixel is empty"
    y, x = [int(v[0]) for v in np.nonzero(out)]
    assert {"x0": x == 0, "x1": x == W - 1, "y0": y == 0, "y1": y == H - 1}[side] and 0 < (x if side[0] == "y" else y) < (W if side[0] == "y" else H) - 1
    for conn in (6, 26):
        bits, offs, rec, roffs, runs, dec, n = restated("frame_only_" + side, conn)
        assert np.diff(offs).tolist() == [2, 2, 2, 1, 1], "one void drains through the pixel; the other's channel stops short and stays closed"
        assert bits[:3][:, np_cups.frame(H, W)].all() and len(set(rec[:, 6].tolist())) == 2


def test_the_diagonal_gap_leaks_under_26_only():
    assert per_layer("diagonal", 6) == [0] + [1] * 7 and per_layer("diagonal", 26) == [0, 1, 1, 1, 0, 0, 0, 0]


def test_rows_of_more_than_64_runs_hold_cups():
    for name, rows_h in (("dense_rows", 3), ("dense_rows_framed", 5), ("rounds_framed", 4)):
        bits, offs, rec, roffs, runs, dec, n = restated(name, 6)
        W = bits.shape[2]
        per_row = np.bincount(runs[roffs[0]:roffs[1], 0] // W, minlength=rows_h)
        assert per_row.max() >= 64, (name, per_row.tolist())
    assert per_layer("dense_rows", 6) == [64] * 3 and per_layer("dense_rows", 26) == [0] * 3
    assert per_layer("rounds_framed", 6)[0] == 150 and per_layer("arch_inverted", 6) == [2, 2, 2, 2, 1]
    r = restated("arch_inverted", 6)[2]
    assert r[-1].tolist() == [20 * 70 + 2, 66, 2, 20, 67, 20, 20 * 70 + 2], "the bridge joins the shafts: a run across the 64-pixel seam"


def test_long_rows_hold_a_pocket_up_to_the_last_columns():
    for W in (256, 257):
        for conn in (6, 26):
            bits, offs, rec, roffs, runs, dec, n = restated("long_%d" % W, conn)
            assert (dec[:, 3, 200:W - 1] >= 0).all() and not (dec[:, 5] >= 0).any(), "one pixel short of the frame is closed, the frame is not"
            assert rec[0].tolist() == [3 * W + 200, W - 201, 200, 3, W - 2, 3, 3 * W + 200] and np.diff(offs)[2] > 40


def test_the_growing_stack_outgrows_its_arrays_chunk_by_chunk():
    bits, offs, rec, roffs, runs, dec, n = restated("growing", 6)
    L = bits.shape[0]
    counts = [int((~bits[l] & np.pad(bits[l], ((0, 0), (1, 0)), constant_values=True)[:, :-1]).sum()) for l in range(L)]   # the starts of empty runs
    assert sum(counts) == n and all(b > a for a, b in zip(counts, counts[1:])), "the empty run count rises from layer to layer"
    # cup_layers' sizing, a layer per chunk: entries 0 .. total + cc and one to spare; entry 0 is the outside
    for item in (8, 4):
        size, total, moved = 0, 0, 0
        for cc in counts:
            want = (total + cc + 2) * item
            if not (size and want <= size):
                moved += total > 0
                size = cb.pool_class(max(want, size + size // 2, 256))
            total += cc
        assert moved >= 3, "the arrays move at least three times with earlier chunks' entries in them"
    assert np.diff(offs).min() >= 4 and len(set(rec[:, 6].tolist())) > 50


def test_sizes_one_and_two_have_only_frame_voxels():
    for W, H in ((1, 17), (2, 2), (65, 2), (1, 1)):
        offs, rec, roffs, runs, dec, n = np_cups.cups(bi.sized(W, H, 3).astype(np.uint8), 1, 6)
        assert len(rec) == 0 and len(runs) == 0
    assert len(np_cups.cups(bi.sized(17, 15, 3).astype(np.uint8), 1, 6)[1]) > 0


# ---- the host helpers ------------------------------------------------------------------------------------------------
def test_cups_decode_and_cup_areas_on_hand_made_records(impli):
    # two layers of 3 rows x 5 columns
    roffs = np.array([0, 2, 3], np.int64)
    rows = np.array([[6, 2, 0], [8, 1, 1], [6, 3, 2]], np.int32)
    runs = np.ascontiguousarray(rows).view(impli.CUP_RUN_DTYPE).reshape(-1)
    want = np.full((2, 3, 5), -1, np.int32)
    want[0, 1, 1:3] = 0
    want[0, 1, 3] = 1
    want[1, 1, 1:4] = 2
    for given in (runs, rows):
        got = impli.cups_decode(roffs, given, 5, 3)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (impli.cups_decode([0, 0, 0], np.zeros((0, 3), np.int32), 5, 3) == -1).all()
    for bad_offs, bad_rows in (([0, 2], rows), ([0, 3, 2], rows), ([0, 2, 3], [[6, 2, 0], [8, 3, 1], [6, 3, 2]]), ([0, 2, 3], [[6, 0, 0], [8, 1, 1], [6, 3, 2]])):
        with pytest.raises(ValueError) as e:
            impli.cups_decode(bad_offs, np.array(bad_rows, np.int32), 5, 3)
        assert str(e.value).startswith("cups_decode: ")
    with pytest.raises(ValueError) as e:
        impli.bodies_decode([0, 2], rows, 5, 3)
    assert str(e.value).startswith("bodies_decode: "), "the shared body keeps each caller's name"
    offs = np.array([0, 2, 2, 3], np.int64)
    recs = np.array([[6, 2, 1, 1, 2, 1, 6], [8, 1, 3, 1, 3, 1, 8], [6, 3, 1, 1, 3, 1, 6]], np.int64)
    cups = np.ascontiguousarray(recs).view(impli.CUP_DTYPE).reshape(-1)
    for given in (cups, recs):
        a = impli.cup_areas(offs, given)
        assert a.dtype == np.int64 and a.tolist() == [3, 0, 3]
    assert impli.cup_areas([0, 0], np.zeros((0, 7), np.int64)).tolist() == [0]
    for bad in ([0, 2], [0, 3, 2, 3], [1, 2, 3]):
        with pytest.raises(ValueError):
            impli.cup_areas(bad, recs)


def test_the_helpers_invert_the_restatement(impli):
    for name, conn in (("u_bend", 6), ("chunked", 6), ("dense_rows_framed", 6), ("merge", 26)):
        bits, offs, rec, roffs, runs, dec, n = restated(name, conn)
        assert np.array_equal(impli.cups_decode(roffs, runs, bits.shape[2], bits.shape[1]), dec), name
        assert np.array_equal(impli.cup_areas(offs, rec), (dec >= 0).sum(axis=(1, 2))), name


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declares_the_cup_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name, decl in (("implisolid_layer_cups", "int64_t implisolid_layer_cups("),
                       ("implisolid_layer_cups_copy", "int implisolid_layer_cups_copy(int64_t* cups, int32_t* runs)"),
                       ("implisolid_debug_layer_cups_ms", "int implisolid_debug_layer_cups_ms(int enable, double ms[4])")):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and decl in header, name
    for word in ("connectivity", "want_runs", "cup_offsets", "run_offsets", "pocket", "IMPLISOLID_CUPS_CHUNK", "2^31 cups"):
        assert word in header, word
    assert impli.CUP_DTYPE.names == np_cups.FIELDS and impli.CUP_DTYPE.itemsize == 56
    assert impli.CUP_RUN_DTYPE.names == np_cups.RUN_FIELDS and impli.CUP_RUN_DTYPE.itemsize == 12


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
ip = ctypes.POINTER(ctypes.c_int32)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
NO_COPY = "implisolid_layer_cups_copy: no cups to copy (the last implisolid_layer_cups failed, or none ran)"
WHO = "implisolid_layer_cups: "
REFUSALS = [
    (dict(n=0), WHO + "n_layers must be in [1, 65536]"),
    (dict(n=65537), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[0.0, np.nan]), WHO + "every z must be finite"),
    (dict(W=0), WHO + "width and height must be in [1, 16384]"),
    (dict(H=16385), WHO + "width and height must be in [1, 16384]"),
    (dict(s=3), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0), WHO + "threshold must be in [1, supersample^2]"),
    (dict(threshold=5), WHO + "threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), WHO + "threshold must be in [1, supersample^2]"),
    (dict(connectivity=8), WHO + "connectivity must be 6 or 26"),
    (dict(connectivity=18), WHO + "connectivity must be 6 or 26"),
    (dict(want_runs=2), WHO + "want_runs must be 0 or 1"),
    (dict(want_runs=-1), WHO + "want_runs must be 0 or 1"),
    (dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
    (dict(shape=None), WHO + "bad arguments"),
    (dict(offsets=None), WHO + "bad arguments"),
    (dict(want_runs=1, run_offsets=None), WHO + "bad arguments"),   # run_offsets may be NULL iff want_runs == 0
    # the documented order: implisolid_layer_bodies' without target, then the rect, and the shape last
    (dict(n=0, z=[np.nan, 0.0], W=0), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[np.nan, 0.0], W=0, s=3), WHO + "every z must be finite"),
    (dict(W=0, s=3, threshold=0), WHO + "width and height must be in [1, 16384]"),
    (dict(s=3, threshold=0, connectivity=4), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0, connectivity=4, want_runs=2), WHO + "threshold must be in [1, supersample^2]"),
    (dict(connectivity=4, want_runs=2, rect=[1, -1, -1, 1]), WHO + "connectivity must be 6 or 26"),
    (dict(want_runs=2, rect=[1, -1, -1, 1], shape=b"{"), WHO + "want_runs must be 0 or 1"),
    (dict(rect=[1, -1, -1, 1], shape=b"{"), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b"{", offsets=None), WHO + "bad arguments"),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = np.array(kw.get("rect", UNIT), np.float32)
    offs, roffs = np.zeros(max(n, 2) + 1, np.int64), np.zeros(max(n, 2) + 1, np.int64)
    return L.implisolid_layer_cups(kw.get("shape", SPHERE), 0, rect.ctypes.data_as(fp), kw.get("W", 8), kw.get("H", 8), kw.get("s", 2),
                                   z.ctypes.data_as(fp), n, kw.get("threshold", 1), kw.get("connectivity", 6), kw.get("want_runs", 0),
                                   None if "offsets" in kw else offs.ctypes.data_as(lp),
                                   None if "run_offsets" in kw else roffs.ctypes.data_as(lp), None)


def _copy_refuses(impli):
    L = impli.lib()
    cups, runs = np.zeros(7, np.int64), np.zeros(3, np.int32)
    assert L.implisolid_layer_cups_copy(cups.ctypes.data_as(lp), runs.ctypes.data_as(ip)) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_layer_cups_copy(cups.ctypes.data_as(lp), None) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_layer_cups_copy(None, None) == -1 and impli.last_error() == NO_COPY


def test_copy_refuses_with_an_empty_slot(impli):
    # whatever ran before in this process, a refused call leaves the slot empty
    assert _call(impli.lib(), dict(n=0)) == -1
    _copy_refuses(impli)


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_bad_input_is_refused_before_a_device_and_empties_the_slot(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    _copy_refuses(impli)
    # the same refusal straight after a refused call
    assert _call(L, kw) == -1 and impli.last_error() == message
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(connectivity=8), dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_cups(**a)
    assert str(e.value)
    with pytest.raises(ValueError):
        impli.layer_cups(json.loads(SPHERE), [0, 1, 2], 8, 8, [0.0])


def test_the_timer_answers_without_a_call(impli):
    assert len(impli.layer_cups_kernel_ms(False)) == 4
