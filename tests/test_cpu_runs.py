"""Host side of the run-length query (implisolid_layer_runs' argument checks, implisolid_layer_runs_copy,
run_lengths, runs_decode), the restatement tests/np_runs.py against a plain loop over the pixels, and the
preconditions of the cases of test_gpu_runs.py.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import island_inputs as ii   # noqa: E402
import np_raster   # noqa: E402
import np_runs   # noqa: E402
import np_sdf3d   # noqa: E402
import run_inputs as ri   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = ii.EYE
UNIT = [-1, 1, -1, 1]


def loop_encode(v):
    """the definition, pixel by pixel"""
    L, H, W = v.shape
    offs, start, value = [0], [], []
    for l in range(L):
        prev = None
        for py in range(H):
            for px in range(W):
                x = int(v[l, py, px])
                if prev is None or x != prev:
                    start.append(py * W + px)
                    value.append(x)
                prev = x
        offs.append(len(start))
    return np.array(offs, np.int64), np.array(start, np.uint32), np.array(value, np.uint8)


_ENC = {}


def encoded(name):
    """(bits, run_offsets, start, value) of a painted input, computed once"""
    if name not in _ENC:
        bits = ri.PAINTED[name]()
        _ENC[name] = (bits,) + np_runs.encode(bits.astype(np.uint8), 1)
    return _ENC[name]


def comb_image(oracle, s):
    """the comb's reference image uint8 (2, 3, 1030): np_raster.coverage of the oracle's field, through
    test_gpu_raster._ref, which keeps it for the GPU tests"""
    import test_gpu_raster as gr   # its tests are not collected from here
    return gr._ref(None, oracle, "comb", ri.COMB, ri.COMB_RECT, ri.COMB_W, ri.COMB_H, s, ri.COMB_Z)[0]


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---- the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ri.PAINTED))
def test_the_restatement_equals_a_loop_over_the_pixels(impli, name):
    bits, offs, start, value = encoded(name)
    L, H, W = bits.shape
    assert _same((offs, start, value), loop_encode(bits.astype(np.uint8)))
    assert np.array_equal(np_runs.decode(offs, start, value, W, H), bits)
    assert np.array_equal(impli.runs_decode(offs, start, value, W, H), bits.astype(np.uint8))
    n = impli.run_lengths(offs, start, W * H)
    assert n.dtype == np.int64 and np.array_equal(n, np_runs.lengths(offs, start, W * H)) and (n >= 1).all()
    assert np.add.reduceat(n, offs[:-1]).tolist() == [W * H] * L


def test_the_restatement_equals_a_loop_at_the_step_sizes(impli):
    for W in ri.SIZES:
        for H in ri.SIZES:
            bits = ri.sized(W, H)
            got = np_runs.encode(bits.astype(np.uint8), 1)
            assert _same(got, loop_encode(bits.astype(np.uint8))), (W, H)
            assert np.array_equal(impli.runs_decode(*got, W, H), bits), (W, H)
            assert np.add.reduceat(impli.run_lengths(got[0], got[1], W * H), got[0][:-1]).tolist() == [W * H] * 2


def test_grey_and_binary_values():
    cov = np.array([[[0, 1, 1, 4], [4, 3, 0, 0]], [[2, 2, 2, 2], [2, 2, 2, 2]]], np.uint8)
    grey = np_runs.encode(cov, 0)
    assert _same(grey, loop_encode(cov))
    assert grey[0].tolist() == [0, 5, 6] and grey[1].tolist() == [0, 1, 3, 5, 6, 0] and grey[2].tolist() == [0, 1, 4, 3, 0, 2]
    for thr, starts, vals in ((1, [0, 1, 6, 0], [0, 1, 0, 1]), (3, [0, 3, 6, 0], [0, 1, 0, 0]), (4, [0, 3, 5, 0], [0, 1, 0, 0])):
        got = np_runs.encode(cov, thr)
        assert _same(got, loop_encode((cov >= thr).astype(np.uint8)))
        assert got[1].tolist() == starts and got[2].tolist() == vals, thr
    # the 4 4 of the grey stream crosses the row end: one run
    assert np.array_equal(np_runs.decode(*grey, 4, 2), cov)
    n = np_runs.lengths(grey[0], grey[1], 8)
    assert (grey[2].astype(np.int64) * n)[:5].sum() == cov[0].sum()


def test_the_host_helpers_refuse_broken_offsets(impli):
    with pytest.raises(ValueError):
        impli.run_lengths([0, 2, 2], [0, 3], 8)     # a layer without a run
    with pytest.raises(ValueError):
        impli.run_lengths([0, 3], [0, 3], 8)
    with pytest.raises(ValueError):
        impli.runs_decode([0, 2], [1, 3], [0, 1], 4, 2)   # the first start is not 0
    with pytest.raises(ValueError):
        impli.runs_decode([0, 2], [0, 0], [0, 1], 4, 2)   # a run of no pixel


# ---- the painted stacks are what they say ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["row_end_17", "row_end_16", "boundaries", "corners"])
def test_a_painted_stack_is_its_bit_pattern(name):
    bits = ri.PAINTED[name]()
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    mx, my = np_raster.coords(rect, W, H, 1)
    T = np_sdf3d.Table.from_node(node)
    assert np.array_equal(mx, (T.ox + T.gs * np.arange(W, dtype=np.float32)).astype(np.float32)), "the samples are the table's nodes"
    assert np.array_equal(my, (T.oy + T.gs * np.arange(H, dtype=np.float32)).astype(np.float32))
    assert np.array_equal(z, (T.oz + T.gs * np.arange(L, dtype=np.float32)).astype(np.float32))
    F = np_sdf3d.evaluate(node, *np_raster.points(mx, my, z).T).reshape(L, H, W)
    assert np.array_equal(np.abs(F), np.ones_like(F))
    assert np.array_equal(np_raster.coverage(F, 1)[0] == 1, bits)


def test_every_painted_stack_fits_the_table_limits():
    for name, make in ri.PAINTED.items():
        ii.painted(make())
    for W in ri.SIZES:
        for H in ri.SIZES:
            node, rect, z = ii.painted(ri.sized(W, H))
            assert node["size_x"] >= 2 and node["size_y"] >= 2 and len(z) == 2


# ---- the preconditions of the GPU cases ------------------------------------------------------------------------
def test_the_checkerboard_starts_a_run_at_every_pixel():
    bits, offs, start, value = encoded("checkerboard")
    assert offs.tolist() == [0, 129 * 129] and np.array_equal(start, np.arange(129 * 129)) and 129 % 2 == 1, \
        "an odd width: the value alternates across the row ends too"


@pytest.mark.parametrize("W", [17, 16])
def test_the_row_end_stacks_cross_and_break_at_row_ends(W):
    bits, offs, start, value = encoded("row_end_%d" % W)
    b = bits[0]
    assert ((W + 15) // 16 * 16 != W) == (W == 17), "the image pitch is not the width only for 17"
    assert b[0, W - 1] and b[1, 0], "a solid last pixel and a solid first pixel of the next row: one run"
    assert b[1, W - 1] and not b[2, 0] and not b[2, W - 1] and b[3, 0], "solid | empty and empty | solid across a row end"
    assert b[3, W - 1] and b[4, 0]
    s0 = set(start[offs[0]:offs[1]].tolist())
    assert W not in s0 and 4 * W not in s0 and 2 * W in s0 and 3 * W in s0
    # the byte in front of a row's first in the padded image is a padding zero: a walk that reads it sees
    # empty | solid at rows 1 and 4 of layer 0, where the stream has solid | solid
    s1 = set(start[offs[1]:offs[2]].tolist())
    assert W not in s1 and 4 * W not in s1, "the complement: the runs of zeros cross there"
    assert not bits[1, 1, W - 1] and bits[1, 2, 0] and 2 * W in s1, "and a zero | one boundary exactly at px = 0"


def test_the_boundaries_lie_on_the_step_seams():
    bits, offs, start, value = encoded("boundaries")
    W = 300
    s0 = start[offs[0]:offs[1]].tolist()
    assert 64 in s0 and 256 in s0 and 63 not in s0 and 255 not in s0
    assert W in s0 and not bits[0, 0, W - 1], "a boundary exactly at px = 0"
    assert 2 * W + 290 in s0 and 3 * W not in s0 and 3 * W + 5 in s0, "a run across the row end, behind pixel 256 of its row"
    assert all(4 * W + x in s0 for x in range(250, 262)), "a run a pixel across 255 | 256"
    s1 = start[offs[1]:offs[2]].tolist()
    assert s1 == [0] + [x for py in range(5) for x in (py * W + 256, py * W + 257)]
    assert sum(1 for p in s0 if p % W >= 256) > 0 and (W + 15) // 16 * 16 == 304


def test_the_corner_pixels_are_runs_of_one():
    bits, offs, start, value = encoded("corners")
    n = 9 * 37
    assert start.tolist() == [0, 1, n - 1, 0, n - 1, 0, 1] and value.tolist() == [1, 0, 1, 0, 1, 1, 0] and offs.tolist() == [0, 3, 5, 7]


def test_the_tall_stack_has_more_rows_than_a_scan_tile():
    bits, offs, start, value = encoded("tall_thin")
    assert bits.shape[0] * bits.shape[1] > 4096 and len(start) > 4096


# ---- rows of two full steps and more ---------------------------------------------------------------------------------
DENSE = ["dense_511", "dense_512", "dense_512_ends"]


def row_step_starts(offs, start, W, H, l):
    """the run starts of layer l in each 256-pixel step of each row: int (H, steps)"""
    p = start[offs[l]:offs[l + 1]].astype(np.int64)
    out = np.zeros((H, (W + 255) // 256), np.int64)
    np.add.at(out, (p // W, p % W // 256), 1)
    return out


@pytest.mark.parametrize("name", DENSE)
def test_the_dense_rows_start_many_runs_in_both_steps(name):
    bits, offs, start, value = encoded(name)
    L, H, W = bits.shape
    assert (L, H) == (2, 3) and 256 < W <= 512 and W in (511, 512), "two steps of the walk; 512 is the table's limit"
    for l in range(L):
        n = row_step_starts(offs, start, W, H, l)
        print(name, l, "starts per row and step", n.tolist())
        assert n.shape == (H, 2) and n.min() >= 80, "a start in most lanes of both steps of every row"
        for target in (False, True):   # the runs of either class, as the bodies query walks them
            assert all(sum(ri.step_starts(bits[l, py] == target)) > 64 for py in range(H))
        p = start[offs[l]:offs[l + 1]].astype(np.int64)
        second = p[p % W >= 256]
        assert len(set((second % W % 256 // 4).tolist())) >= 48, "in many lanes of the second step"
    if W == 512:
        assert {bool(bits[l, py, 511]) for l in range(L) for py in range(H)} == {False, True}
    if name == "dense_512_ends":
        assert bits[0, :, 511].all() and not bits[1, :, 511].any(), "a last pixel of each value in every row"
        assert sum(ri.step_starts(bits[0, 1])) > 128, "more than 128 runs of the solid class in a row"


def test_the_comb_compiles_within_the_program_s_stacks(impli):
    n_instr, depth = impli.program_info(ri.COMB)[:2]
    n = len(ri.COMB_TEETH)
    # two instructions a tooth and two a Union: 33 CSG nodes, so their two-bit pruning modes reach past the low half
    # of the 64-bit modes word (and the last one past the 32 nodes that are pruned at all)
    assert depth <= 16 and n_instr == 2 * n + 2 * (n - 1) and n - 1 > 32, (n_instr, depth)
    flat = {"type": "Union", "matrix": EYE, "children": [c for group in ri.COMB["children"] for c in group["children"]]}
    assert len(flat["children"]) == len(ri.COMB_TEETH)
    with pytest.raises(impli.ImplisolidError) as e:   # why the teeth are grouped
        impli.program_info(flat)
    assert "too deep" in str(e.value)


def test_the_comb_starts_runs_in_every_step_and_straddles_every_seam(oracle):
    W, H = ri.COMB_W, ri.COMB_H
    assert W == 4 * 256 + 6 and (W + 15) // 16 * 16 != W and 30 <= len(ri.COMB_TEETH) <= 48, "five steps, the last of six pixels; a few dozen teeth"
    for s in (1, 2):
        cov = comb_image(oracle, s)
        assert cov.shape == (2, H, W) and cov.dtype == np.uint8
        for threshold in sorted({0, 1, s * s}):
            offs, start, value = np_runs.encode(cov, threshold)
            n = row_step_starts(offs, start, W, H, 0)
            print("comb", s, threshold, "starts per row and step, plane 0", n.tolist(), "plane 1", row_step_starts(offs, start, W, H, 1).tolist())
            assert n.shape == (H, 5)
            if threshold == s * s and s > 1:
                continue   # full coverage only: the teeth of less than a pixel are gone, and the last step with them
            assert n[1].min() >= 4, "the middle row starts four runs and more in each of the five steps"
            v = np_runs.values(cov, threshold)[0]
            first = set(start[offs[0]:offs[1]].tolist())
            for x in ri.COMB_SEAMS:
                assert v[1, x - 1] == v[1, x] != 0 and v[1, x - 2] == 0 and v[1, x + 1] == 0, "a tooth of two pixels on the seam"
                assert W + x - 1 in first and W + x not in first and W + x + 1 in first, "its run crosses the seam"
                assert (v[0, x - 6:x + 6] == 0).all(), "and a run of zeros crosses it in the row above"
        if s == 2:
            assert 1 < int(cov[cov < 4].max()) and int(cov.max()) == 4, "grey values beyond 0 / 1"
    assert (comb_image(oracle, 1)[1] >= 1).any() and not np.array_equal(comb_image(oracle, 1)[0], comb_image(oracle, 1)[1]), "the planes differ"


# ---- the ABI -------------------------------------------------------------------------------------------------------
def test_abi_declares_the_run_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name, decl in (("implisolid_layer_runs", "int64_t implisolid_layer_runs("),
                       ("implisolid_layer_runs_copy", "int implisolid_layer_runs_copy("),
                       ("implisolid_debug_layer_runs_ms", "int implisolid_debug_layer_runs_ms(")):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and decl in header, name
    for word in ("threshold == 0", "run_offsets", "v[p] != v[p - 1]", "W H - start", "IMPLISOLID_RUNS_CHUNK"):
        assert word in header, word


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
NO_COPY = "implisolid_layer_runs_copy: no runs to copy (the last implisolid_layer_runs failed, or none ran)"
BAD_THRESHOLD = "implisolid_layer_runs: threshold must be 0 (grey) or in [1, supersample^2]"
REFUSALS = [
    (dict(threshold=-1), BAD_THRESHOLD),
    (dict(threshold=5), BAD_THRESHOLD),
    (dict(s=1, threshold=2), BAD_THRESHOLD),
    (dict(s=4, threshold=17), BAD_THRESHOLD),
    (dict(n=0), "implisolid_layer_runs: n_layers must be in [1, 65536]"),
    (dict(n=65537), "implisolid_layer_runs: n_layers must be in [1, 65536]"),
    (dict(z=[0.0, np.nan]), "implisolid_layer_runs: every z must be finite"),
    (dict(W=0), "implisolid_layer_runs: width and height must be in [1, 16384]"),
    (dict(H=16385), "implisolid_layer_runs: width and height must be in [1, 16384]"),
    (dict(s=3), "implisolid_layer_runs: supersample must be 1, 2 or 4"),
    (dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
    (dict(shape=None), "implisolid_layer_runs: bad arguments"),
    (dict(rect=None), "implisolid_layer_runs: bad arguments"),
    (dict(z=None), "implisolid_layer_runs: bad arguments"),
    (dict(offsets=None), "implisolid_layer_runs: bad arguments"),
    (dict(sums=None), "implisolid_layer_runs: bad arguments"),
    # raster's refusals come first, in raster's order, and all of them before the shape is compiled
    (dict(n=0, W=0, s=3, threshold=-1), "implisolid_layer_runs: n_layers must be in [1, 65536]"),
    (dict(z=[np.inf, 0.0], W=0, s=3, threshold=-1), "implisolid_layer_runs: every z must be finite"),
    (dict(W=0, s=3, threshold=-1), "implisolid_layer_runs: width and height must be in [1, 16384]"),
    (dict(s=3, threshold=-1), "implisolid_layer_runs: supersample must be 1, 2 or 4"),
    (dict(threshold=-1, rect=[1, -1, -1, 1]), BAD_THRESHOLD),
    (dict(shape=b"{", threshold=99), BAD_THRESHOLD),
    (dict(shape=b"{", rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = None if "z" in kw and kw["z"] is None else (np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32))
    rect = None if "rect" in kw and kw["rect"] is None else np.array(kw.get("rect", UNIT), np.float32)
    offs = np.zeros(max(n, 2) + 1, np.int64)
    sums = np.zeros(max(n, 2), np.int64)
    return L.implisolid_layer_runs(kw.get("shape", SPHERE), 0, None if rect is None else rect.ctypes.data_as(fp), kw.get("W", 8),
                                   kw.get("H", 8), kw.get("s", 2), None if z is None else z.ctypes.data_as(fp), n,
                                   kw.get("threshold", 0), None if "offsets" in kw else offs.ctypes.data_as(lp),
                                   None if "sums" in kw else sums.ctypes.data_as(lp), None)


def _copy_fails(impli):
    L = impli.lib()
    st, va = np.zeros(8, np.uint32), np.zeros(8, np.uint8)
    up, bp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    assert L.implisolid_layer_runs_copy(st.ctypes.data_as(up), va.ctypes.data_as(bp)) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_layer_runs_copy(None, None) == -1 and impli.last_error() == NO_COPY


def test_copy_before_any_call_fails(impli):
    # no test of this process without a GPU can have filled the slot: every call before it was refused
    _copy_fails(impli)


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_bad_input_is_refused_before_a_device_and_empties_the_slot(impli, kw, message):
    assert _call(impli.lib(), kw) == -1
    assert impli.last_error() == message
    _copy_fails(impli)
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=-1),
                                dict(supersample=2, threshold=5), dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_runs(**a)
    assert str(e.value)
    with pytest.raises(ValueError):
        impli.layer_runs(json.loads(SPHERE), [0, 1, 2], 8, 8, [0.0])


def test_the_timer_answers_without_a_call(impli):
    ms = impli.layer_runs_kernel_ms(False)
    assert len(ms) == 3
