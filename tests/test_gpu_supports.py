"""Support tips under the layer stack (implisolid_layer_supports) on the GPU.

The reference is tests/np_supports.py's restatement of the definition, with loops over cells, on the brute-force
distance field of tests/np_distance.py and on images that do not come from the raster kernels: np_raster.coverage of
the oracle's field values (as in test_gpu_raster.py), or the bit pattern itself for the painted stacks of
tests/support_inputs.py.  Tips, offsets, layer records and totals are integers and must equal it exactly, whatever
the pruning level skips or fills, however the layers are chunked and wherever the cell edges fall.  The
preconditions of the cases are asserted without a GPU in test_cpu_supports.py.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_distance   # noqa: E402
import np_supports   # noqa: E402
import support_inputs as si   # noqa: E402
import test_cpu_supports as cs   # noqa: E402  (the cached restatements; its tests are not collected from here)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

NONE = np_supports.NONE
SHAPES = gm.SHAPES
RECTS = gr.RECTS


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_supports(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, want):
    """tips, offsets, layer records and totals against the restatement's (tips, offsets, records, ...)"""
    tips, offs, recs, stats = got
    want_tips, want_offs, want_recs = want[:3]
    assert tips.dtype == impli.SUPPORT_DTYPE and recs.dtype == impli.SUPPORT_REC_DTYPE and offs.dtype == np.int64
    assert offs.tolist() == want_offs.tolist()
    rows = np_supports.as_rows(tips)
    bad = np.argwhere((rows != want_tips).any(axis=1))
    assert len(bad) == 0, ("first differing tips", bad[:3, 0].tolist(), rows[bad[:3, 0]].tolist(), want_tips[bad[:3, 0]].tolist(), len(bad))
    assert np_supports.as_rows(recs, np_supports.REC_FIELDS).tolist() == want_recs.tolist()
    assert stats[5:] == [int(want_recs[:, 0].sum()), len(want_tips), int((want_tips[:, 2] == -1).sum())]


def _painted(impli, bits, cell, reach2=0, level=2):
    node, rect, z = si.painted(bits)
    return _run(impli, level, node, rect, bits.shape[2], bits.shape[1], z, cell, 1, 1, reach2)


# ---- sizes and cells ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", si.SIZES)
@pytest.mark.parametrize("W", si.SIZES)
def test_sizes_and_cells(impli, W, H):
    bits = cs.stack((W, H))[0]
    for cell in si.CELLS:
        want = cs.restated((W, H), 0, cell)[1:]
        got = _painted(impli, bits, cell)
        print((W, H), cell, "records", np_supports.as_rows(got[2], np_supports.REC_FIELDS).tolist(), "stats", got[3])
        _check(impli, got, want)


# ---- ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", si.TIE_CELLS)
@pytest.mark.parametrize("name", sorted(si.TIES))
def test_ties_go_to_the_smallest_pixel(impli, name, cell):
    reach2 = 5 if name == "solid_over_empty" else 0
    bits, want_tips, want_offs, want_recs, U = cs.restated(name, reach2, cell)
    got = _painted(impli, bits, cell, reach2)
    _check(impli, got, (want_tips, want_offs, want_recs))
    if name in ("solid_over_solid", "plate_only"):
        assert len(got[0]) == 0 and got[3][5:] == [0, 0, 0]
    if name == "solid_over_empty":
        assert (got[0]["depth"] == NONE).all() and len(got[0]) > 0


# ---- feet ------------------------------------------------------------------------------------------------------------
def _foot_case(name):
    if name == "shelf_reordered":
        return si.painted_reordered()
    bits = si.FEET[name]()
    return (bits,) + si.painted(bits)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("cell", si.FOOT_CELLS)
@pytest.mark.parametrize("name", sorted(si.FEET))
def test_feet_in_one_chunk(impli, name, cell, level):
    bits, node, rect, z = _foot_case(name)
    got = _run(impli, level, node, rect, bits.shape[2], bits.shape[1], z, cell)
    assert got[3][4] == 1
    _check(impli, got, cs.restated(name, 0, cell)[1:])
    feet = got[0]["foot"]
    assert (feet >= 0).any() and (feet == -1).any()


@pytest.mark.parametrize("items", sorted(si.FOOT_CHUNKS))
def test_feet_across_forced_chunks(impli, items, tmp_path):
    # a process of its own with IMPLISOLID_SUPPORTS_CHUNK in its environment from the start
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "supports_worker.py")
    out = str(tmp_path / ("feet_%s.npz" % items))
    env = {k: v for k, v in os.environ.items() if k != "IMPLISOLID_SUPPORTS_CHUNK"}
    p = subprocess.run([sys.executable, worker, out, items], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "the worker for %s items ended with %d:\n%s" % (items, p.returncode, p.stderr[-4000:])
    with np.load(out) as f:
        for name in sorted(si.FEET):
            L = len(cs.stack(name)[0])
            for cell in si.FOOT_CELLS:
                key = "%s_%d_" % (name, cell)
                got = (f[key + "tips"], f[key + "offs"], f[key + "recs"], f[key + "stats"].tolist())
                print(items, name, cell, "tips per layer", np.diff(got[1]).tolist(), "stats", got[3])
                assert got[3][4] == -(-L // si.FOOT_CHUNKS[items]), "the chunks were forced"
                _check(impli, got, cs.restated(name, 0, cell)[1:])


def test_chunks_in_process_give_the_same(impli, monkeypatch):
    bits, node, rect, z = _foot_case("shelf")
    one = _run(impli, 2, node, rect, 40, 40, z, 3, 1, 1, 1)
    results = []
    for items, chunks in (("36", 3), ("27", 4), ("1", 12)):
        monkeypatch.setenv("IMPLISOLID_SUPPORTS_CHUNK", items)
        got = _run(impli, 0 if items == "1" else 2, node, rect, 40, 40, z, 3, 1, 1, 1)
        monkeypatch.delenv("IMPLISOLID_SUPPORTS_CHUNK")
        assert got[3][4] == chunks
        results.append(got)
    _check(impli, one, cs.restated("shelf", 1, 3)[1:])
    for r in results:
        assert np.array_equal(r[0], one[0]) and np.array_equal(r[1], one[1]) and np.array_equal(r[2], one[2]) and r[3][5:] == one[3][5:]


# ---- the existing stacks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach2", si.EXISTING_REACH2)
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", sorted(si.EXISTING))
def test_existing_stacks_equal_the_restatement(impli, name, level, reach2):
    for cell in si.EXISTING_CELLS:
        bits, want_tips, want_offs, want_recs, U = cs.restated(name, reach2, cell)
        got = _painted(impli, bits, cell, reach2, level)
        print(name, level, reach2, cell, "records", np_supports.as_rows(got[2], np_supports.REC_FIELDS).tolist(), "stats", got[3])
        _check(impli, got, (want_tips, want_offs, want_recs))


# ---- cross-checks against the existing entries -------------------------------------------------------------------------
@pytest.mark.parametrize("reach2", [0, 3])
def test_cell_one_is_the_overhang_mask_of_layer_distance(impli, reach2):
    a = (SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z)
    tips, offs, recs, stats = impli.layer_supports(*a, 1, 2, 3, reach2, return_stats=True)
    dist, drec, dstats = impli.layer_distance(*a, 2, 3, reach2, return_stats=True)
    mask = impli.overhang_mask(dist, reach2)
    assert mask.any() and stats[:5] == dstats[:5] and stats[5] == dstats[6]
    assert recs["unsupported"].tolist() == drec["unsupported"].tolist() == recs["tips"].tolist()
    l, py, px = impli.supports_decode(tips, offs, 40)
    listed = np.zeros_like(mask)
    listed[l, py, px] = True
    assert np.array_equal(listed, mask) and len(tips) == mask.sum() and (tips["load"] == 1).all()
    assert np.array_equal(tips["depth"], dist[l, py, px])
    # a coarser grid stands for the same pixels
    coarse, coffs, crecs = impli.layer_supports(*a, 7, 2, 3, reach2)
    assert crecs["unsupported"].tolist() == drec["unsupported"].tolist() and coarse["load"].sum() == mask.sum()
    cl, cy, cx = impli.supports_decode(coarse, coffs, 40)
    assert mask[cl, cy, cx].all() and 0 < len(coarse) < len(tips)


# ---- real shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("s, threshold", [(2, 3), (4, 9)])
def test_a_shape_equals_the_restatement(impli, oracle, s, threshold, level):
    cov = gr._ref(impli, oracle, "csg", SHAPES["csg"], RECTS["non_dyadic"], 40, 40, s, gr.Z12)[0]
    dist = np_distance.field(cov >= threshold)
    for cell in (1, 5, 16):
        want = np_supports.supports(cov, threshold, 2, cell, dist)
        assert len(want[0]) > 0
        got = _run(impli, level, SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z12, cell, s, threshold, 2)
        print("csg", s, threshold, level, cell, "records", np_supports.as_rows(got[2], np_supports.REC_FIELDS).tolist(), "stats", got[3])
        _check(impli, got, want)


def test_a_wide_flat_image(impli, oracle):
    # wider than 4096: many blocks a row, a width that is no multiple of 4, cells across the block edges
    W, H, z = 4099, 3, gr.Z[1:5]
    cov = gr._ref(impli, oracle, "egg", SHAPES["egg"], RECTS["non_dyadic"], W, H, 1, z)[0]
    dist = np_distance.field(cov >= 1)
    for cell in (1, 17, 64):
        want = np_supports.supports(cov, 1, 0, cell, dist)
        assert len(want[0]) > 0
        got = _run(impli, 2, SHAPES["egg"], RECTS["non_dyadic"], W, H, z, cell)
        _check(impli, got, want)


# ---- slot and timer ------------------------------------------------------------------------------------------------------
def test_the_copy_after_a_failed_call_is_refused(impli):
    L = impli.lib()
    bits = cs.stack("island_start")[0]
    tips, offs, recs, stats = _painted(impli, bits, 16384)
    assert len(tips) == 1
    buf = np.full(4, 77, np.int32)
    assert L.implisolid_layer_supports_copy(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0 and buf.tolist() == list(tips[0].tolist())
    with pytest.raises(impli.ImplisolidError):
        impli.layer_supports(SHAPES["csg"], RECTS["unit"], 8, 8, gr.Z, 4, 3)   # supersample 3
    buf[:] = 77
    assert L.implisolid_layer_supports_copy(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1 and (buf == 77).all()
    assert impli.last_error().startswith("implisolid_layer_supports_copy: no tips to copy")
    # a result without tips is a result: the copy takes no pointer
    none = _painted(impli, cs.stack("solid_over_solid")[0], 4)
    assert len(none[0]) == 0 and L.implisolid_layer_supports_copy(None) == 0
    assert L.implisolid_layer_supports_copy(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0 and (buf == 77).all()


def test_the_kernel_timer(impli):
    # one process runs the whole suite: this test is the only one that switches the timer on
    a = (SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, 8, 2, 1, 0)
    before = impli.layer_supports_kernel_ms(False)
    assert before == (-1.0,) * 4, "no timed call yet"
    impli.layer_supports(*a)
    assert impli.layer_supports_kernel_ms(True) == (-1.0,) * 4, "an untimed call leaves the figures"
    try:
        timed = impli.layer_supports(*a, return_stats=True)
        ms = impli.layer_supports_kernel_ms(False)
    finally:
        impli.layer_supports_kernel_ms(False)
    print("raster, columns + rows, cells, count + scan + emit + top ms", ms)
    assert len(ms) == 4 and all(0 <= v < 1000 for v in ms) and ms[0] > 0 and ms[1] > 0
    again = impli.layer_supports(*a, return_stats=True)
    assert impli.layer_supports_kernel_ms(False) == ms, "unchanged by an untimed call"
    assert np.array_equal(timed[0], again[0]) and timed[3] == again[3] and len(timed[0]) > 0


def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, 3, 4, 9, 2)
    first = impli.layer_supports(*a, return_stats=True)
    # another shape, size and cell in between: nothing of it may stay behind in the table or the slot
    assert len(_painted(impli, cs.stack("solid_over_empty")[0], 1)[0]) == 33 * 17
    again = impli.layer_supports(*a, return_stats=True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    assert first[3] == again[3] and len(first[0]) > 0
