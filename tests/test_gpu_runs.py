"""Run-length layer images (implisolid_layer_runs) on the GPU.

The reference is tests/np_runs.py's restatement of the definition on coverage images that do not come from
the raster kernels: np_raster.coverage of the oracle's field values (ImplicitService.eval for the sdf_3d shape,
as in test_gpu_raster.py), or the bit pattern itself for the painted stacks of tests/run_inputs.py.
run_offsets, start, value and layer_sum are integers and must equal it exactly, whatever the pruning level
skips or fills, however the layers are chunked, wherever a run crosses a row end or a seam of the walk.  The
decoded runs must also equal raster_layers' image, which reaches the host by another kernel path.  The
preconditions of the cases are asserted without a GPU in test_cpu_runs.py.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import island_inputs as ii   # noqa: E402
import nonfinite_inputs as nf   # noqa: E402
import np_raster   # noqa: E402
import np_runs   # noqa: E402
import run_inputs as ri   # noqa: E402
import test_cpu_islands as ci   # noqa: E402  (the sphere pair; its tests are not collected from here)
import test_cpu_runs as cr   # noqa: E402  (the cached encodings of the painted stacks)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

SHAPES = dict(gm.SHAPES, pair=ci.PAIR)
PLANES = {name: gr.Z for name in gm.NAMES}
PLANES["pair"] = ci.PAIR_Z
RECTS = gr.RECTS
GRIDS = gr.GRIDS


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_runs(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, cov, threshold):
    """against the restatement of cov; returns the decoded images"""
    offs, start, value, sums, stats = got
    L, H, W = cov.shape
    ro, rs, rv = np_runs.encode(cov, threshold)
    assert offs.dtype == np.int64 and start.dtype == np.uint32 and value.dtype == np.uint8 and sums.dtype == np.int64
    assert np.array_equal(offs, ro), (offs.tolist(), ro.tolist())
    assert start.shape == rs.shape and value.shape == rv.shape
    bad = np.flatnonzero((start != rs) | (value != rv))
    assert len(bad) == 0, ("first differing runs", bad[:5].tolist(), start[bad[:5]].tolist(), rs[bad[:5]].tolist(), len(bad))
    assert np.array_equal(sums, cov.reshape(L, -1).sum(axis=1, dtype=np.int64)), sums.tolist()
    assert stats[5] == len(rs) == offs[-1] and stats[6] == int((rv != 0).sum()) == int((value != 0).sum())
    n = impli.run_lengths(offs, start, W * H)
    assert (n >= 1).all() and np.add.reduceat(n, offs[:-1]).tolist() == [W * H] * L
    if threshold == 0:
        assert np.array_equal(np.add.reduceat(value.astype(np.int64) * n, offs[:-1]), sums)
    img = impli.runs_decode(offs, start, value, W, H)
    assert np.array_equal(img, np_runs.values(cov, threshold))
    return img


# ---- the shapes ------------------------------------------------------------------------------------------------
# the sphere pair's planes are chosen for the unit rect
SHAPE_RECTS = [(name, rect) for name in sorted(SHAPES) for rect in sorted(RECTS) if name != "pair" or rect == "unit"]


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("name, rect", SHAPE_RECTS)
def test_runs_equal_the_restatement_and_the_raster_image(impli, oracle, name, rect, W, H, s, level):
    z = PLANES[name]
    cov = gr._ref(impli, oracle, name, SHAPES[name], RECTS[rect], W, H, s, z)[0]
    image, isums, istats = gr._at_level(impli, level, SHAPES[name], RECTS[rect], W, H, z, s)
    for threshold in sorted({0, 1, s * s}):
        got = _run(impli, level, SHAPES[name], RECTS[rect], W, H, z, s, threshold)
        print(name, (W, H, s), rect, level, threshold, "per layer", np.diff(got[0]).tolist(), "stats", got[4])
        img = _check(impli, got, cov, threshold)
        assert np.array_equal(img, np_runs.values(image, threshold)), "the decoded runs are raster_layers' image"
        assert np.array_equal(got[3], isums) and got[4][:5] == istats
        assert got[4][4] == 1 and got[4][5] > len(z), "the case holds a layer of more than one run"
        if level == 0:
            assert got[4][1] == got[4][0] and got[4][2] == 0
        if threshold == 0 and s > 1:
            assert 1 < int(got[2].max()) <= s * s, "grey values beyond 0 / 1"
    if name != "pair":
        # the repeated plane (entries 1 and 3) repeats its runs
        o, st, va = got[0], got[1], got[2]
        assert np.array_equal(st[o[1]:o[2]], st[o[3]:o[4]]) and np.array_equal(va[o[1]:o[2]], va[o[3]:o[4]])


# ---- the painted stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", sorted(ri.PAINTED))
def test_painted_stacks_equal_the_restatement(impli, name, level):
    bits, ro, rs, rv = cr.encoded(name)
    node, rect, z = ii.painted(bits)
    L, H, W = bits.shape
    for threshold in (0, 1):
        got = _run(impli, level, node, rect, W, H, z, 1, threshold)
        print(name, level, threshold, "per layer", np.diff(got[0]).tolist()[:12], "stats", got[4])
        assert np.array_equal(got[0], ro) and np.array_equal(got[1], rs) and np.array_equal(got[2], rv)
        assert np.array_equal(_check(impli, got, bits.astype(np.uint8), threshold), bits)
    if name == "checkerboard":
        assert got[0].tolist() == [0, W * H] and np.array_equal(got[1], np.arange(W * H)), "every pixel a start"
    if name == "tall_thin":
        assert got[4][4] == 1 and L * H > 4096, "one chunk of more rows than a tile of the scan"


@pytest.mark.parametrize("W", ri.SIZES)
def test_step_edges(impli, W):
    for H in ri.SIZES:
        bits = ri.sized(W, H)
        node, rect, z = ii.painted(bits)
        got = _run(impli, 2, node, rect, W, H, z, 1, 1)
        assert np.array_equal(_check(impli, got, bits.astype(np.uint8), 1), bits), (W, H)


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_a_solid_stack_is_one_run_a_layer_without_a_sample(impli, W, H, s):
    z = gr.Z
    for threshold in (0, s * s):
        offs, start, value, sums, stats = _run(impli, 2, gm.BIG, RECTS["unit"], W, H, z, s, threshold)
        assert offs.tolist() == list(range(len(z) + 1)) and (start == 0).all() and (value == (s * s if threshold == 0 else 1)).all()
        assert sums.tolist() == [W * H * s * s] * len(z)
        assert stats[1] == 0 and stats[3] == 0 and stats[2] == stats[0] and stats[5:] == [len(z), len(z)]


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_an_empty_stack_is_one_run_of_zero_a_layer(impli, W, H, s):
    for threshold in (0, 1):
        offs, start, value, sums, stats = _run(impli, 2, gm.AWAY, RECTS["unit"], W, H, gr.Z, s, threshold)
        assert offs.tolist() == list(range(len(gr.Z) + 1)) and (start == 0).all() and (value == 0).all() and (sums == 0).all()
        assert stats[1:4] == [0, 0, 0] and stats[5:] == [len(gr.Z), 0]


# ---- chunks ----------------------------------------------------------------------------------------------------------
def test_three_and_twelve_chunks_give_the_same_runs(impli, monkeypatch):
    bits, ro, rs, rv = cr.encoded("chunked")
    node, rect, z = ii.painted(bits)
    one = _run(impli, 2, node, rect, 40, 40, z, 1, 1)
    monkeypatch.setenv("IMPLISOLID_RUNS_CHUNK", "36")   # four layers of nine raster tiles
    three = _run(impli, 2, node, rect, 40, 40, z, 1, 1)
    monkeypatch.setenv("IMPLISOLID_RUNS_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 0, node, rect, 40, 40, z, 1, 1)
    monkeypatch.delenv("IMPLISOLID_RUNS_CHUNK")
    assert one[4][4] == 1 and three[4][4] == 3 and each[4][4] == 12
    for r in (one, three, each):
        _check(impli, r, bits.astype(np.uint8), 1)
        assert all(np.array_equal(x, y) for x, y in zip(r[:4], one[:4])) and r[4][5:] == one[4][5:]


def test_chunks_of_a_shape_give_the_same_runs(impli, oracle, monkeypatch):
    cov = gr._ref(impli, oracle, "tree_deep", SHAPES["tree_deep"], RECTS["non_dyadic"], 40, 40, 2, gr.Z12)[0]
    monkeypatch.setenv("IMPLISOLID_RUNS_CHUNK", "36")
    got = _run(impli, 2, SHAPES["tree_deep"], RECTS["non_dyadic"], 40, 40, gr.Z12, 2, 0)
    monkeypatch.delenv("IMPLISOLID_RUNS_CHUNK")
    assert got[4][4] == 3
    _check(impli, got, cov, 0)


# ---- rows of five steps: the comb ------------------------------------------------------------------------------------
# 1030 x 3: four full steps of the walk and one of six pixels, run starts in every step of the middle row and a
# tooth across every seam (test_cpu_runs.py asserts it on the reference image)
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("s", [1, 2])
def test_the_comb_equals_the_restatement_and_the_raster_image(impli, oracle, s, level):
    W, H, z = ri.COMB_W, ri.COMB_H, ri.COMB_Z
    cov = gr._ref(impli, oracle, "comb", ri.COMB, ri.COMB_RECT, W, H, s, z)[0]
    assert np.array_equal(cov, cr.comb_image(oracle, s))
    image, isums, istats = gr._at_level(impli, level, ri.COMB, ri.COMB_RECT, W, H, z, s)
    for threshold in sorted({0, 1, s * s}):
        got = _run(impli, level, ri.COMB, ri.COMB_RECT, W, H, z, s, threshold)
        print("comb", s, level, threshold, "per layer", np.diff(got[0]).tolist(), "stats", got[4])
        img = _check(impli, got, cov, threshold)
        assert np.array_equal(img, np_runs.values(image, threshold)), "the decoded runs are raster_layers' image"
        assert np.array_equal(got[3], isums) and got[4][:5] == istats and got[4][4] == 1
        if threshold == 0 and s > 1:
            assert 1 < int(got[2].max()) <= s * s, "grey values beyond 0 / 1"


def test_comb_chunks_give_the_same_runs(impli, oracle, monkeypatch):
    W, H, z = ri.COMB_W, ri.COMB_H, ri.COMB_Z
    cov = gr._ref(impli, oracle, "comb", ri.COMB, ri.COMB_RECT, W, H, 2, z)[0]
    monkeypatch.setenv("IMPLISOLID_RUNS_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 2, ri.COMB, ri.COMB_RECT, W, H, z, 2, 0)
    monkeypatch.delenv("IMPLISOLID_RUNS_CHUNK")
    assert each[4][4] == len(z) == 2
    _check(impli, each, cov, 0)


# ---- the call sequence -----------------------------------------------------------------------------------------------
def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, 4, 0)
    first = impli.layer_runs(*a, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch or the slot
    bits = ii.checkerboard()
    node, rect, z = ii.painted(bits)
    assert impli.layer_runs(node, rect, 129, 129, z, 1, 1, return_stats=True)[4][5] == 129 * 129
    again = impli.layer_runs(*a, return_stats=True)
    assert all(np.array_equal(x, y) for x, y in zip(first[:4], again[:4])) and first[4] == again[4] and len(first[1]) > len(gr.Z)


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    moved = dict(SHAPES["csg"], matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    ignored = gr._ref(impli, oracle, "csg_ignored", moved, RECTS["unit"], 40, 40, 2, gr.Z, True)[0]
    kept = gr._ref(impli, oracle, "csg_moved", moved, RECTS["unit"], 40, 40, 2, gr.Z)[0]
    plain = gr._ref(impli, oracle, "csg", SHAPES["csg"], RECTS["unit"], 40, 40, 2, gr.Z)[0]
    assert np.array_equal(ignored, plain) and not np.array_equal(kept, plain), "the root matrix moves the solid"
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 0, ignore_root_matrix=True), ignored, 0)
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 0), kept, 0)


def test_the_kernel_timer_reports_every_pass(impli):
    impli.layer_runs_kernel_ms(True)
    try:
        impli.layer_runs(SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, 2, 0)
        ms = impli.layer_runs_kernel_ms(True)
    finally:
        impli.layer_runs_kernel_ms(False)
    print("raster, count + scan, emit ms", ms)
    assert len(ms) == 3 and all(0 < v < 1000 for v in ms)


def test_a_failed_call_empties_the_slot(impli):
    a = (SHAPES["egg"], RECTS["unit"], 40, 40, gr.Z, 2)
    assert len(impli.layer_runs(*a, 0)[1]) > len(gr.Z)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_runs(*a, 5)
    assert "threshold" in str(e.value)
    st, va = np.zeros(8, np.uint32), np.zeros(8, np.uint8)
    assert impli.lib().implisolid_layer_runs_copy(st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                  va.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == -1
    assert impli.last_error() == cr.NO_COPY
    assert len(impli.layer_runs(*a, 0)[1]) > len(gr.Z), "and the next call works"


# ---- NaN and infinite samples ----------------------------------------------------------------------------------------
def test_non_finite_samples_in_one_chunk_and_in_several(impli, oracle, monkeypatch):
    name = nf.MIXED[0]
    W, H, s = nf.GRIDS[0]
    cov = np_raster.coverage(nf.raster_field(oracle, name, W, H, s), s)[0]
    assert 0 < int(cov.astype(np.int64).sum()) < cov.size * s * s
    for threshold in (0, s * s):
        one = _run(impli, 2, nf.TREES[name], nf.RECT, W, H, nf.Z, s, threshold)
        monkeypatch.setenv("IMPLISOLID_RUNS_CHUNK", "18")   # two layers of nine raster tiles
        several = _run(impli, 0, nf.TREES[name], nf.RECT, W, H, nf.Z, s, threshold)
        monkeypatch.delenv("IMPLISOLID_RUNS_CHUNK")
        assert one[4][4] == 1 and several[4][4] == 4
        _check(impli, one, cov, threshold)
        _check(impli, several, cov, threshold)
