"""Suction cups of the layer stack (implisolid_layer_cups) on the GPU.

The reference is tests/np_cups.py's restatement of the definition on coverage images that do not come from the raster
kernels: the bit pattern itself for the painted stacks of tests/cup_inputs.py, or np_raster.coverage of the oracle's
field values for the shapes (test_gpu_raster._ref).  cup_offsets, the records, run_offsets, the run records and
their decoded stack are integers and must equal it exactly, for both connectivities, whatever the pruning level
skips or fills and however the layers are chunked.  The preconditions of the cases are asserted without a GPU in
test_cpu_cups.py.  The query is checked against code that exists besides: layer_bodies of every prefix of the
stack, and layer_islands of the empty class on single layers.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_inputs as bi   # noqa: E402
import cup_inputs as cu   # noqa: E402
import island_inputs as ii   # noqa: E402
import np_cups   # noqa: E402
import test_cpu_cups as cc   # noqa: E402  (the cached restatements; its tests are not collected from here)
import test_cpu_islands as ci   # noqa: E402  (the sphere pair)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

SHAPES = dict(gm.SHAPES, pair=ci.PAIR)
PLANES = {name: gr.Z for name in gm.NAMES}   # a plane that misses every shape, a repeated plane and an unsorted order
PLANES["pair"] = ci.PAIR_Z
RECTS = gr.RECTS
GRIDS = [(40, 40, 1), (40, 40, 2)]
CONNECTIVITIES = (6, 26)


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_cups(*a, want_runs=True, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, want, W, H):
    offs, cups, roffs, runs, stats = got
    ro, rc, rro, rr, rd, n_empty = want
    assert offs.dtype == np.int64 and roffs.dtype == np.int64 and cups.dtype == impli.CUP_DTYPE and runs.dtype == impli.CUP_RUN_DTYPE
    assert np.array_equal(offs, ro), (offs.tolist(), ro.tolist())
    rows = np_cups.as_rows(cups)
    assert rows.shape == rc.shape, (rows.shape, rc.shape, rows[:4].tolist(), rc[:4].tolist())
    bad = np.argwhere((rows != rc).any(axis=1))
    assert len(bad) == 0, ("first differing cups", rows[bad[:3, 0]].tolist(), rc[bad[:3, 0]].tolist(), len(bad))
    assert np.array_equal(roffs, rro), (roffs.tolist(), rro.tolist())
    rrows = np_cups.as_rows(runs, np_cups.RUN_FIELDS)
    assert rrows.shape == rr.shape
    bad = np.argwhere((rrows != rr).any(axis=1))
    assert len(bad) == 0, ("first differing runs", bad[:3, 0].tolist(), rrows[bad[:3, 0]].tolist(), rr[bad[:3, 0]].tolist(), len(bad))
    dec = impli.cups_decode(roffs, runs, W, H)
    assert dec.dtype == np.int32 and np.array_equal(dec, rd)
    assert stats[5] == n_empty and stats[6] == len(rc) and stats[7] == int((rd >= 0).sum()) == int(rc[:, 1].sum())
    assert np.array_equal(impli.cup_areas(offs, cups), (rd >= 0).sum(axis=(1, 2)))


# ---- the painted stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(cu.PAINTED))
def test_painted_stacks_equal_the_restatement(impli, name, connectivity, level):
    bits, *want = cc.restated(name, connectivity)
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    got = _run(impli, level, node, rect, W, H, z, 1, 1, connectivity)
    print(name, connectivity, level, "cups per layer", np.diff(got[0]).tolist(), "cupped runs", len(got[3]), "stats", got[4])
    _check(impli, got, want, W, H)
    assert got[4][4] == 1
    if level == 0:
        assert got[4][1] == got[4][0] and got[4][2] == 0


def test_the_painted_answers_a_slicer_wants(impli):
    # the default connectivity is 6, the dual of 26 for the solid; a glass printed mouth-up has no enclosed void
    bits = cu.glass_up()
    node, rect, z = ii.painted(bits)
    offs, cups = impli.layer_cups(node, rect, 22, 20, z)
    assert np.array_equal(np_cups.as_rows(cups), cc.restated("glass_up", 6)[2]) and np.diff(offs).tolist() == [0] + [1] * 7
    assert impli.cup_areas(offs, cups).tolist() == [0] + [144] * 7
    assert len(impli.enclosed_voids(impli.layer_bodies(node, rect, 22, 20, z, target=0)[1], 22, 20, 8)) == 0
    node, rect, z = ii.painted(cu.diagonal())
    assert np.diff(impli.layer_cups(node, rect, 22, 20, z)[0]).tolist() == [0] + [1] * 7
    assert np.diff(impli.layer_cups(node, rect, 22, 20, z, connectivity=26)[0]).tolist() == [0, 1, 1, 1, 0, 0, 0, 0]
    node, rect, z = ii.painted(cu.merge())
    offs, cups = impli.layer_cups(node, rect, 24, 14, z)
    assert (cups["pocket"] // (24 * 14)).tolist() == [1, 1, 2, 1, 2, 1, 2, 1, 1, 1], "the layer where each cup's pocket begins"


@pytest.mark.parametrize("H", bi.SIZES)
@pytest.mark.parametrize("W", bi.SIZES)
def test_sizes_around_the_steps_of_the_walk(impli, W, H):
    for L in bi.LAYERS:
        bits = bi.sized(W, H, L)
        node, rect, z = ii.painted(bits)
        for connectivity in CONNECTIVITIES:
            want = np_cups.cups(bits.astype(np.uint8), 1, connectivity)
            got = _run(impli, 2, node, rect, W, H, z, 1, 1, connectivity)
            _check(impli, got, want, W, H)
            if min(W, H) <= 2:
                assert len(got[1]) == 0, "only frame voxels"


# ---- against code that exists besides ---------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", ["merge", "merge_open", "u_bend", "vented", "chunked", "dense_rows_framed"])
def test_every_prefix_is_layer_bodies_of_the_empty_class(impli, name, connectivity):
    bits = cu.PAINTED[name]()
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    offs, cups, roffs, runs = impli.layer_cups(node, rect, W, H, z, 1, 1, connectivity, want_runs=True)
    dec = impli.cups_decode(roffs, runs, W, H)
    seen = 0
    for l in range(L):
        bo, bodies, bruns = impli.layer_bodies(node, rect, W, H, z[:l + 1], 1, 1, 0, connectivity, want_runs=True)
        inner = (bodies["x0"] > 0) & (bodies["y0"] > 0) & (bodies["x1"] < W - 1) & (bodies["y1"] < H - 1)
        top = impli.bodies_decode(bo, bruns, W, H)[l]   # the bodies of the prefix, restricted to layer l
        mine = cups[offs[l]:offs[l + 1]]
        closed = np.where(top >= 0, inner[np.maximum(top, 0)], False)
        assert np.array_equal(dec[l] >= 0, closed), (name, l)
        ids = np.unique(top[closed])   # in seed order, which is not the cups' order within the layer
        assert sorted(bodies["seed"][ids].tolist()) == sorted(mine["pocket"].tolist()), "the body's seed is the pocket"
        for c, rec in enumerate(mine):
            b = int(np.searchsorted(bodies["seed"], rec["pocket"]))
            at = top == b
            assert np.array_equal(dec[l] == offs[l] + c, at) and rec["area"] == at.sum() and rec["seed"] == np.flatnonzero(at)[0]
        seen += len(mine)
    assert seen == len(cups) == len(cc.restated(name, connectivity)[2])
    assert len(cups) > 0 or (name, connectivity) == ("dense_rows_framed", 26), "under 26 the checkerboard's voids all drain"


@pytest.mark.parametrize("name", sorted(ii.PAINTED))
def test_one_layer_is_the_empty_layer_islands_that_miss_the_frame(impli, name):
    stack = ii.PAINTED[name]()
    H, W = stack.shape[1:]
    for l in range(min(2, len(stack))):
        node, rect, z = ii.painted(stack[l:l + 1])
        inv, irect, iz = ii.painted(~stack[l:l + 1])   # the empty class as the solid of another stack
        for conn3, conn2 in ((6, 4), (26, 8)):
            offs, cups = impli.layer_cups(node, rect, W, H, z, 1, 1, conn3)
            io, comps = impli.layer_islands(inv, irect, W, H, iz, 1, 1, conn2)
            keep = comps[(comps["x0"] > 0) & (comps["y0"] > 0) & (comps["x1"] < W - 1) & (comps["y1"] < H - 1)]
            assert offs.tolist() == [0, len(keep)]
            for a, b in (("seed", "seed"), ("area", "area"), ("x0", "x0"), ("y0", "y0"), ("x1", "x1"), ("y1", "y1"), ("pocket", "seed")):
                assert np.array_equal(cups[a], keep[b].astype(np.int64)), (name, l, conn3, a)


# ---- chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name, tiles", [("chunked", 9), ("arch_inverted", 15), ("merge", 2)])
def test_chunks_give_the_same_answer(impli, name, tiles, connectivity, monkeypatch):
    bits, *want = cc.restated(name, connectivity)
    L, H, W = bits.shape
    assert tiles == -(-W // 16) * -(-H // 16)
    node, rect, z = ii.painted(bits)
    one = _run(impli, 2, node, rect, W, H, z, 1, 1, connectivity)
    monkeypatch.setenv("IMPLISOLID_CUPS_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 0, node, rect, W, H, z, 1, 1, connectivity)
    monkeypatch.setenv("IMPLISOLID_CUPS_CHUNK", str(4 * tiles))   # four layers of raster tiles
    four = _run(impli, 2, node, rect, W, H, z, 1, 1, connectivity)
    monkeypatch.delenv("IMPLISOLID_CUPS_CHUNK")
    assert one[4][4] == 1 and each[4][4] == L and four[4][4] == (L + 3) // 4
    for r in (one, each, four):
        _check(impli, r, want, W, H)
        assert all(np.array_equal(x, y) for x, y in zip(r[:4], one[:4])) and r[4][5:] == one[4][5:]


def test_a_fresh_process_grows_its_arrays_chunk_by_chunk(impli, tmp_path):
    # In this process the scratch that earlier tests left holds any test stack, and grow_keeping returns at once.
    # A child's engine starts empty: with a layer per chunk the five run arrays of `growing` take a larger block in
    # most chunks, the earlier chunks' entries copied over (test_cpu_cups.py restates the sizes)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cups_grow_worker.py")
    for connectivity in CONNECTIVITIES:
        bits, *want = cc.restated("growing", connectivity)
        L, H, W = bits.shape
        out = str(tmp_path / ("growing_%d.npz" % connectivity))
        env = {k: v for k, v in os.environ.items() if k != "IMPLISOLID_CUPS_CHUNK"}
        p = subprocess.run([sys.executable, worker, out, str(connectivity)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, "the worker for %d ended with %d:\n%s" % (connectivity, p.returncode, p.stderr[-4000:])
        with np.load(out) as f:
            got = (f["offsets"], f["cups"], f["run_offsets"], f["runs"], f["stats"].tolist())
        print("growing", connectivity, "cups per layer", np.diff(got[0]).tolist(), "stats", got[4])
        _check(impli, got, want, W, H)
        assert got[4][4] == L, "a layer per chunk"


# ---- the shapes ------------------------------------------------------------------------------------------------
SHAPE_RECTS = [(name, rect) for name in sorted(SHAPES) for rect in sorted(RECTS) if name != "pair" or rect == "unit"]
_REF = {}


def _ref(impli, oracle, name, rect, W, H, s, threshold, connectivity):
    key = (name, rect, W, H, s, threshold, connectivity)
    if key not in _REF:
        cov = gr._ref(impli, oracle, name, SHAPES[name], RECTS[rect], W, H, s, PLANES[name])[0]
        _REF[key] = np_cups.cups(cov, threshold, connectivity)
    return _REF[key]


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("name, rect", SHAPE_RECTS)
def test_shapes_equal_the_restatement(impli, oracle, name, rect, W, H, s, level):
    z = PLANES[name]
    for threshold in sorted({1, s * s}):
        for connectivity in CONNECTIVITIES:
            want = _ref(impli, oracle, name, rect, W, H, s, threshold, connectivity)
            got = _run(impli, level, SHAPES[name], RECTS[rect], W, H, z, s, threshold, connectivity)
            print(name, (W, H, s), rect, level, threshold, connectivity, "cups", np_cups.as_rows(got[1]).tolist()[:4], "stats", got[4])
            _check(impli, got, want, W, H)
            assert got[4][4] == 1


# ---- invariants ------------------------------------------------------------------------------------------------------
def _chunked_stack():
    bits = cu.PAINTED["chunked"]()
    return ii.painted(bits) + bits.shape[1:]


def test_areas_runs_and_the_copy_entry(impli):
    lp, ip = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    node, rect, z, H, W = _chunked_stack()
    a = (node, rect, W, H, z, 1, 1, 6)
    offs, cups, roffs, runs, stats = impli.layer_cups(*a, want_runs=True, return_stats=True)
    rstats = impli.raster_layers(node, rect, W, H, z, 1, return_stats=True)[2]
    assert int(cups["area"].sum()) == stats[7] == int(runs["length"].sum()) > 0 and stats[:5] == rstats
    assert stats[6] == len(cups) == offs[-1] and len(runs) == roffs[-1] and stats[5] == impli.layer_bodies(*a[:7], 0, 6, return_stats=True)[2][5]
    # without want_runs the records are the same, and the copy entry takes runs = NULL
    plain = impli.layer_cups(*a)
    assert len(plain) == 2 and np.array_equal(plain[0], offs) and np.array_equal(plain[1], cups)
    out = np.zeros(len(cups), impli.CUP_DTYPE)
    assert impli.lib().implisolid_layer_cups_copy(out.ctypes.data_as(lp), None) == 0 and np.array_equal(out, cups)
    # a call that asked for runs needs the pointer
    impli.layer_cups(*a, want_runs=True)
    assert impli.lib().implisolid_layer_cups_copy(out.ctypes.data_as(lp), None) == -1
    assert impli.last_error() == "implisolid_layer_cups_copy: bad arguments"
    got = np.zeros(len(runs), impli.CUP_RUN_DTYPE)
    assert impli.lib().implisolid_layer_cups_copy(out.ctypes.data_as(lp), got.ctypes.data_as(ip)) == 0 and np.array_equal(got, runs)


def test_two_calls_give_identical_results(impli):
    node, rect, z, H, W = _chunked_stack()
    a = (node, rect, W, H, z, 1, 1, 6)
    first = impli.layer_cups(*a, want_runs=True, return_stats=True)
    # another stack in between, with more runs: nothing of it may stay behind in the scratch
    bits = cu.PAINTED["dense_rows_framed"]()
    n2, r2, z2 = ii.painted(bits)
    assert impli.layer_cups(n2, r2, 130, 5, z2, 1, 1, 6, return_stats=True)[2][5:] == [585, 576, 576]
    again = impli.layer_cups(*a, want_runs=True, return_stats=True)
    assert all(np.array_equal(x, y) for x, y in zip(first[:4], again[:4])) and first[4] == again[4] and len(first[1]) > 0


def test_the_kernel_timer_reports_every_pass(impli):
    node, rect, z, H, W = _chunked_stack()
    a = (node, rect, W, H, z)
    assert impli.layer_cups_kernel_ms(False) == (-1.0,) * 4, "no timed call has run in this process"
    impli.layer_cups(*a)
    assert impli.layer_cups_kernel_ms(True) == (-1.0,) * 4, "an untimed call leaves the figures"
    try:
        impli.layer_cups(*a)
        ms = impli.layer_cups_kernel_ms(True)
    finally:
        impli.layer_cups_kernel_ms(False)
    print("raster, count + scan + emit + frame, link + mark + head, finish ms", ms)
    assert len(ms) == 4 and all(0 <= v < 1000 for v in ms)


def test_a_failed_call_empties_the_slot(impli):
    node, rect, z, H, W = _chunked_stack()
    a = (node, rect, W, H, z)
    assert len(impli.layer_cups(*a)[1]) > 0
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_cups(*a, connectivity=8)
    assert "connectivity" in str(e.value)
    out = np.zeros(7, np.int64)
    assert impli.lib().implisolid_layer_cups_copy(out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == -1
    assert impli.last_error() == cc.NO_COPY
    assert len(impli.layer_cups(*a)[1]) > 0, "and the next call works"
