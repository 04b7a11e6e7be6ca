"""Bodies of the layer stack (implisolid_layer_bodies) on the GPU.

The reference is tests/np_bodies.py's restatement of the definition on coverage images that do not come from the
raster kernels: the bit pattern itself for the painted stacks of tests/body_inputs.py, or np_raster.coverage of
the oracle's field values for the shapes (test_gpu_raster._ref, as in test_gpu_islands.py).  run_offsets, the body
records, the run records and their decoded label stack are integers and must equal it exactly, for both targets
and both connectivities, whatever the pruning level skips or fills and however the layers are chunked.  The
preconditions of the cases are asserted without a GPU in test_cpu_bodies.py.

Rows of two full steps of the walk with runs in every lane (dense_511, dense_512, dense_512_ends) and of five steps
(the comb, 1030 pixels), rows of two to four rounds of 64 runs (the dense rows, rounds) and a stack whose arrays
outgrow their block chunk by chunk in a process of its own (growing, tests/bodies_grow_worker.py) are among them.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_inputs as bi   # noqa: E402
import island_inputs as ii   # noqa: E402
import np_bodies   # noqa: E402
import np_islands   # noqa: E402
import run_inputs as ri   # noqa: E402
import test_cpu_bodies as cb   # noqa: E402  (the cached restatements; its tests are not collected from here)
import test_cpu_islands as ci   # noqa: E402  (the sphere pair)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

SHAPES = dict(gm.SHAPES, pair=ci.PAIR)
PLANES = {name: gr.Z for name in gm.NAMES}   # a plane that misses every shape, a repeated plane and an unsorted order
PLANES["pair"] = ci.PAIR_Z
RECTS = gr.RECTS
GRIDS = [(40, 40, 1), (40, 40, 2)]
CASES = [(target, connectivity) for target in (1, 0) for connectivity in (6, 26)]


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_bodies(*a, want_runs=True, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, want, W, H):
    offs, bodies, runs, stats = got
    ro, rb, rr, rd = want
    assert offs.dtype == np.int64 and bodies.dtype == impli.BODY_DTYPE and runs.dtype == impli.BODY_RUN_DTYPE
    assert np.array_equal(offs, ro), (offs.tolist(), ro.tolist())
    rows = np_bodies.as_rows(bodies)
    assert rows.shape == rb.shape, (rows.shape, rb.shape, rows[:4].tolist(), rb[:4].tolist())
    bad = np.argwhere((rows != rb).any(axis=1))
    assert len(bad) == 0, ("first differing bodies", rows[bad[:3, 0]].tolist(), rb[bad[:3, 0]].tolist(), len(bad))
    rrows = np_bodies.as_rows(runs, np_bodies.RUN_FIELDS)
    assert rrows.shape == rr.shape
    bad = np.argwhere((rrows != rr).any(axis=1))
    assert len(bad) == 0, ("first differing runs", bad[:3, 0].tolist(), rrows[bad[:3, 0]].tolist(), rr[bad[:3, 0]].tolist(), len(bad))
    dec = impli.bodies_decode(offs, runs, W, H)
    assert dec.dtype == np.int32 and np.array_equal(dec, rd)
    assert stats[5] == len(rr) and stats[6] == len(rb) and stats[7] == int((rd >= 0).sum()) == int(rb[:, 1].sum())


# ---- the painted stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("target, connectivity", CASES)
@pytest.mark.parametrize("name", sorted(bi.PAINTED))
def test_painted_stacks_equal_the_restatement(impli, name, target, connectivity, level):
    bits, ro, rb, rr, rd = cb.restated(name, target, connectivity)
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    got = _run(impli, level, node, rect, W, H, z, 1, 1, target, connectivity)
    print(name, target, connectivity, level, "runs per layer", np.diff(got[0]).tolist(), "bodies", len(got[1]), "stats", got[3])
    _check(impli, got, (ro, rb, rr, rd), W, H)
    assert np.array_equal(impli.bodies_decode(got[0], got[2], W, H) >= 0, bits == (target == 1))
    assert got[3][4] == 1
    if level == 0:
        assert got[3][1] == got[3][0] and got[3][2] == 0


def test_the_painted_answers_a_slicer_wants(impli):
    # the default connectivity is the dual pair: 26 for the solid, 6 for the empty class
    bits = bi.cavities()
    node, rect, z = ii.painted(bits)
    offs, bodies = impli.layer_bodies(node, rect, 24, 24, z, target=0)
    assert np.array_equal(np_bodies.as_rows(bodies), cb.restated("cavities", 0, 6)[2])
    assert sorted(impli.enclosed_voids(bodies, 24, 24, 7)["volume"].tolist()) == [18, 18]
    assert impli.enclosed_voids(impli.layer_bodies(node, rect, 24, 24, z, target=0, connectivity=26)[1], 24, 24, 7)["volume"].tolist() == [18]
    bits = bi.floating()
    node, rect, z = ii.painted(bits)
    offs, bodies = impli.layer_bodies(node, rect, 20, 20, z)
    assert np.array_equal(np_bodies.as_rows(bodies), cb.restated("floating", 1, 26)[2])
    assert len(bodies) == 2 and impli.floating_bodies(bodies)["volume"].tolist() == [18]
    for name, n in (("arch", 1), ("arch_open", 2), ("arch_bottom", 1)):
        node, rect, z = ii.painted(bi.PAINTED[name]())
        assert len(impli.layer_bodies(node, rect, 70, 40, z)[1]) == n, name


@pytest.mark.parametrize("H", bi.SIZES)
@pytest.mark.parametrize("W", bi.SIZES)
def test_sizes_around_the_steps_of_the_walk(impli, W, H):
    for L in bi.LAYERS:
        bits = bi.sized(W, H, L)
        node, rect, z = ii.painted(bits)
        for target, connectivity in CASES:
            want = np_bodies.bodies(bits.astype(np.uint8), 1, target, connectivity)
            _check(impli, _run(impli, 2, node, rect, W, H, z, 1, 1, target, connectivity), want, W, H)


def test_rows_of_256_and_257_pixels(impli):
    # a row that ends with the walk's step (the last run is closed behind the loop) and one pixel past it
    for W in (256, 257):
        bits = np.random.default_rng(W).random((2, 3, W)) < 0.6
        bits[:, 0, W - 3:] = True
        bits[:, 1, W - 1] = False
        bits[0, 2, :] = True
        node, rect, z = ii.painted(bits)
        for target, connectivity in CASES:
            want = np_bodies.bodies(bits.astype(np.uint8), 1, target, connectivity)
            _check(impli, _run(impli, 2, node, rect, W, 3, z, 1, 1, target, connectivity), want, W, 3)


# ---- one layer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ii.PAINTED))
def test_one_layer_is_layer_islands(impli, name):
    stack = ii.PAINTED[name]()
    H, W = stack.shape[1:]
    node, rect, z = ii.painted(stack)
    for l in range(min(2, len(z))):
        for conn3, conn2 in ((6, 4), (26, 8)):
            offs, bodies = impli.layer_bodies(node, rect, W, H, z[l:l + 1], 1, 1, 1, conn3)
            io, comps = impli.layer_islands(node, rect, W, H, z[l:l + 1], 1, 1, conn2)
            assert len(bodies) == len(comps) > 0
            for a, b in (("seed", "seed"), ("volume", "area"), ("x0", "x0"), ("y0", "y0"), ("x1", "x1"), ("y1", "y1")):
                assert np.array_equal(bodies[a], comps[b].astype(np.int64)), (name, l, conn3, a)
            assert (bodies["l0"] == 0).all() and (bodies["l1"] == 0).all()


def test_one_layer_of_a_shape_is_layer_islands(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 40, 40, gr.Z[1:2], 2)
    for threshold in (1, 4):
        offs, bodies = impli.layer_bodies(*a, threshold, 1, 26)
        io, comps = impli.layer_islands(*a, threshold, 8)
        assert len(bodies) == len(comps) > 0 and np.array_equal(bodies["seed"], comps["seed"]) and np.array_equal(bodies["volume"], comps["area"])


# ---- chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target, connectivity", CASES)
@pytest.mark.parametrize("name, tiles", [("chunked", 9), ("arch", 15)])
def test_chunks_give_the_same_answer(impli, name, tiles, target, connectivity, monkeypatch):
    bits, ro, rb, rr, rd = cb.restated(name, target, connectivity)
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    one = _run(impli, 2, node, rect, W, H, z, 1, 1, target, connectivity)
    monkeypatch.setenv("IMPLISOLID_BODIES_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 0, node, rect, W, H, z, 1, 1, target, connectivity)
    monkeypatch.setenv("IMPLISOLID_BODIES_CHUNK", str(4 * tiles))   # four layers of raster tiles
    four = _run(impli, 2, node, rect, W, H, z, 1, 1, target, connectivity)
    monkeypatch.delenv("IMPLISOLID_BODIES_CHUNK")
    assert one[3][4] == 1 and each[3][4] == L and four[3][4] == (L + 3) // 4
    for r in (one, each, four):
        _check(impli, r, (ro, rb, rr, rd), W, H)
        assert all(np.array_equal(x, y) for x, y in zip(r[:3], one[:3])) and r[3][5:] == one[3][5:]


def test_a_fresh_process_grows_its_arrays_chunk_by_chunk(impli, tmp_path):
    # In this process the scratch that earlier tests left holds any test stack, and grow_keeping returns at once.
    # A child's engine starts empty: with a layer per chunk the runs and the union-find of `growing` take a larger
    # block in most chunks, the earlier chunks' entries copied over (test_cpu_bodies.py restates the sizes)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bodies_grow_worker.py")
    for target, connectivity in cb.GROWING_CASES:
        bits, ro, rb, rr, rd = cb.restated("growing", target, connectivity)
        L, H, W = bits.shape
        out = str(tmp_path / ("growing_%d_%d.npz" % (target, connectivity)))
        env = {k: v for k, v in os.environ.items() if k != "IMPLISOLID_BODIES_CHUNK"}
        p = subprocess.run([sys.executable, worker, out, str(target), str(connectivity)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, "the worker for %s ended with %d:\n%s" % ((target, connectivity), p.returncode, p.stderr[-4000:])
        with np.load(out) as f:
            got = (f["offsets"], f["bodies"], f["runs"], f["stats"].tolist())
        print("growing", target, connectivity, "runs per layer", np.diff(got[0]).tolist(), "bodies", len(got[1]), "stats", got[3])
        _check(impli, got, (ro, rb, rr, rd), W, H)
        assert got[3][4] == L, "a layer per chunk"


# ---- rows of five steps: the comb ----------------------------------------------------------------------------------
def _comb_ref(oracle, s, threshold, target, connectivity):
    # of the reference image that test_gpu_raster._ref keeps; test_cpu_bodies.py asserts what it holds
    return cb.comb_bodies(oracle, s, threshold, target, connectivity)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("s, threshold", [(1, 1), (2, 1), (2, 4)])
def test_the_comb_equals_the_restatement(impli, oracle, s, threshold, level):
    W, H, z = ri.COMB_W, ri.COMB_H, ri.COMB_Z
    assert np.array_equal(cb.comb_image(oracle, s), gr._ref(impli, oracle, "comb", ri.COMB, ri.COMB_RECT, W, H, s, z)[0])
    for target, connectivity in CASES:
        want = _comb_ref(oracle, s, threshold, target, connectivity)
        got = _run(impli, level, ri.COMB, ri.COMB_RECT, W, H, z, s, threshold, target, connectivity)
        print("comb", s, threshold, level, target, connectivity, "runs per layer", np.diff(got[0]).tolist(), "bodies", len(got[1]), "stats", got[3])
        _check(impli, got, want, W, H)
        assert got[3][4] == 1 and len(want[1]) > 0
        if target == 0 and threshold == 1:
            assert len(got[1]) == 1 and got[1][0].tolist() == (0, got[3][7], 0, 0, 0, W - 1, H - 1, 1), "the empty class is one body"


def test_comb_chunks_give_the_same_answer(impli, oracle, monkeypatch):
    z = ri.COMB_Z
    for target, connectivity in ((1, 26), (0, 6)):
        want = _comb_ref(oracle, 1, 1, target, connectivity)
        monkeypatch.setenv("IMPLISOLID_BODIES_CHUNK", "1")    # a layer per chunk: plane 1 links to plane 0 in the stack's arrays
        each = _run(impli, 2, ri.COMB, ri.COMB_RECT, ri.COMB_W, ri.COMB_H, z, 1, 1, target, connectivity)
        monkeypatch.delenv("IMPLISOLID_BODIES_CHUNK")
        assert each[3][4] == len(z) == 2
        _check(impli, each, want, ri.COMB_W, ri.COMB_H)


# ---- the shapes ------------------------------------------------------------------------------------------------
SHAPE_RECTS = [(name, rect) for name in sorted(SHAPES) for rect in sorted(RECTS) if name != "pair" or rect == "unit"]
_REF = {}


def _ref(impli, oracle, name, rect, W, H, s, threshold, target, connectivity):
    key = (name, rect, W, H, s, threshold, target, connectivity)
    if key not in _REF:
        cov = gr._ref(impli, oracle, name, SHAPES[name], RECTS[rect], W, H, s, PLANES[name])[0]
        _REF[key] = np_bodies.bodies(cov, threshold, target, connectivity)
    return _REF[key]


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("name, rect", SHAPE_RECTS)
def test_shapes_equal_the_restatement(impli, oracle, name, rect, W, H, s, level):
    z = PLANES[name]
    for threshold in sorted({1, s * s}):
        for target, connectivity in CASES:
            want = _ref(impli, oracle, name, rect, W, H, s, threshold, target, connectivity)
            got = _run(impli, level, SHAPES[name], RECTS[rect], W, H, z, s, threshold, target, connectivity)
            print(name, (W, H, s), rect, level, threshold, target, connectivity, "bodies", np_bodies.as_rows(got[1]).tolist()[:4], "stats", got[3])
            _check(impli, got, want, W, H)
            assert got[3][4] == 1 and (len(want[1]) > 0 or threshold > 1)


def test_the_sphere_pair_is_three_bodies_two_of_them_floating(impli):
    # the lower sphere in planes 0 .. 2, the small one beside it in plane 1 only, plane 3 in the gap, the upper sphere in 4 .. 6
    a = (ci.PAIR, RECTS["unit"], 40, 40, ci.PAIR_Z)
    for connectivity in (6, 26):
        offs, bodies = impli.layer_bodies(*a, 1, 1, 1, connectivity)
        assert list(zip(bodies["l0"].tolist(), bodies["l1"].tolist())) == [(0, 2), (1, 1), (4, 6)]
        assert (np.diff(bodies["seed"]) > 0).all() and (bodies["seed"] // 1600 == bodies["l0"]).all()
        assert impli.floating_bodies(bodies)["l0"].tolist() == [1, 4]
        # the empty class is one body that touches every face: there is no enclosed void
        offs0, empty = impli.layer_bodies(*a, 1, 1, 0, connectivity)
        assert len(empty) == 1 and empty[0].tolist() == (0, 7 * 1600 - int(bodies["volume"].sum()), 0, 0, 0, 39, 39, 6)
        assert len(impli.enclosed_voids(empty, 40, 40, 7)) == 0


# ---- invariants ------------------------------------------------------------------------------------------------------
def test_volumes_runs_and_the_copy_entry(impli):
    lp, ip = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    a = (SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z)
    cov, sums, rstats = impli.raster_layers(*a, 1, return_stats=True)
    offs, bodies, runs, stats = impli.layer_bodies(*a, 1, 1, 1, 26, want_runs=True, return_stats=True)
    assert int(bodies["volume"].sum()) == stats[7] == int(sums.sum()) == int(runs["length"].sum()) and stats[:5] == rstats
    assert stats[5] == len(runs) == offs[-1] and stats[6] == len(bodies) > 0
    e = impli.layer_bodies(*a, 1, 1, 0, 6, return_stats=True)
    assert int(e[1]["volume"].sum()) == e[2][7] == cov.size - stats[7]
    for s, threshold in ((2, 1), (2, 4)):
        cov2 = impli.raster_layers(*a, s)[0]
        for target in (0, 1):
            o, b, st = impli.layer_bodies(*a, s, threshold, target, return_stats=True)
            assert int(b["volume"].sum()) == st[7] == int(((cov2 >= threshold) == (target == 1)).sum())
    # without want_runs the records are the same, and the copy entry takes runs = NULL
    plain = impli.layer_bodies(*a, 1, 1, 1, 26)
    assert len(plain) == 2 and np.array_equal(plain[0], offs) and np.array_equal(plain[1], bodies)
    out = np.zeros(len(bodies), impli.BODY_DTYPE)
    assert impli.lib().implisolid_layer_bodies_copy(out.ctypes.data_as(lp), None) == 0 and np.array_equal(out, bodies)
    # a call that asked for runs needs the pointer
    impli.layer_bodies(*a, 1, 1, 1, 26, want_runs=True)
    assert impli.lib().implisolid_layer_bodies_copy(out.ctypes.data_as(lp), None) == -1
    assert impli.last_error() == "implisolid_layer_bodies_copy: bad arguments"
    got = np.zeros(len(runs), impli.BODY_RUN_DTYPE)
    assert impli.lib().implisolid_layer_bodies_copy(out.ctypes.data_as(lp), got.ctypes.data_as(ip)) == 0 and np.array_equal(got, runs)


def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, 4, 9, 1, 26)
    first = impli.layer_bodies(*a, want_runs=True, return_stats=True)
    # another stack in between, with more runs: nothing of it may stay behind in the scratch
    node, rect, z = ii.painted(bi.dense_rows())
    assert impli.layer_bodies(node, rect, 130, 3, z, 1, 1, 1, 6, return_stats=True)[2][5:] == [585, 585, 585]
    again = impli.layer_bodies(*a, want_runs=True, return_stats=True)
    assert all(np.array_equal(x, y) for x, y in zip(first[:3], again[:3])) and first[3] == again[3] and len(first[1]) > 0


def test_the_kernel_timer_reports_every_pass(impli):
    a = (SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, 2)
    assert impli.layer_bodies_kernel_ms(False) == (-1.0,) * 4, "no timed call has run in this process"
    impli.layer_bodies(*a)
    assert impli.layer_bodies_kernel_ms(True) == (-1.0,) * 4, "an untimed call leaves the figures"
    try:
        impli.layer_bodies(*a)
        ms = impli.layer_bodies_kernel_ms(True)
    finally:
        impli.layer_bodies_kernel_ms(False)
    print("raster, count + scan + emit, link, finish ms", ms)
    assert len(ms) == 4 and all(0 <= v < 1000 for v in ms)


def test_a_failed_call_empties_the_slot(impli):
    a = (SHAPES["egg"], RECTS["unit"], 40, 40, gr.Z, 2)
    assert len(impli.layer_bodies(*a)[1]) > 0
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_bodies(*a, connectivity=8)
    assert "connectivity" in str(e.value)
    out = np.zeros(8, np.int64)
    assert impli.lib().implisolid_layer_bodies_copy(out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == -1
    assert impli.last_error() == cb.NO_COPY
    assert len(impli.layer_bodies(*a)[1]) > 0, "and the next call works"
