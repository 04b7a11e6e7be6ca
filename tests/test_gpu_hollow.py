"""Hollowing the layer stack (implisolid_layer_hollow) on the GPU.

The reference is tests/np_hollow.py's brute force, which searches every solid voxel's lens for an empty voxel and
goes through no distance transform, on images that do not come from the raster kernels: np_raster.coverage of the
oracle's field values (as in test_gpu_raster.py), or the bit pattern itself for the painted stacks of
tests/hollow_inputs.py.  out and the records are integers and must equal it exactly, whatever the pruning level
skips or fills, however the layers are chunked and however far the window reaches.  The preconditions of the cases
are asserted without a GPU in test_cpu_hollow.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hollow_inputs as hi   # noqa: E402
import np_hollow   # noqa: E402
import test_cpu_hollow as ch   # noqa: E402  (the cached restatements; its tests are not collected from here)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

SHAPES = gm.SHAPES
RECTS = gr.RECTS
GRIDS = gr.GRIDS


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_hollow(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, cov, threshold, want_core):
    """out, records and the totals against the core mask of the restatement"""
    out, rec, stats = got
    cov = np.asarray(cov, np.uint8)
    solid = cov >= threshold
    want_rec = np.stack([solid.sum(axis=(1, 2)), want_core.sum(axis=(1, 2))], axis=1).astype(np.int64)
    rows = np_hollow.as_rows(rec)
    assert rec.dtype == impli.HOLLOW_DTYPE and rows.shape == want_rec.shape
    if out is not None:
        want_out = np.where(want_core, np.uint8(0), cov)
        assert out.dtype == np.uint8 and out.shape == want_out.shape
        bad = np.argwhere(out != want_out)
        assert len(bad) == 0, ("first differing [l, py, px]", bad[:5].tolist(), [int(out[tuple(b)]) for b in bad[:5]],
                               [int(want_out[tuple(b)]) for b in bad[:5]], len(bad))
    bad = np.argwhere((rows != want_rec).any(axis=1))
    assert len(bad) == 0, ("first differing records", bad[:3, 0].tolist(), rows[bad[:3, 0]].tolist(), want_rec[bad[:3, 0]].tolist())
    assert stats[5:] == [int(solid.sum()), int(want_core.sum()), len(cov)]


def _painted(impli, bits, wall2, ends, level=2, **kw):
    node, rect, z = hi.painted(bits)
    return _run(impli, level, node, rect, bits.shape[2], bits.shape[1], z, wall2, 1, 1, ends, **kw)


# ---- the box, closed form --------------------------------------------------------------------------------------------
def test_the_box_s_core_is_the_box_shrunk_by_the_wall(impli):
    w2 = impli.hollow_wall2(*hi.BOX_WALL)
    assert w2.tolist() == [9, 8, 5, 0]
    bits = hi.box()
    got = _painted(impli, bits, w2, 0)
    _check(impli, got, bits, 1, hi.box_core(3))
    assert got[2][6] == 34 * 34 * 6


def test_the_box_against_the_ends_of_the_stack(impli):
    w2 = impli.hollow_wall2(*hi.BOX_WALL)
    bits = hi.box_touching()
    outs = []
    for ends, layers in ((0, range(0, 14)), (1, range(3, 14)), (2, range(0, 11)), (3, range(3, 11))):
        want = np.zeros_like(bits)
        want[list(layers), 7:41, 7:41] = True
        got = _painted(impli, bits, w2, ends)
        _check(impli, got, bits, 1, want)
        outs.append(got[0].tobytes())
    assert len(set(outs)) == 4


# ---- one hole ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hi.HOLE_WALLS))
def test_the_shell_round_one_hole_is_the_digital_ellipsoid(impli, name):
    w2 = impli.hollow_wall2(*hi.HOLE_WALLS[name])
    bits, want = ch.restated("one_hole", w2, 0)
    got = _painted(impli, bits, w2, 0)
    _check(impli, got, bits, 1, want)
    hx, hy, hl = hi.HOLE
    l, y, x = np.mgrid[0:9, 0:70, 0:70]
    dl = np.abs(l - hl)
    lens = (dl < len(w2)) & ((x - hx) ** 2 + (y - hy) ** 2 <= np.array(w2.tolist() + [-1] * 9)[np.minimum(dl, len(w2))])
    assert np.array_equal(got[0] != 0, lens & bits)


# ---- the painted stacks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", sorted(hi.WALLS))
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", sorted(hi.PAINTED))
def test_painted_stacks_equal_the_brute_force(impli, name, level, reach):
    w2 = hi.WALLS[reach]
    for ends in (0, 3):
        bits, want = ch.restated(name, w2, ends)
        got = _painted(impli, bits, w2, ends, level)
        print(name, level, reach, ends, "records", np_hollow.as_rows(got[1]).tolist(), "stats", got[2])
        _check(impli, got, bits, 1, want)


@pytest.mark.parametrize("H", hi.SIZES)
@pytest.mark.parametrize("W", hi.SIZES)
def test_tile_edges(impli, W, H):
    bits = hi.sized(W, H)
    _check(impli, _painted(impli, bits, hi.SIZED_WALL, 0), bits, 1, np_hollow.core(bits, hi.SIZED_WALL, 0))


@pytest.mark.parametrize("ends", [0, 3])
@pytest.mark.parametrize("n_layers", hi.DEPTHS)
def test_stacks_shorter_and_longer_than_the_window(impli, n_layers, ends):
    bits = hi.deep(n_layers)
    _check(impli, _painted(impli, bits, hi.DEPTH_WALL, ends), bits, 1, np_hollow.core(bits, hi.DEPTH_WALL, ends))


@pytest.mark.parametrize("ends", [0, 1, 2])
def test_a_reach_larger_than_the_stack(impli, ends, monkeypatch):
    bits = hi.shallow()
    want = np_hollow.core(bits, hi.FAR_REACH_WALL, ends)
    _check(impli, _painted(impli, bits, hi.FAR_REACH_WALL, ends), bits, 1, want)
    monkeypatch.setenv("IMPLISOLID_HOLLOW_CHUNK", "1")   # a layer per chunk
    got = _painted(impli, bits, hi.FAR_REACH_WALL, ends)
    monkeypatch.delenv("IMPLISOLID_HOLLOW_CHUNK")
    assert got[2][4] == len(bits)
    _check(impli, got, bits, 1, want)


# ---- chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", sorted(hi.WALLS))
def test_chunks_of_one_three_and_twelve_layers_give_the_same(impli, reach, monkeypatch):
    w2 = hi.WALLS[reach]
    bits, want = ch.restated("staircase", w2, 3)
    results = []
    for items, chunks in ((None, 1), (108, 1), (27, 4), (9, 12), (1, 12)):   # nine raster tiles a layer
        if items is not None:
            monkeypatch.setenv("IMPLISOLID_HOLLOW_CHUNK", str(items))
        got = _painted(impli, bits, w2, 3, 0 if items == 1 else 2)
        if items is not None:
            monkeypatch.delenv("IMPLISOLID_HOLLOW_CHUNK")
        assert got[2][4] == chunks and got[2][7] == 12, (items, got[2])
        _check(impli, got, bits, 1, want)
        results.append(got)
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1]) and r[2][5:] == results[0][2][5:]


# ---- the shapes ------------------------------------------------------------------------------------------------------
SHAPE_WALL = [2, 1]


def _shape_case(impli, oracle, name, rect, W, H, s, threshold, level, z=None, wall2=SHAPE_WALL, ends=0, **kw):
    z = gr.Z if z is None else z
    cov = gr._ref(impli, oracle, name, kw.pop("shape", None) or SHAPES[name], RECTS[rect], W, H, s, z, kw.get("ignore_root_matrix", False))[0]
    want = np_hollow.core(cov >= threshold, wall2, ends)
    got = _run(impli, level, kw.pop("run_shape", None) or SHAPES[name], RECTS[rect], W, H, z, wall2, s, threshold, ends, **kw)
    print(name, (W, H, s), rect, level, threshold, "records", np_hollow.as_rows(got[1]).tolist(), "stats", got[2])
    _check(impli, got, cov, threshold, want)
    shell = got[0][~want]
    assert np.array_equal(shell, cov[~want]), "grey levels are kept in the shell"
    return got, cov, want


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("rect", sorted(RECTS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_equal_the_brute_force(impli, oracle, name, rect, W, H, s, level):
    for threshold in sorted({1, s * s}):
        got, cov, want = _shape_case(impli, oracle, name, rect, W, H, s, threshold, level)
        assert got[2][4] == 1
        if level == 0:
            assert got[2][1] == got[2][0] and got[2][2] == 0


def test_grey_levels_survive_in_a_shape_s_shell(impli, oracle):
    got, cov, want = _shape_case(impli, oracle, "csg", "unit", 40, 40, 4, 16, 2, wall2=[1, 0], ends=0)
    grey = (cov > 0) & (cov < 16)
    assert grey.any() and np.array_equal(got[0][grey], cov[grey]) and (got[0][want] == 0).all()


def test_chunks_of_a_shape_give_the_same(impli, oracle, monkeypatch):
    monkeypatch.setenv("IMPLISOLID_HOLLOW_CHUNK", "36")
    got, cov, want = _shape_case(impli, oracle, "tree_deep", "non_dyadic", 40, 40, 2, 2, 2, z=gr.Z12, wall2=[2, 1, 0], ends=3)
    monkeypatch.delenv("IMPLISOLID_HOLLOW_CHUNK")
    assert got[2][4] == 3 and got[2][7] == 12


# ---- cross-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 5])
def test_reach_zero_is_the_layer_s_own_erosion(impli, w):
    a = (SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z, 2)
    out, rec, stats = impli.layer_hollow(*a[:5], [w], a[5], 3, 0, return_stats=True)
    dist, drec, dstats = impli.layer_distance(*a, 3, 0, return_stats=True)
    cov, sums, rstats = impli.raster_layers(*a, return_stats=True)
    core = impli.offset_mask(dist, -w)
    assert core.any() or w > 1
    assert np.array_equal(out == 0, core | (cov == 0)) and np.array_equal(out[~core], cov[~core])
    assert rec["core"].tolist() == core.sum(axis=(1, 2)).tolist() and rec["solid"].tolist() == drec["solid"].tolist()
    assert stats[:5] == rstats == dstats[:5] and stats[5] == dstats[5] == int(rec["solid"].sum()) > 0 and stats[7] == len(gr.Z)


# ---- call forms ----------------------------------------------------------------------------------------------------------
def test_without_out_the_records_are_the_same(impli, monkeypatch):
    a = (SHAPES["tree_deep"], RECTS["unit"], 40, 40, gr.Z12, [2, 1], 2, 2, 3)
    out, rec, stats = impli.layer_hollow(*a, return_stats=True)
    none, rec2, stats2 = impli.layer_hollow(*a, want_out=False, return_stats=True)
    assert none is None and np.array_equal(rec, rec2) and stats == stats2 and rec["solid"].sum() > 0
    monkeypatch.setenv("IMPLISOLID_HOLLOW_CHUNK", "27")
    none, rec3, stats3 = impli.layer_hollow(*a, want_out=False, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_HOLLOW_CHUNK")
    assert none is None and np.array_equal(rec, rec3) and stats3[4] == 4 and stats3[5:] == stats[5:]
    assert len(impli.layer_hollow(*a)) == 2


def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, [1, 0], 4, 9, 0)
    first = impli.layer_hollow(*a, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the rings
    bits = hi.box()
    assert _painted(impli, bits, [9, 8, 5, 0], 0)[2][6] == 34 * 34 * 6
    again = impli.layer_hollow(*a, return_stats=True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2] and first[1]["solid"].sum() > 0


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    moved = dict(SHAPES["csg"], matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    ignored = _shape_case(impli, oracle, "csg_ignored", "unit", 40, 40, 2, 2, level, shape=moved, run_shape=moved, ignore_root_matrix=True)
    kept = _shape_case(impli, oracle, "csg_moved", "unit", 40, 40, 2, 2, level, shape=moved, run_shape=moved)
    assert not np.array_equal(ignored[0][0], kept[0][0]), "the root matrix moves the solid"


def test_the_kernel_timer_reports_every_pass(impli):
    impli.layer_hollow_kernel_ms(True)
    try:
        impli.layer_hollow(SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, [2, 1], 2, 1, 0)
        ms = impli.layer_hollow_kernel_ms(True)
    finally:
        impli.layer_hollow_kernel_ms(False)
    print("raster, ring copy + columns, rows, window ms", ms)
    assert len(ms) == 4 and all(0 < v < 1000 for v in ms)
