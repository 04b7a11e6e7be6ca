"""Islands of the layers (implisolid_islands) on the GPU.

The reference is tests/np_islands.py's restatement of the definition on coverage images that do not come
from the raster kernels: np_raster.coverage of the oracle's field values (ImplicitService.eval for the
sdf_3d shape, as in test_gpu_raster.py), or the bit pattern itself for the painted stacks of
tests/island_inputs.py.  comp_offsets, the records and the labels are integers and must equal it exactly,
whatever the pruning level skips or fills, however the layers are chunked and wherever a component crosses
the 64 x 32-pixel tiles of the label pass.  The preconditions of the cases are asserted without a GPU in
test_cpu_islands.py.  NaN and infinite samples are pinned in test_gpu_nonfinite.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import island_inputs as ii   # noqa: E402
import np_islands   # noqa: E402
import test_cpu_islands as ci   # noqa: E402  (the sphere pair and the cached restatements; its tests are not collected from here)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

SHAPES = dict(gm.SHAPES, pair=ci.PAIR)
PLANES = {name: gr.Z for name in gm.NAMES}
PLANES["pair"] = ci.PAIR_Z
RECTS = gr.RECTS
GRIDS = gr.GRIDS

_REF = {}


def _ref(impli, oracle, name, rect, W, H, s, threshold, connectivity, z=None, shape=None, ignore_root_matrix=False):
    z = PLANES[name] if z is None else z
    key = (name, rect, W, H, s, threshold, connectivity, tuple(float(v) for v in z), ignore_root_matrix)
    if key not in _REF:
        cov = gr._ref(impli, oracle, name, shape or SHAPES[name], RECTS[rect], W, H, s, z, ignore_root_matrix)[0]
        _REF[key] = np_islands.islands(cov, threshold, connectivity)
    return _REF[key]


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_islands(*a, want_labels=True, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, want):
    offs, comps, labels, stats = got
    ro, rc, rl = want
    rows = np_islands.as_rows(comps)
    assert offs.dtype == np.int64 and comps.dtype == impli.COMP_DTYPE and labels.dtype == np.int32 and labels.shape == rl.shape
    assert np.array_equal(offs, ro), (offs.tolist(), ro.tolist())
    bad = np.argwhere(labels != rl)
    assert len(bad) == 0, ("first differing [l, py, px]", bad[:5].tolist(), len(bad))
    assert rows.shape == rc.shape
    bad = np.argwhere((rows != rc).any(axis=1))
    assert len(bad) == 0, ("first differing records", rows[bad[:3, 0]].tolist(), rc[bad[:3, 0]].tolist(), len(bad))
    assert stats[5] == len(rc) and stats[6] == int((rc[:, 2] == 0).sum()) == len(impli.islands_of(comps))
    assert stats[7] == int(rc[:, 1].sum()) == int((labels >= 0).sum())


# ---- the shapes ------------------------------------------------------------------------------------------------
# the sphere pair's planes are chosen for the unit rect
SHAPE_RECTS = [(name, rect) for name in sorted(SHAPES) for rect in sorted(RECTS) if name != "pair" or rect == "unit"]


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("name, rect", SHAPE_RECTS)
def test_records_and_labels_equal_the_restatement(impli, oracle, name, rect, W, H, s, level):
    z = PLANES[name]
    for threshold in (1, s * s):
        for connectivity in (4, 8):
            want = _ref(impli, oracle, name, rect, W, H, s, threshold, connectivity)
            got = _run(impli, level, SHAPES[name], RECTS[rect], W, H, z, s, threshold, connectivity)
            print(name, (W, H, s), rect, level, threshold, connectivity, "per layer", np.diff(got[0]).tolist(), "stats", got[3])
            _check(impli, got, want)
            assert got[3][4] == 1 and (len(want[1]) > 0 or threshold > 1), "at threshold 1 the case holds components"
            if level == 0:
                assert got[3][1] == got[3][0] and got[3][2] == 0
    if name != "pair":
        # the repeated plane (entries 1 and 3): by list order it lies above entry 2's image, and its labels repeat
        assert np.array_equal(got[2][1], got[2][3])
        # entry 0 is empty, entry 1 stands on it: all islands; a plane listed twice in a row rests on itself
        rows = np_islands.as_rows(got[1])
        assert (rows[rows[:, 7] == 1][:, 2] == 0).all()
        busiest = int(np.argmax(np.diff(_ref(impli, oracle, name, rect, W, H, s, 1, 8)[0])))
        twice = np.array([z[busiest], z[busiest]], np.float32)
        o2, c2 = impli.layer_islands(SHAPES[name], RECTS[rect], W, H, twice, s, 1, 8)
        r2 = np_islands.as_rows(c2)
        assert len(r2) and (r2[:, 2] == r2[:, 1]).all() and np.array_equal(r2[:o2[1], :7], r2[o2[1]:, :7])


def test_the_sphere_pair_s_upper_sphere_starts_as_an_island(impli):
    offs, comps = impli.layer_islands(ci.PAIR, RECTS["unit"], 40, 40, ci.PAIR_Z, 1, 1, 8)
    isl = impli.islands_of(comps)
    assert np.diff(offs).tolist() == [1, 2, 1, 0, 1, 1, 1]
    assert sorted(isl["layer"].tolist()) == [1, 4], "the small sphere beside the lower one, and the upper sphere's lowest plane"
    assert (comps[comps["layer"] >= 5]["below"] > 0).all()


# ---- the painted stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(ii.PAINTED))
def test_painted_stacks_equal_the_restatement(impli, name, connectivity, level):
    bits, ro, rc, rl = ci.restated(name, connectivity)
    node, rect, z = ii.painted(bits)
    got = _run(impli, level, node, rect, bits.shape[2], bits.shape[1], z, 1, 1, connectivity)
    print(name, connectivity, level, "per layer", np.diff(got[0]).tolist(), "stats", got[3])
    _check(impli, got, (ro, rc, rl))
    assert np.array_equal(got[2] >= 0, bits)


@pytest.mark.parametrize("H", ii.SIZES)
@pytest.mark.parametrize("W", ii.SIZES)
def test_tile_edges(impli, W, H):
    bits = ii.sized(W, H)
    node, rect, z = ii.painted(bits)
    for connectivity in (4, 8):
        want = np_islands.islands(bits.astype(np.uint8), 1, connectivity)
        _check(impli, _run(impli, 2, node, rect, W, H, z, 1, 1, connectivity), want)


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_a_solid_stack_is_one_component_a_layer_without_a_sample(impli, W, H, s):
    z = gr.Z
    offs, comps, labels, stats = _run(impli, 2, gm.BIG, RECTS["unit"], W, H, z, s, s * s, 4)
    assert offs.tolist() == list(range(len(z) + 1)) and (labels == 0).all()
    for l, c in enumerate(comps):
        assert c.tolist() == (0, W * H, W * H, 0, 0, W - 1, H - 1, l)
    assert stats[1] == 0 and stats[3] == 0 and stats[2] == stats[0] and stats[5:] == [len(z), 0, len(z) * W * H]


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_an_empty_stack_has_no_component(impli, W, H, s):
    offs, comps, labels, stats = _run(impli, 2, gm.AWAY, RECTS["unit"], W, H, gr.Z, s, 1, 8)
    assert (offs == 0).all() and len(comps) == 0 and (labels == -1).all() and stats[1:4] == [0, 0, 0] and stats[5:] == [0, 0, 0]


# ---- chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_three_and_twelve_chunks_give_the_same_records(impli, connectivity, monkeypatch):
    bits, ro, rc, rl = ci.restated("chunked", connectivity)
    node, rect, z = ii.painted(bits)
    one = _run(impli, 2, node, rect, 40, 40, z, 1, 1, connectivity)
    monkeypatch.setenv("IMPLISOLID_ISLANDS_CHUNK", "36")   # four layers of nine raster tiles
    three = _run(impli, 2, node, rect, 40, 40, z, 1, 1, connectivity)
    monkeypatch.setenv("IMPLISOLID_ISLANDS_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 0, node, rect, 40, 40, z, 1, 1, connectivity)
    monkeypatch.delenv("IMPLISOLID_ISLANDS_CHUNK")
    assert one[3][4] == 1 and three[3][4] == 3 and each[3][4] == 12
    for r in (one, three, each):
        _check(impli, r, (ro, rc, rl))
        assert r[3][5:] == one[3][5:]


def test_chunks_of_a_shape_give_the_same_records(impli, oracle, monkeypatch):
    want = _ref(impli, oracle, "tree_deep", "non_dyadic", 40, 40, 2, 2, 8, z=gr.Z12)
    monkeypatch.setenv("IMPLISOLID_ISLANDS_CHUNK", "36")
    got = _run(impli, 2, SHAPES["tree_deep"], RECTS["non_dyadic"], 40, 40, gr.Z12, 2, 2, 8)
    monkeypatch.delenv("IMPLISOLID_ISLANDS_CHUNK")
    assert got[3][4] == 3
    _check(impli, got, want)


# ---- cross-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [1, 3, 4])
def test_labels_cover_the_raster_image_at_the_threshold(impli, threshold):
    a = (SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z, 2)
    offs, comps, labels, stats = impli.layer_islands(*a, threshold, 8, want_labels=True, return_stats=True)
    cov, sums, rstats = impli.raster_layers(*a, return_stats=True)
    assert np.array_equal(labels >= 0, cov >= threshold) and stats[:5] == rstats
    assert int(comps["area"].sum()) == stats[7] == int((cov >= threshold).sum()) and len(impli.islands_of(comps)) == stats[6]
    plain = impli.layer_islands(*a, threshold, 8)
    assert len(plain) == 2 and np.array_equal(plain[0], offs) and np.array_equal(plain[1], comps), "want_labels changes no record"
    for l in range(len(gr.Z)):   # every record against its labels
        for c in comps[offs[l]:offs[l + 1]]:
            ys, xs = np.nonzero(labels[l] == c["seed"])
            assert (c["area"], c["x0"], c["y0"], c["x1"], c["y1"], c["layer"]) == (len(xs), xs.min(), ys.min(), xs.max(), ys.max(), l)
            assert c["seed"] == (ys * 40 + xs).min()


def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, 4, 9, 4)
    first = impli.layer_islands(*a, want_labels=True, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch
    bits = ii.checkerboard()
    node, rect, z = ii.painted(bits)
    assert impli.layer_islands(node, rect, 129, 129, z, 1, 1, 4, return_stats=True)[2][5] == 8321
    again = impli.layer_islands(*a, want_labels=True, return_stats=True)
    assert all(np.array_equal(x, y) for x, y in zip(first[:3], again[:3])) and first[3] == again[3] and len(first[1]) > 0


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    moved = dict(SHAPES["csg"], matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    ignored = _ref(impli, oracle, "csg_ignored", "unit", 40, 40, 2, 2, 8, z=gr.Z, shape=moved, ignore_root_matrix=True)
    kept = _ref(impli, oracle, "csg_moved", "unit", 40, 40, 2, 2, 8, z=gr.Z, shape=moved)
    plain = _ref(impli, oracle, "csg", "unit", 40, 40, 2, 2, 8)
    assert np.array_equal(ignored[2], plain[2]) and not np.array_equal(kept[2], plain[2]), "the root matrix moves the solid"
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 2, 8, ignore_root_matrix=True), ignored)
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 2, 8), kept)


def test_the_kernel_timer_reports_every_pass(impli):
    impli.islands_kernel_ms(True)
    try:
        impli.layer_islands(SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, 2, 1, 8)
        ms = impli.islands_kernel_ms(True)
    finally:
        impli.islands_kernel_ms(False)
    print("raster, tiles, merge, rows + scan, records + tally ms", ms)
    assert len(ms) == 5 and all(0 < v < 1000 for v in ms)


def test_a_failed_call_empties_the_slot(impli):
    import ctypes
    a = (SHAPES["egg"], RECTS["unit"], 40, 40, gr.Z, 2)
    assert len(impli.layer_islands(*a, 1, 8)[1]) > 0
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_islands(*a, 1, 6)
    assert "connectivity" in str(e.value)
    out = np.zeros(8, np.int32)
    assert impli.lib().implisolid_islands_copy(out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
    assert impli.last_error() == ci.NO_COPY
    assert len(impli.layer_islands(*a, 1, 8)[1]) > 0, "and the next call works"
