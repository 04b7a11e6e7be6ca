"""Pixel distance field of the layers (implisolid_layer_distance) on the GPU.

The reference is tests/np_distance.py's brute-force restatement of the definition on images that do not come
from the raster kernels: np_raster.coverage of the oracle's field values (as in test_gpu_raster.py), or the
bit pattern itself for the painted stacks of tests/distance_inputs.py.  dist and the records are integers and
must equal it exactly, whatever the pruning level skips or fills, however the layers are chunked and however
far a search runs.  The preconditions of the cases are asserted without a GPU in test_cpu_distance.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_inputs as di   # noqa: E402
import np_distance   # noqa: E402
import test_cpu_distance as cd   # noqa: E402  (the cached restatements; its tests are not collected from here)
import test_gpu_mass as gm   # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its reference images of the shapes)

pytestmark = pytest.mark.gpu

NONE = np_distance.NONE
SHAPES = gm.SHAPES
RECTS = gr.RECTS
GRIDS = gr.GRIDS

_REF = {}


def _ref(impli, oracle, name, rect, W, H, s, threshold, z=None, shape=None, ignore_root_matrix=False):
    """the restated field of a shape's reference image; computed once per case"""
    z = gr.Z if z is None else z
    key = (name, rect, W, H, s, threshold, tuple(float(v) for v in z), ignore_root_matrix)
    if key not in _REF:
        cov = gr._ref(impli, oracle, name, shape or SHAPES[name], RECTS[rect], W, H, s, z, ignore_root_matrix)[0]
        _REF[key] = np_distance.field(cov >= threshold)
    return _REF[key]


def _run(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.layer_distance(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check(impli, got, want_dist, reach2):
    dist, rec, stats = got
    want_rec = np_distance.records(want_dist, reach2)
    rows = np_distance.as_rows(rec)
    assert rec.dtype == impli.DIST_DTYPE and rows.shape == want_rec.shape
    if dist is not None:
        assert dist.dtype == np.int32 and dist.shape == want_dist.shape
        bad = np.argwhere(dist != want_dist)
        assert len(bad) == 0, ("first differing [l, py, px]", bad[:5].tolist(), [int(dist[tuple(b)]) for b in bad[:5]],
                               [int(want_dist[tuple(b)]) for b in bad[:5]], len(bad))
        assert np.array_equal(impli.overhang_mask(dist, reach2).sum(axis=(1, 2)), rows[:, 3])
    bad = np.argwhere((rows != want_rec).any(axis=1))
    assert len(bad) == 0, ("first differing records", bad[:3, 0].tolist(), rows[bad[:3, 0]].tolist(), want_rec[bad[:3, 0]].tolist())
    assert stats[5:] == [int(want_rec[:, 0].sum()), int(want_rec[:, 3].sum()), int((want_rec[:, 1] == NONE).sum())]


# ---- the painted stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach2", [0, 4])
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", sorted(di.PAINTED))
def test_painted_stacks_equal_the_restatement(impli, name, level, reach2):
    bits, want = cd.restated(name)
    node, rect, z = di.painted(bits)
    got = _run(impli, level, node, rect, bits.shape[2], bits.shape[1], z, 1, 1, reach2)
    print(name, level, reach2, "records", np_distance.as_rows(got[1]).tolist(), "stats", got[2])
    _check(impli, got, want, reach2)
    assert np.array_equal(got[0] > 0, bits) and (got[0] != 0).all()


@pytest.mark.parametrize("reach2", di.STAIR_REACH2)
def test_the_staircase_at_every_reach(impli, reach2):
    bits, want = cd.restated("staircase")
    node, rect, z = di.painted(bits)
    _check(impli, _run(impli, 2, node, rect, 40, 40, z, 1, 1, reach2), want, reach2)


def test_the_hole_s_widest_pixel(impli):
    bits, want = cd.restated("one_hole")
    node, rect, z = di.painted(bits)
    dist, rec = impli.layer_distance(node, rect, 70, 70, z)
    assert rec[0].tolist() == (4899, 2896, 4830, 0)
    assert np.array_equal(impli.offset_mask(dist, -2895).reshape(-1).nonzero()[0], [4830]), "eroded to its last pixel"


@pytest.mark.parametrize("H", di.SIZES)
@pytest.mark.parametrize("W", di.SIZES)
def test_tile_edges(impli, W, H):
    bits = di.sized(W, H)
    node, rect, z = di.painted(bits)
    _check(impli, _run(impli, 2, node, rect, W, H, z, 1, 1, 1), np_distance.field(bits), 1)


# ---- the shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", [(1030, 3), (3, 1030)])
def test_wide_and_tall_images(impli, oracle, W, H):
    # wider than the row pass's block of 256 lanes; taller than many batches of the column pass
    z = gr.Z[1:3]
    want = _ref(impli, oracle, "egg", "non_dyadic", W, H, 1, 1, z=z)
    assert (want[0] > 0).any() and (want[0] < 0).any() and (want[1] > 0).any() and (want[1] < 0).any(), "both classes in the reference image"
    for level in (0, 2):
        _check(impli, _run(impli, level, SHAPES["egg"], RECTS["non_dyadic"], W, H, z, 1, 1, 2), want, 2)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("rect", sorted(RECTS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_equal_the_restatement(impli, oracle, name, rect, W, H, s, level):
    for threshold in (1, s * s):
        want = _ref(impli, oracle, name, rect, W, H, s, threshold)
        got = _run(impli, level, SHAPES[name], RECTS[rect], W, H, gr.Z, s, threshold, 2)
        print(name, (W, H, s), rect, level, threshold, "records", np_distance.as_rows(got[1]).tolist(), "stats", got[2])
        _check(impli, got, want, 2)
        assert got[2][4] == 1
        if level == 0:
            assert got[2][1] == got[2][0] and got[2][2] == 0
    # entry 0 of the planes misses every shape: whatever stands on it is unsupported at any reach
    assert got[1]["unsupported"][1] == got[1]["solid"][1] and got[1]["widest"][0] == 0 and got[1]["widest_at"][0] == -1


# ---- chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chunked", "staircase"])
def test_three_and_twelve_chunks_give_the_same(impli, name, monkeypatch):
    bits, want = cd.restated(name)
    node, rect, z = di.painted(bits)
    one = _run(impli, 2, node, rect, 40, 40, z, 1, 1, 1)
    monkeypatch.setenv("IMPLISOLID_DISTANCE_CHUNK", "36")   # four layers of nine raster tiles
    three = _run(impli, 2, node, rect, 40, 40, z, 1, 1, 1)
    monkeypatch.setenv("IMPLISOLID_DISTANCE_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = _run(impli, 0, node, rect, 40, 40, z, 1, 1, 1)
    nodist = _run(impli, 2, node, rect, 40, 40, z, 1, 1, 1, want_dist=False)
    monkeypatch.delenv("IMPLISOLID_DISTANCE_CHUNK")
    assert one[2][4] == 1 and three[2][4] == 3 and each[2][4] == 12 and nodist[2][4] == 12
    for r in (one, three, each, nodist):
        _check(impli, r, want, 1)
        assert np.array_equal(r[1], one[1]) and r[2][5:] == one[2][5:]
    assert np.array_equal(three[0], one[0]) and np.array_equal(each[0], one[0]) and nodist[0] is None


def test_chunks_of_a_shape_give_the_same(impli, oracle, monkeypatch):
    want = _ref(impli, oracle, "tree_deep", "non_dyadic", 40, 40, 2, 2, z=gr.Z12)
    monkeypatch.setenv("IMPLISOLID_DISTANCE_CHUNK", "36")
    got = _run(impli, 2, SHAPES["tree_deep"], RECTS["non_dyadic"], 40, 40, gr.Z12, 2, 2, 3)
    monkeypatch.delenv("IMPLISOLID_DISTANCE_CHUNK")
    assert got[2][4] == 3
    _check(impli, got, want, 3)


# ---- cross-checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [1, 3, 4])
def test_records_agree_with_the_raster_and_the_islands(impli, threshold):
    a = (SHAPES["csg"], RECTS["non_dyadic"], 40, 40, gr.Z, 2)
    dist, rec, stats = impli.layer_distance(*a, threshold, 0, return_stats=True)
    cov, sums, rstats = impli.raster_layers(*a, return_stats=True)
    offs, comps = impli.layer_islands(*a, threshold, 8)
    assert stats[:5] == rstats and np.array_equal(dist > 0, cov >= threshold)
    assert rec["solid"].tolist() == (cov >= threshold).sum(axis=(1, 2)).tolist() and stats[5] == int(rec["solid"].sum()) > 0
    assert rec["unsupported"][0] == 0
    for l in range(1, len(gr.Z)):
        c = comps[offs[l]:offs[l + 1]]
        assert rec["unsupported"][l] == int((c["area"].astype(np.int64) - c["below"]).sum()), l
    assert stats[6] == int(rec["unsupported"].sum()) > 0


def test_without_dist_the_records_are_the_same(impli):
    a = (SHAPES["tree_deep"], RECTS["unit"], 40, 40, gr.Z, 2, 2, 5)
    dist, rec, stats = impli.layer_distance(*a, return_stats=True)
    none, rec2, stats2 = impli.layer_distance(*a, want_dist=False, return_stats=True)
    assert none is None and np.array_equal(rec, rec2) and stats == stats2 and rec["solid"].sum() > 0
    assert len(impli.layer_distance(*a)) == 2


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_a_solid_and_an_empty_stack_are_none_without_a_sample(impli, W, H, s):
    z = gr.Z
    dist, rec, stats = _run(impli, 2, gm.BIG, RECTS["unit"], W, H, z, s, s * s, 7)
    assert (dist == NONE).all() and stats[1] == 0 and stats[3] == 0 and stats[2] == stats[0] and stats[5:] == [len(z) * W * H, 0, len(z)]
    for r in rec:
        assert r.tolist() == (W * H, NONE, 0, 0)
    dist, rec, stats = _run(impli, 2, gm.AWAY, RECTS["unit"], W, H, z, s, 1, 7)
    assert (dist == -NONE).all() and stats[1:4] == [0, 0, 0] and stats[5:] == [0, 0, 0]
    for r in rec:
        assert r.tolist() == (0, 0, -1, 0)


def test_two_calls_give_identical_results(impli):
    a = (SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, gr.Z, 4, 9, 2)
    first = impli.layer_distance(*a, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch
    bits, want = cd.restated("one_hole")
    node, rect, z = di.painted(bits)
    assert impli.layer_distance(node, rect, 70, 70, z)[1]["widest"][0] == 2896
    again = impli.layer_distance(*a, return_stats=True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2] and first[1]["solid"].sum() > 0


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    moved = dict(SHAPES["csg"], matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    ignored = _ref(impli, oracle, "csg_ignored", "unit", 40, 40, 2, 2, shape=moved, ignore_root_matrix=True)
    kept = _ref(impli, oracle, "csg_moved", "unit", 40, 40, 2, 2, shape=moved)
    plain = _ref(impli, oracle, "csg", "unit", 40, 40, 2, 2)
    assert np.array_equal(ignored, plain) and not np.array_equal(kept, plain), "the root matrix moves the solid"
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 2, 2, ignore_root_matrix=True), ignored, 2)
    _check(impli, _run(impli, level, moved, RECTS["unit"], 40, 40, gr.Z, 2, 2, 2), kept, 2)


def test_the_kernel_timer_reports_every_pass(impli):
    impli.layer_distance_kernel_ms(True)
    try:
        impli.layer_distance(SHAPES["csg"], RECTS["unit"], 40, 40, gr.Z, 2, 1, 0)
        ms = impli.layer_distance_kernel_ms(True)
    finally:
        impli.layer_distance_kernel_ms(False)
    print("raster, columns, rows + records ms", ms)
    assert len(ms) == 3 and all(0 < v < 1000 for v in ms)
