"""implisolid_slice where tests/test_gpu_slice.py is blind: every marching-squares case (the saddles
and their second segment), a tile loaded to its 512 segments, -0.0 samples, unequal axes, resolutions
at the tile edges, item lists that leave the scan's single-block path, planes of exact zeros and
ignore_root_matrix.

The inputs and references are tests/slice_edge_inputs.py's (np_slice.march of np_sdf3d.evaluate or
oracle field values; tests/test_cpu_slice.py asserts what they hold).  Every comparison is on bits:
the uint32 view of the segments, the keys and all layer offsets, at pruning levels 0 and 2.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_slice   # noqa: E402
import slice_edge_inputs as edges   # noqa: E402
from test_gpu_slice import EGG, SHAPES   # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = [0, 2]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _slice(impli, level, shape, ref, **kw):
    impli.set_pruning(level)
    try:
        return impli.slice_layers(shape, ref.rect, ref.R, ref.z, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _first_difference(got, ref):
    """where the slices part: the layer, tile, cell, case and corner values of the first differing segment"""
    seg, keys, offs = got[:3]
    n = min(len(keys), len(ref.keys))
    bad = np.flatnonzero((keys[:n] != ref.keys[:n]).any(axis=1) | (_u32(seg[:n]) != _u32(ref.seg[:n])).any(axis=(1, 2)))
    if not len(bad):
        return "segments %d against %d; offsets differ at layers %s" % (len(keys), len(ref.keys),
                                                                      np.flatnonzero(offs != ref.offs)[:8].tolist())
    s = int(bad[0])
    l = int(np.searchsorted(ref.offs, s, side="right")) - 1
    W = ref.R + 1
    c = np_slice.cases(ref.F[l])
    # the reference segment's cell: the only one whose edges hold both keys
    k0, k1 = (int(k) for k in ref.keys[s])
    cells = [set((((k // 2) % W) - di, ((k // 2) // W) - dj) for di, dj in ((0, 0), (1, 0) if k % 2 else (0, 1))) for k in (k0, k1)]
    i, j = sorted(cells[0] & cells[1])[0]
    return ("segment %d of %d: layer %d, tile (%d, %d), cell (%d, %d), case %d, corners %s; keys %s want %s, points %s want %s"
            % (s, len(ref.keys), l, i // 16, j // 16, i, j, int(c[j, i]),
               [float(ref.F[l][j, i]), float(ref.F[l][j, i + 1]), float(ref.F[l][j + 1, i + 1]), float(ref.F[l][j + 1, i])],
               keys[s].tolist(), ref.keys[s].tolist(), seg[s].tolist(), ref.seg[s].tolist()))


def _assert_bits(got, ref, what):
    seg, keys, offs, stats = got
    print(what, "segments", len(seg), "stats", stats)
    assert seg.dtype == np.float32 and keys.dtype == np.uint32 and offs.dtype == np.int64
    same = (offs.shape == ref.offs.shape and np.array_equal(offs, ref.offs) and keys.shape == ref.keys.shape and
            np.array_equal(keys, ref.keys) and seg.shape == ref.seg.shape and np.array_equal(_u32(seg), _u32(ref.seg)))
    assert same, "%s: %s" % (what, _first_difference(got, ref))
    assert stats[0] == len(ref.z) * ((ref.R + 15) // 16) ** 2


def _assert_chains(impli, got, ref):
    """test_gpu_slice.test_every_layer_chains_into_polylines, on one result"""
    seg, keys, offs = got[:3]
    for l in range(len(ref.z)):
        k = keys[offs[l]:offs[l + 1]]
        order, lo, closed = impli.slice_loops(k)      # raises on a key that starts or ends two segments
        ro, rf, rc = np_slice.loops(ref.keys[ref.offs[l]:ref.offs[l + 1]])
        assert np.array_equal(ro, order) and np.array_equal(rf, lo) and np.array_equal(rc, closed)
        s = seg[offs[l]:offs[l + 1]]
        for p in range(len(closed)):
            idx = order[lo[p]:lo[p + 1]]
            assert np.array_equal(_u32(s[idx[1:], 0]), _u32(s[idx[:-1], 1])), "chained endpoints are the same bits"


# ---- 1. injected fields ---------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("grid", sorted(edges.INJ_GRIDS))
def test_injected_field_every_case_full_tile_negative_zeros(impli, grid, level):
    ref = edges.injected_ref(grid)
    got = _slice(impli, level, edges.injected_node(), ref)
    _assert_bits(got, ref, "injected %s level %d" % (grid, level))
    stats = got[3]
    if edges.INJ_GRIDS[grid][2]:
        _assert_chains(impli, got, ref)
        assert np.array_equal(_u32(got[0][got[2][1]:got[2][2]]), _u32(got[0][got[2][4]:got[2][5]])), "the repeated plane"
    if level == 0:
        assert stats[1] == stats[0]
    # Level 2 on R = 33: the corner tile (tx = ty = 2, one cell) samples only the quiet quadrant's 0.5,
    # and the issue supposed the bound would drop it (stats[1] < stats[0]).  It does not: measured
    # stats = [45, 45, 6480, 1] at level 2, every tile listed.  The bound covers every table entry a
    # point of the tile's box may read, and the cell at the table's last index (x = y = 1.0625) reads
    # on into the next row and plane, with weight 0 at the samples themselves: mixed signs.  Keeping a
    # tile is always allowed, so only <= is asserted; that pruning drops tiles at all is
    # test_gpu_slice.test_pruning_skips_tiles_on_the_egg's to show, and here the lid's and the long
    # lists' stats do (4 of 12, 1826 of 8400 tiles at level 2).
    assert stats[1] <= stats[0]


# ---- 2. unequal axes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", edges.UNEQUAL_NAMES)
def test_unequal_axes(impli, oracle, name, level):
    ref = edges.unequal_ref(oracle, name)
    _assert_bits(_slice(impli, level, SHAPES[name], ref), ref, "unequal %s level %d" % (name, level))


@pytest.mark.parametrize("level", LEVELS)
def test_far_from_the_origin(impli, oracle, level):
    ref = edges.far_ref(oracle)
    print("equal neighbours in xs", int((np.diff(ref.xs) == 0).sum()), "in ys", int((np.diff(ref.ys) == 0).sum()))
    _assert_bits(_slice(impli, level, edges.FAR_EGG, ref), ref, "far egg level %d" % level)


# ---- 3. resolutions at the tile edges -------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("R", edges.SMALL_RS)
def test_resolutions_at_the_tile_edges(impli, oracle, R, level):
    ref = edges.small_ref(oracle, R)
    got = _slice(impli, level, EGG, ref)
    _assert_bits(got, ref, "R %d level %d" % (R, level))
    assert len(got[0]) > 0 and got[3][0] == len(edges.SMALL_Z) * int(np.ceil(R / 16)) ** 2


# ---- 4. item lists longer than one scan tile ---------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", sorted(edges.LONG))
def test_long_item_lists(impli, oracle, name, level, monkeypatch):
    ref = edges.long_ref(oracle, name)
    monkeypatch.delenv("IMPLISOLID_SLICE_CHUNK", raising=False)
    got = _slice(impli, level, SHAPES[name], ref)
    _assert_bits(got, ref, "long %s level %d" % (name, level))
    assert got[2].shape == (len(ref.z) + 1,) and got[3][3] == 1
    if name != "egg":
        return
    # 4100 items: 1025 layers per chunk -- two chunks of two scan tiles, the second tile four items
    # long, and 50 layers through the single-block scan
    monkeypatch.setenv("IMPLISOLID_SLICE_CHUNK", "4100")
    chunked = _slice(impli, level, SHAPES[name], ref)
    monkeypatch.delenv("IMPLISOLID_SLICE_CHUNK")
    _assert_bits(chunked, ref, "long %s level %d in chunks" % (name, level))
    assert chunked[3][3] == 3 and chunked[3][:3] == got[3][:3]


# ---- 5. planes of exact zeros and ignore_root_matrix -------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_lid_planes_of_exact_zeros(impli, oracle, level):
    ref = edges.lid_ref(oracle, False)
    got = _slice(impli, level, edges.LID, ref)
    _assert_bits(got, ref, "lid level %d" % level)
    _assert_chains(impli, got, ref)


@pytest.mark.parametrize("level", LEVELS)
def test_bare_lid_planes_are_empty(impli, oracle, level):
    ref = edges.lid_ref(oracle, True)
    got = _slice(impli, level, edges.BARE_LID, ref)
    _assert_bits(got, ref, "bare lid level %d" % level)
    offs = got[2]
    assert offs[1] == offs[0] == 0 and offs[3] == offs[2], "every sample of z = +-0.5 is zero: solid, case 15"


@pytest.mark.parametrize("level", LEVELS)
def test_ignore_root_matrix(impli, oracle, level):
    ref = edges.root_ref(oracle, "eye")
    got = _slice(impli, level, edges.MOVED_DIFFERENCE, ref, ignore_root_matrix=True)
    _assert_bits(got, ref, "ignored root matrix level %d" % level)
    moved = edges.root_ref(oracle, "moved")
    kept = _slice(impli, level, edges.MOVED_DIFFERENCE, moved)
    _assert_bits(kept, moved, "kept root matrix level %d" % level)
    assert kept[0].shape != got[0].shape or not np.array_equal(_u32(kept[0]), _u32(got[0]))
