"""The count kernel (k_mc_count / k_mc_count_s / k_mc_count_b, mc.hip mc_count_body) has a fixed
block size per kernel and collects its marked (unit, chunk) pairs two rounds at a time, in an
order that differs from the earlier kernel's.  Grids where that can go wrong, byte for byte against
the oracle: one chunk against two and two against three, more than 512 items in one group from the
marks, a partial last unit and last group, the halo layer of a second slab, the counters of the
headline, object streams (one large enough for the 128-lane kernel's second step of pairs).  The
layer-straddling cases are plain oracle comparisons at every phase of m mod 4: the kernel does not
rely on how a pair's rows lie in a wave (a quad form of the row sums was measured and dropped).

Not repeated here (they exist and run the same kernel): config 4 at R = 512, nch = 9, whole --
tests/test_gpu_parity.py::test_headline_against_oracle_summary[config4_mc_r512] -- and as eight
balanced slabs -- tests/test_gpu_parity.py::test_config4_slabs_against_summary[512-8-True]."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX = [-1.0, 1.0] * 3
UNIT_ROWS, GROUP_UNITS = 4, 64   # mc_types.hpp kUnitRows, kGroupUnits


def _ellipsoid(sx=1.5, sy=1.3, sz=1.1, t=(0.02, -0.03, 0.01)):
    return {"type": "iellipsoid", "matrix": [sx, 0, 0, t[0], 0, sy, 0, t[1], 0, 0, sz, t[2]]}


def _flat(tilt_deg=0.0, t=(0.01, 0.02, 0.03)):
    """The flattened ellipsoid of tests/test_gpu_cells_pairing.py: radii 0.8, 0.8, 0.1, tilted about x."""
    c, s = math.cos(math.radians(tilt_deg)), math.sin(math.radians(tilt_deg))
    return {"type": "iellipsoid", "matrix": [1.6, 0, 0, t[0], 0, 1.6 * c, -0.2 * s, t[1], 0, 1.6 * s, 0.2 * c, t[2]]}


_REF = {}


def _reference(oracle, shape, R):
    """The oracle's mesh and its non-trivial cells, (layers, m, m) bool in cell order, from its own
    field (the stored samples are 1 .. res - 2 of every axis, the outermost of them sealed); computed
    once per (shape, R) and shared read-only."""
    key = (json.dumps(shape), R)
    if key not in _REF:
        tree = oracle.mp5_to_nodes(json.dumps(shape))
        v, f = oracle.marching_cubes(tree, R, BOX)
        F = np.array(oracle.mc_field(tree, R, BOX)[1:-1, 1:-1, 1:-1])
        F[0] = F[-1] = -1e7
        F[:, 0] = F[:, -1] = -1e7
        F[:, :, 0] = F[:, :, -1] = -1e7
        sg = F < 0
        c = [sg[dz:sg.shape[0] - 1 + dz, dy:sg.shape[1] - 1 + dy, dx:sg.shape[2] - 1 + dx]
             for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        nt = np.logical_or.reduce(c) & ~np.logical_and.reduce(c)
        assert nt.shape == (R + 2,) * 3
        for a in (v, f, nt):
            a.setflags(write=False)
        _REF[key] = (v, f, nt)
    return _REF[key]


def _rows(nt):
    """Non-trivial cells per (cell row, 64-cell chunk), rows padded to whole units: (units, 4, nch)."""
    m = nt.shape[1]
    nch = (m + 63) // 64
    x = np.zeros(nt.shape[:2] + (64 * nch,), np.int64)
    x[:, :, :m] = nt
    per = x.reshape(-1, nch, 64).sum(axis=2)
    per = np.concatenate([per, np.zeros((-per.shape[0] % UNIT_ROWS, nch), np.int64)])
    return per.reshape(-1, UNIT_ROWS, nch)


def _straddling_units(nt):
    """Units holding a non-trivial cell whose rows lie in two cell layers."""
    m = nt.shape[1]
    cells = _rows(nt).sum(axis=(1, 2))
    first = np.arange(len(cells)) * UNIT_ROWS
    last = np.minimum(first + UNIT_ROWS - 1, m * nt.shape[0] - 1)
    return int(((cells > 0) & (first // m != last // m)).sum())


def _stats(impli, slab):
    out = (ctypes.c_int64 * 13)()
    assert impli.lib().implisolid_slab_stats_n(slab.h, out, 13) == 13
    d = slab.stats()
    d.update(small_units=int(out[10]), heavy_parts=int(out[11]), wave_items=int(out[12]))
    return d


def _check_one_slab(impli, shape, mc, ref):
    s = impli.Slab(shape, mc)
    try:
        nv, nf = s.run()
        v, f = s.download(nv, nf)
        st = _stats(impli, s)
    finally:
        s.close()
    assert f.shape == ref[1].shape and np.array_equal(f, ref[1])
    assert np.array_equal(v.view(np.uint32), ref[0].view(np.uint32))
    # the count kernel's own sums against the recount from the oracle's field
    assert st["nonempty_units"] == int((_rows(ref[2]).sum(axis=(1, 2)) > 0).sum())
    assert st["act"] == int(ref[2].sum()) and st["tri"] == len(ref[1]) and st["own"] == len(ref[0])
    return st


@pytest.fixture
def pruning(impli):
    yield impli.set_pruning
    impli.set_pruning(2)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("solid", ["ellipsoid", "flat"])
@pytest.mark.parametrize("R", [13, 14, 15, 16])
def test_layer_wrap_inside_a_quad(impli, oracle, pruning, R, solid, level):
    """m = R + 2 = 15 .. 18 takes every residue mod 4: units holding non-trivial cells straddle cell
    layers at each of the three phases that can (m = 16 is the aligned one: m^2 rows are whole
    units, so none does; it is the control)."""
    from implisolid_amd import scenes
    # (a unit straddles where a layer's last rows meet the next one's first: both solids reach past
    # the box in y, the ellipsoid by its y radius of 1.4, the flat one moved by 0.55)
    shape = _ellipsoid(1.5, 2.8, 1.1) if solid == "ellipsoid" else _flat(25.0, t=(0.01, 0.55, 0.03))
    ref = _reference(oracle, shape, R)
    if (R + 2) % 4 == 0:
        assert _straddling_units(ref[2]) == 0
    else:
        assert _straddling_units(ref[2]) > 0
    pruning(level)
    _check_one_slab(impli, shape, scenes.mc_settings(R, 1.0), ref)


@pytest.mark.parametrize("solid", ["ellipsoid", "flat"])
@pytest.mark.parametrize("R", [62, 63, 126, 127])
def test_chunk_edges(impli, oracle, R, solid):
    """m = 64 / 65: one chunk against two, the second holding one cell; m = 128 / 129: two against
    three (R = 62 also takes the 256-lane kernel of one-chunk rows)."""
    from implisolid_amd import scenes
    # (the ellipsoid reaches the last cells of a row: radii 1.2 past the box, cut by the sealed layer)
    shape = _ellipsoid(2.4, 2.2, 1.1) if solid == "ellipsoid" else _flat(25.0)
    ref = _reference(oracle, shape, R)
    if solid == "ellipsoid":   # a non-trivial cell in the row's last chunk, in its last cell
        assert ref[2][:, :, -1].any()
    _check_one_slab(impli, shape, scenes.mc_settings(R, 1.0), ref)


def _pairs_per_group(nt):
    """(unit, chunk) pairs holding a non-trivial cell, per 64-unit group: every one of them is
    marked (the marks are a superset: the pairs touching an evaluated brick)."""
    pairs = (_rows(nt).sum(axis=1) > 0).sum(axis=1)
    pairs = np.concatenate([pairs, np.zeros(-len(pairs) % GROUP_UNITS, np.int64)])
    return pairs.reshape(-1, GROUP_UNITS).sum(axis=1)


MANY_ITEMS_R = 286


@pytest.mark.parametrize("level", [2, 0])
def test_more_than_512_items_in_one_group(impli, oracle, pruning, level):
    """More than 128 marked (unit, chunk) pairs in one group, so that its 512 lanes take the item
    loop more than once on the list the marks gave (pruning level 2).  The flattened ellipsoid's
    pairs holding a non-trivial cell, recounted from the oracle's field for every R = 127 (the first
    with three chunks per row) .. 291, pass 128 in the fullest group first at R = 286 (nch = 5): 132
    pairs; 127 at R = 284, 121 at R = 285, at most 123 below that.  Every such pair is marked (the
    marks are a superset), so that group has at least 528 items.  Level 0 beside it: no marks, every
    pair of a group a candidate (320 pairs, 1 280 items)."""
    from implisolid_amd import scenes
    shape = _flat(0.0)
    nch = (MANY_ITEMS_R + 2 + 63) // 64
    assert nch >= 3
    ref = _reference(oracle, shape, MANY_ITEMS_R)
    most = int(_pairs_per_group(ref[2]).max())
    print("pairs with non-trivial cells in the fullest group:", most)
    assert most == 132 and most * UNIT_ROWS > 512
    pruning(level)
    _check_one_slab(impli, shape, scenes.mc_settings(MANY_ITEMS_R, 1.0), ref)


def test_partial_last_unit_and_group(impli, oracle):
    """R = 15: 17 x 17 = 289 rows are 72 units and one row, and the second group holds 9 units.  A
    solid covering the whole grid meets the sealed layer everywhere, the last row included."""
    from implisolid_amd import scenes
    R = 15
    rows = (R + 2) ** 2
    units = (rows + UNIT_ROWS - 1) // UNIT_ROWS
    assert rows % UNIT_ROWS != 0 and units % GROUP_UNITS != 0
    shape = _ellipsoid(5.0, 5.0, 5.0)
    ref = _reference(oracle, shape, R)
    assert _rows(ref[2])[units - 1].sum() > 0   # the last, partial unit holds non-trivial cells
    _check_one_slab(impli, shape, scenes.mc_settings(R, 1.0), ref)


@pytest.mark.parametrize("R", [13, 15])
def test_halo_layer_two_slabs(impli, oracle, R):
    """Two Z-slabs: the upper one's first cell layer is a halo (cells below cz_emit: owned vertices
    counted as halo, no triangles), in units that straddle it and the first emitted layer."""
    from implisolid_amd import scenes
    shape, mc = _ellipsoid(), scenes.mc_settings(R, 1.0)
    ref = _reference(oracle, shape, R)
    slabs = [impli.Slab(shape, mc, r, 2) for r in range(2)]
    try:
        counts = []
        for s in slabs:
            s.eval()
            s.count()
            counts.append(s.counts()[:2])
        assert slabs[1].stats()["halo_own"] > 0
        voff = np.concatenate([[0], np.cumsum([c[0] for c in counts])])
        foff = np.concatenate([[0], np.cumsum([c[1] for c in counts])])
        vs, fs = [], []
        for r, s in enumerate(slabs):
            s.set_offsets(int(voff[r]), int(foff[r]))
            s.emit()
            nv, nf, of = s.counts()
            assert not of
            v, f = s.download(nv, nf)
            vs.append(v)
            fs.append(f)
    finally:
        for s in slabs:
            s.close()
    assert np.array_equal(np.concatenate(fs), ref[1])
    assert np.array_equal(np.concatenate(vs).view(np.uint32), ref[0].view(np.uint32))


@pytest.mark.parametrize("R", [512, 256])
def test_headline_counters(impli, R):
    """Config 4: the non-empty units and the vertex pass's wave work items are the committed figures
    of profiles/r13_cells_pairing_hist.json."""
    from implisolid_amd import scenes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hist = json.load(open(os.path.join(root, "profiles", "r13_cells_pairing_hist.json")))
    run = [r for r in hist["runs"] if r["R"] == R]
    assert len(run) == 1
    want = (run[0]["nonempty_units"], run[0]["wave_items_with_pairing"])
    assert want == {512: (11484, 7543), 256: (3011, 1964)}[R]   # the committed figures
    s = impli.Slab(*scenes.config4(R))
    try:
        s.run()
        st = _stats(impli, s)
    finally:
        s.close()
    assert (st["nonempty_units"], st["wave_items"]) == want


@pytest.mark.parametrize("n,R", [(8, 128), (2, 255)])
def test_object_stream_matches_per_object_builds(impli, n, R):
    """Seeded config-5 objects as one merged stream (k_mc_count_b, 128-lane blocks of the same
    body): every object's mesh is its own Slab build's, byte for byte.  Eight at 128^3 (192 pairs a
    group: one step of two rounds); two at 255^3, the smallest R with five chunks per row: 320
    pairs a group, so the 128-lane kernel takes its second step of pairs."""
    from implisolid_amd import scenes
    assert (R == 255) == (GROUP_UNITS * ((R + 2 + 63) // 64) > 2 * 128)
    objs = scenes.config5_objects(n, R)
    shapes, mc = [o[0] for o in objs], objs[0][1]
    with impli.Batch(shapes, mc, n_streams=0) as b:
        assert b.n == n and b.merged
        b.run()
        got = [b.download(i) for i in range(n)]
        assert sum(len(g[1]) for g in got) > 0
    for i, sh in enumerate(shapes):
        s = impli.Slab(sh, mc)
        try:
            nv, nf = s.run()
            v, f = s.download(nv, nf)
        finally:
            s.close()
        assert got[i][1].tobytes() == f.tobytes() and got[i][0].tobytes() == v.tobytes(), i
