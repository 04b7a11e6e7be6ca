"""The head and the issue groups of the vertex pass (mc_device.hpp mc_cells_body, mc_cells_part,
mc_cells_pair, cell_emit; mc.hip k_mc_cells, k_mc_cells_b): the counter words come from one load
ahead of every branch and reach the items as arguments, the case words from a 256-word device
table, the four field samples of a cell are loaded before any is used, and the wave scans are DPP
scans, 64 wide in the part path and 32 wide in the pair path.  The smallest grids where each of
these can go wrong, vertices, faces and counts byte for byte against the oracle's marching_cubes.

The two scans have no entry point of their own: they are pinned through the meshes.  A wrong
64-wide prefix moves the ids of a window's cells (the heavy and light units below), a 32-wide scan
that lets the lower half's sum into the upper half moves the ids of every pair's second unit (the
spheres' small units).

Not covered: more than kChunkMaskBits = 24 chunks per row first happens at R = 1535, a grid of
3.6e9 samples, far from a few seconds."""
import ctypes
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX = [-1.0, 1.0] * 3
UNIT_ROWS = 4   # mc_types.hpp kUnitRows


def _ellipsoid(sx, sy, sz, t=(0.02, -0.03, 0.01)):
    return {"type": "iellipsoid", "matrix": [sx, 0, 0, t[0], 0, sy, 0, t[1], 0, 0, sz, t[2]]}


def _box(a, b, c, t=(0.013, -0.021, 0.017), turn=None):
    """The unit cube scaled to a x b x c, then turned 90 degrees about the axis `turn`, then moved."""
    rows = {None: [[a, 0, 0], [0, b, 0], [0, 0, c]],
            "x": [[a, 0, 0], [0, 0, -c], [0, b, 0]],
            "y": [[0, 0, c], [0, b, 0], [-a, 0, 0]],
            "z": [[0, -b, 0], [a, 0, 0], [0, 0, c]]}[turn]
    return {"type": "cube", "matrix": [v for r, tr in zip(rows, t) for v in r + [tr]]}


_REF = {}


def _reference(oracle, shape, R):
    """The oracle's mesh and the signs of its sealed field, (R + 3)^3 bool; once per (shape, R),
    shared read-only."""
    key = (json.dumps(shape), R)
    if key not in _REF:
        tree = oracle.mp5_to_nodes(json.dumps(shape))
        v, f = oracle.marching_cubes(tree, R, BOX)
        F = np.array(oracle.mc_field(tree, R, BOX)[1:-1, 1:-1, 1:-1])
        F[0] = F[-1] = -1e7
        F[:, 0] = F[:, -1] = -1e7
        F[:, :, 0] = F[:, :, -1] = -1e7
        sg = F < 0
        for a in (v, f, sg):
            a.setflags(write=False)
        _REF[key] = (v, f, sg)
    return _REF[key]


def _corner(sg, dz, dy, dx):
    return sg[dz:sg.shape[0] - 1 + dz, dy:sg.shape[1] - 1 + dy, dx:sg.shape[2] - 1 + dx]


def _unit_cells(sg):
    """Non-trivial cells per unit of a whole grid."""
    c = [_corner(sg, dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    nt = np.logical_or.reduce(c) & ~np.logical_and.reduce(c)
    per = nt.reshape(-1, nt.shape[2]).sum(axis=1)
    per = np.concatenate([per, np.zeros(-len(per) % UNIT_ROWS, np.int64)])
    return per.reshape(-1, UNIT_ROWS).sum(axis=1)


def _stats(impli, slab):
    """Slab.stats() with the figures past its ten: small units, heavy parts, wave work items."""
    out = (ctypes.c_int64 * 13)()
    assert impli.lib().implisolid_slab_stats_n(slab.h, out, 13) == 13
    d = slab.stats()
    d.update(small_units=int(out[10]), heavy_parts=int(out[11]), wave_items=int(out[12]))
    d["light_parts"] = d["unit_parts"] - d["heavy_parts"] - d["small_units"]
    return d


def _slab_mesh(impli, shape, R):
    """One slab through eval, count and emit: vertices, faces, statistics."""
    from implisolid_amd import scenes
    s = impli.Slab(shape, scenes.mc_settings(R, 1.0))
    try:
        s.eval()
        s.count()
        nv, nf = s.counts()[:2]
        s.set_offsets(0, 0)
        s.emit()
        assert s.counts() == (nv, nf, 0)
        v, f = s.download(nv, nf)
        st = _stats(impli, s)
    finally:
        s.close()
    assert v.shape == (nv, 3) and f.shape == (nf, 3)
    assert st["wave_items"] == st["heavy_parts"] + (st["small_units"] + 1) // 2 + st["light_parts"]
    return v, f, st


def _check(impli, oracle, shape, R):
    ref = _reference(oracle, shape, R)
    v, f, st = _slab_mesh(impli, shape, R)
    assert f.shape == ref[1].shape and f.tobytes() == ref[1].tobytes()
    assert v.shape == ref[0].shape and v.tobytes() == ref[0].tobytes()
    return st, ref


def test_empty_grid_runs_the_head_and_writes_nothing(impli, oracle):
    """A solid wholly outside the box: counters[0] == 0, so every block loads the counters and its
    case words, passes the barrier and finds no item."""
    st, ref = _check(impli, oracle, _ellipsoid(0.5, 0.5, 0.5, t=(40.0, 40.0, 40.0)), 16)
    assert len(ref[0]) == 0 and len(ref[1]) == 0
    assert st["wave_items"] == 0 and st["nonempty_units"] == 0


def test_one_small_unit_odd_pair(impli, oracle):
    """Spheres about one cell wide at R = 16, around four stored samples in a row of y: a handful of
    small units and nothing else, and for some of them an odd number, whose last pair's second half
    has no cells and reads the first half's list entry."""
    R, w = 16, 2.0 / 16
    odd = []
    for sy in (5, 6, 7, 8):
        shape = _ellipsoid(0.8 * w, 0.8 * w, 0.8 * w, t=(-1.0 + 8 * w, -1.0 + (sy - 1) * w, -1.0 + 6 * w))
        st, ref = _check(impli, oracle, shape, R)
        assert len(ref[1]) == 8   # an octahedron about the one sample inside
        assert st["heavy_parts"] == 0 and st["light_parts"] == 0 and 0 < st["small_units"] <= 4
        odd.append(st["small_units"] % 2)
    assert any(odd), odd


@pytest.mark.parametrize("turn", [None, "x", "y", "z"])
def test_each_owned_edge_alone(impli, oracle, turn):
    """A box with faces along the axes: the cells on a face normal to x own only the crossing edge
    along x, and so for y and z -- each of cell_emit's three slot branches with the other two slots
    unused, which is where one field load used to sit.  The same box turned a quarter about each
    axis moves every face to other cells."""
    R = 24
    st, ref = _check(impli, oracle, _box(0.9, 0.5, 0.3, turn=turn), R)
    sg = ref[2]
    c7 = _corner(sg, 1, 1, 1)
    e5, e6, e10 = c7 ^ _corner(sg, 1, 0, 1), c7 ^ _corner(sg, 1, 1, 0), c7 ^ _corner(sg, 0, 1, 1)
    assert (e5 & ~e6 & ~e10).any() and (e6 & ~e5 & ~e10).any() and (e10 & ~e5 & ~e6).any()


def test_sealed_border_samples(impli, oracle):
    """A sphere larger than the box: every border cell is non-trivial and takes kSealed for its
    outer samples on x, y and z -- selected after the (unconditional) field loads."""
    st, ref = _check(impli, oracle, _ellipsoid(5.0, 5.0, 5.0), 16)
    assert len(ref[1]) > 0 and st["nonempty_units"] > 0


def _tree():
    from implisolid_amd import scenes
    return scenes.config4()[0]


@pytest.mark.parametrize("solid", ["tree", "slab"])
def test_heavy_light_and_small_units(impli, oracle, solid):
    """Config 4's tree, and a slab thin in z whose faces fill whole rows, at R = 64: units of more
    than 64 and more than 128 cells (several windows, several parts, the win % parts ownership),
    light parts and pairs in one launch."""
    R = 64
    shape = _tree() if solid == "tree" else _box(1.7, 1.5, 0.11, t=(0.013, -0.021, 0.03))
    st, ref = _check(impli, oracle, shape, R)
    cells = _unit_cells(ref[2])
    assert (cells > 64).any() and ((cells > 0) & (cells <= 32)).any()
    assert st["heavy_parts"] > 0 and st["light_parts"] > 0 and st["small_units"] > 1
    if solid == "slab":
        assert (cells > 128).any() and st["unit_parts"] > st["nonempty_units"]


def test_three_chunks_per_row(impli, oracle):
    """A plane-like solid at R = 130: rows of 132 cells, three 64-cell chunks, the last one short."""
    R = 130
    st, ref = _check(impli, oracle, _box(1.9, 1.9, 0.05, t=(0.003, -0.004, 0.011)), R)
    cells = _unit_cells(ref[2])
    assert (R + 2 + 63) // 64 == 3 and (cells > 128).any() and st["heavy_parts"] > 0


def test_halo_two_slabs(impli, oracle):
    """Two z-slabs of one grid on one device, with gathered counts: the upper slab's halo layer owns
    vertices (H = counters[1] > 0), so its ids start below the slab's first and its halo cells
    write id triples only."""
    import torch
    from implisolid_amd import scenes
    R = 21
    shape, mc = _ellipsoid(1.5, 1.3, 1.1), scenes.mc_settings(R, 1.0)
    ref = _reference(oracle, shape, R)
    slabs = [impli.Slab(shape, mc, r, 2) for r in range(2)]
    try:
        gath = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
        for r, s in enumerate(slabs):
            s.eval()
            s.count()
            s.counts()   # sizes the output buffers
            s.copy_counts(gath[r].data_ptr())
        torch.cuda.synchronize()
        assert slabs[1].stats()["halo_own"] > 0 and slabs[0].stats()["halo_own"] == 0
        vs, fs, total = [], [], []
        for r, s in enumerate(slabs):
            s.emit_verts()
            s.emit_faces(0, gath.data_ptr(), r)
            nv, nf, of = s.counts()
            assert not of
            v, f = s.download(nv, nf)
            vs.append(v)
            fs.append(f)
            total.append((nv, nf))
    finally:
        for s in slabs:
            s.close()
    assert tuple(map(sum, zip(*total))) == (len(ref[0]), len(ref[1]))
    assert np.concatenate(fs).tobytes() == ref[1].tobytes()
    assert np.concatenate(vs).tobytes() == ref[0].tobytes()


def test_merged_stream(impli, oracle):
    """k_mc_cells_b: a stream of three objects at R = 32 in merged launches, the middle one wholly
    outside the box; every object's mesh is the oracle's and its own Slab's."""
    from implisolid_amd import scenes
    R = 32
    mc = scenes.mc_settings(R, 1.0)
    shapes = [_ellipsoid(1.5, 1.3, 1.1), _ellipsoid(0.5, 0.5, 0.5, t=(40.0, 40.0, 40.0)),
              _box(1.5, 1.3, 0.2, t=(0.013, -0.021, 0.03))]
    with impli.Batch(shapes, mc, n_streams=0) as b:
        assert b.n == 3 and b.merged
        b.run()
        meshes = [b.download(i) for i in range(3)]
    for i, (sh, (v, f)) in enumerate(zip(shapes, meshes)):
        ref = _reference(oracle, sh, R)
        assert (len(ref[1]) == 0) == (i == 1)
        assert f.shape == ref[1].shape and f.tobytes() == ref[1].tobytes(), i
        assert v.shape == ref[0].shape and v.tobytes() == ref[0].tobytes(), i
        vs, fs, _ = _slab_mesh(impli, sh, R)
        assert f.tobytes() == fs.tobytes() and v.tobytes() == vs.tobytes(), i
