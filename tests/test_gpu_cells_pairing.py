"""The vertex pass takes small units (at most 32 non-trivial cells) two to a wave, half a wave
each (mc_types.hpp kPairCells).  Small shapes where that can go wrong -- an odd last small unit,
small / light / heavy units side by side, units of exactly 32 and 33 cells, slabs, an object
stream, empty and single-unit grids -- byte for byte against the oracle."""
import ctypes
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _sphere(scale=1.0, t=(0, 0, 0)):
    return {"type": "iellipsoid", "matrix": [scale, 0, 0, t[0], 0, scale, 0, t[1], 0, 0, scale, t[2]]}


def _flat(tilt_deg=0.0, t=(0.01, 0.02, 0.03)):
    """An ellipsoid of radii 0.8, 0.8, 0.1, tilted about x: wide flat faces (whole rows of cells, the
    surface in many cells of a unit) with a thin rim (few cells per unit)."""
    c, s = math.cos(math.radians(tilt_deg)), math.sin(math.radians(tilt_deg))
    return {"type": "iellipsoid", "matrix": [1.6, 0, 0, t[0], 0, 1.6 * c, -0.2 * s, t[1], 0, 1.6 * s, 0.2 * c, t[2]]}


def _stats(impli, slab):
    """Slab.stats() with the figures past its ten: small units, heavy parts, wave work items."""
    out = (ctypes.c_int64 * 13)()
    assert impli.lib().implisolid_slab_stats_n(slab.h, out, 13) == 13
    d = slab.stats()
    d.update(small_units=int(out[10]), heavy_parts=int(out[11]), wave_items=int(out[12]))
    return d


def _unit_cells(slab, R):
    """Non-trivial cells per unit (4 cell rows) of a one-slab grid, from the sign bitmap."""
    sg = slab.read_signs().astype(bool)
    c = [sg[dz:sg.shape[0] - 1 + dz, dy:sg.shape[1] - 1 + dy, dx:sg.shape[2] - 1 + dx]
         for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    nt = np.logical_or.reduce(c) & ~np.logical_and.reduce(c)
    assert nt.shape[1] == R + 2
    per_row = nt.sum(axis=2).reshape(-1)
    per_row = np.concatenate([per_row, np.zeros(-per_row.size % 4, per_row.dtype)])
    return per_row.reshape(-1, 4).sum(axis=1)


def _one_slab(impli, oracle, shape, mc):
    """One-slab mesh checked against the oracle; returns (v, f, stats, cells per unit)."""
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    s = impli.Slab(shape, mc)
    try:
        nv, nf = s.run()
        v, f = s.download(nv, nf)
        st = _stats(impli, s)
        cells = _unit_cells(s, mc["resolution"])
    finally:
        s.close()
    assert f.shape == fr.shape and np.array_equal(f, fr)
    assert np.array_equal(v.view(np.uint32), vr.view(np.uint32))
    ne = cells[cells > 0]
    print("R", mc["resolution"], "stats", st, "units with 1-32 / 33-64 / >64 cells:",
          int((ne <= 32).sum()), int(((ne > 32) & (ne <= 64)).sum()), int((ne > 64).sum()))
    # the counters are consistent: work items = heavy parts + pairs + light parts
    light = st["unit_parts"] - st["heavy_parts"] - st["small_units"]
    assert light >= 0
    assert st["wave_items"] == st["heavy_parts"] + (st["small_units"] + 1) // 2 + light
    assert st["small_units"] <= int((ne <= 32).sum())
    return v, f, st, cells


def test_sphere_small_units_odd_tail(impli, oracle):
    """Spheres at R = 20 and 33: most units hold 1-32 cells; at one of them the small units are an
    odd number, so the last pair has an empty second half."""
    from implisolid_amd import scenes
    small = []
    for R in (20, 33):
        _, _, st, _ = _one_slab(impli, oracle, _sphere(1.2), scenes.mc_settings(R, 1.0))
        assert st["small_units"] > st["nonempty_units"] // 2
        small.append(st["small_units"])
    assert any(k % 2 == 1 for k in small), small


@pytest.mark.parametrize("tilt", [0.0, 25.0])
def test_flat_solid_all_three_classes(impli, oracle, tilt):
    """A flat solid at R = 40: its faces fill whole rows (heavy units), its rim crosses few cells
    (small units), light units (33-64 cells) between them."""
    from implisolid_amd import scenes
    _, _, st, cells = _one_slab(impli, oracle, _flat(tilt), scenes.mc_settings(40, 1.0))
    light = st["unit_parts"] - st["heavy_parts"] - st["small_units"]
    assert st["small_units"] > 0 and light > 0 and st["heavy_parts"] > 0, st


def test_units_of_exactly_32_and_33_cells(impli, oracle):
    """The class boundary at R = 32: units with exactly 32 non-trivial cells (small, half a wave)
    and with exactly 33 (light, a whole wave), over a fixed set of tilts of the flat solid; every
    grid's mesh is checked against the oracle."""
    from implisolid_amd import scenes
    seen = set()
    for tilt in (25.0, 10.0, 40.0, 55.0, 70.0, 17.0, 33.0, 48.0):
        _, _, st, cells = _one_slab(impli, oracle, _flat(tilt), scenes.mc_settings(32, 1.0))
        seen |= set(cells.tolist())
        if 32 in seen and 33 in seen:
            break
    assert 32 in seen and 33 in seen, sorted(seen)


@pytest.mark.parametrize("nranks", [2, 3])
def test_sphere_slabs_match_one_slab(impli, oracle, nranks):
    """Two and three z-slabs of the R = 33 sphere (halo-owned vertices, pairs at a slab's first
    emitted layer): the concatenated mesh is the one-slab mesh."""
    from implisolid_amd import scenes
    shape, mc = _sphere(1.2), scenes.mc_settings(33, 1.0)
    ref_v, ref_f, _, _ = _one_slab(impli, oracle, shape, mc)
    slabs = [impli.Slab(shape, mc, r, nranks) for r in range(nranks)]
    try:
        counts = []
        for s in slabs:
            s.eval()
            s.count()
            counts.append(s.counts()[:2])
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
            assert _stats(impli, s)["small_units"] > 0
    finally:
        for s in slabs:
            s.close()
    assert np.array_equal(np.concatenate(fs), ref_f)
    assert np.array_equal(np.concatenate(vs).view(np.uint32), ref_v.view(np.uint32))


def test_batch_with_an_empty_object(impli, oracle):
    """A 3-object stream at R = 24 (merged launches), the middle object wholly outside the box:
    every object's mesh is its own build's and the oracle's."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0)
    shapes = [_sphere(1.2), _sphere(0.4, (5, 5, 5)), _flat(25.0)]
    with impli.Batch(shapes, mc, n_streams=0) as b:
        assert b.n == 3 and b.merged
        for rep in range(2):
            b.run()
            for i, sh in enumerate(shapes):
                v, f = b.download(i)
                vr, fr = oracle.polygonize(json.dumps(sh), json.dumps(mc))
                assert (len(fr) == 0) == (i == 1)
                assert f.shape == fr.shape and np.array_equal(f, fr), (rep, i)
                assert np.array_equal(v.view(np.uint32), vr.view(np.uint32)), (rep, i)
    for i, sh in enumerate(shapes):
        v1, f1 = impli.make_geometry(sh, mc)
        vr, fr = oracle.polygonize(json.dumps(sh), json.dumps(mc))
        assert np.array_equal(f1, fr) and np.array_equal(v1.view(np.uint32), vr.view(np.uint32)), i


def test_empty_and_single_unit(impli, oracle):
    """No unit at all (a solid outside the box) and a tiny sphere at R = 8."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(8, 1.0)
    s = impli.Slab(_sphere(0.4, (5, 5, 5)), mc)
    try:
        assert s.run() == (0, 0)
        st = _stats(impli, s)
        assert st["nonempty_units"] == 0 and st["small_units"] == 0 and st["wave_items"] == 0
    finally:
        s.close()
    _, f, st, _ = _one_slab(impli, oracle, _sphere(0.3, (0.1, 0.05, 0.0)), mc)
    assert len(f) > 0 and 0 < st["nonempty_units"] <= 4
