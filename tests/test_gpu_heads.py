"""The heads of the unit-scan and face kernels (mc.hip unit_scan_body, mc_faces_body): every load is
issued through a clamped index ahead of the value that decides whether it is used -- the units'
entries before the group's non-empty count, the other groups' sums in steps of a uniform trip
count, the lane's first record before the table barrier.  Grids where such a head can go wrong,
byte for byte against the oracle's marching_cubes, with counts() equal to the mesh sizes.

Scan: one group; 65 units (a second group of one unit); every group empty but the last, whose
only non-empty unit is its last one; the flat solid at R = 286 (heavy, light and small units).
A whole grid cannot show the third case: a closed surface's non-trivial cells span two cell
layers, m rows apart, and units of the lower one are never the last.  Slab 0 of a two-slab cut
can: a solid holding the one sample on its top sample layer touches its last cell layer only.

Faces: fewer than 256 records (one partly filled block, 2047 without records); a record count
that is no multiple of the 2048 blocks; no records; the two-slab path with gathered counts.

Refine (brick_modes.hpp brick_refine_item; its head is unchanged in this change, the cases pin
it for the change to come): the JIT module's kernels, unbaked and baked, against the interpreter's
at pruning levels 1 and 2 -- field, sign bitmap, brick classes and brick counts identical -- and
against level 0.  Level 1 prunes CSG operands only, so its field is level 0's bit for bit (the
modes show there: a wrongly pruned operand changes a sample).  Level 2 also leaves sign-filled
bricks unevaluated, so there the sign bitmap and the mesh are level 0's."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX = [-1.0, 1.0] * 3
UNIT_ROWS, GROUP_UNITS = 4, 64   # mc_types.hpp kUnitRows, kGroupUnits
FACE_BLOCKS = 2048               # mc.hip kFacesBlocks


def _ellipsoid(sx=1.5, sy=1.3, sz=1.1, t=(0.02, -0.03, 0.01)):
    return {"type": "iellipsoid", "matrix": [sx, 0, 0, t[0], 0, sy, 0, t[1], 0, 0, sz, t[2]]}


def _flat():
    """The flattened ellipsoid of tests/test_gpu_count_quads.py: radii 0.8, 0.8, 0.1."""
    return {"type": "iellipsoid", "matrix": [1.6, 0, 0, 0.01, 0, 1.6, 0, 0.02, 0, 0, 0.2, 0.03]}


def _one_sample(R, sx, sy, sz):
    """A ball of radius 0.4 spacings about stored sample (sx, sy, sz) (the grid's sample s lies at
    -1 + (s - 1) 2 / R): the only sample inside it."""
    w = 2.0 / R
    return _ellipsoid(0.8 * w, 0.8 * w, 0.8 * w, t=tuple(-1.0 + (s - 1) * w for s in (sx, sy, sz)))


_REF = {}


def _reference(oracle, shape, R):
    """The oracle's mesh and its non-trivial cells, (layers, m, m) bool in cell order, from its own
    field (the outermost stored samples sealed); once per (shape, R), shared read-only."""
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


def _unit_cells(nt):
    """Non-trivial cells per unit of the cell layers given."""
    per = nt.reshape(-1, nt.shape[2]).sum(axis=1)
    per = np.concatenate([per, np.zeros(-len(per) % UNIT_ROWS, np.int64)])
    return per.reshape(-1, UNIT_ROWS).sum(axis=1)


def _check(impli, shape, R, ref, cuts=None):
    """The slabs of `cuts` (None: the whole grid), each through eval, count, host offsets and emit:
    the concatenated mesh is the oracle's and every counts() is its slab's mesh size.  Returns each
    slab's statistics."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(R, 1.0)
    n = 1 if cuts is None else len(cuts) - 1
    slabs = [impli.Slab(shape, mc, r, n, cuts) if cuts is not None else impli.Slab(shape, mc) for r in range(n)]
    try:
        counts, stats = [], []
        for s in slabs:
            s.eval()
            s.count()
            counts.append(s.counts()[:2])
            stats.append(s.stats())
        voff = np.concatenate([[0], np.cumsum([c[0] for c in counts])])
        foff = np.concatenate([[0], np.cumsum([c[1] for c in counts])])
        vs, fs = [], []
        for r, s in enumerate(slabs):
            s.set_offsets(int(voff[r]), int(foff[r]))
            s.emit()
            nv, nf, of = s.counts()
            assert not of and (nv, nf) == counts[r]
            v, f = s.download(nv, nf)
            assert v.shape == (nv, 3) and f.shape == (nf, 3)
            vs.append(v)
            fs.append(f)
    finally:
        for s in slabs:
            s.close()
    v, f = np.concatenate(vs), np.concatenate(fs)
    assert f.shape == ref[1].shape and f.tobytes() == ref[1].tobytes()
    assert v.shape == ref[0].shape and v.tobytes() == ref[0].tobytes()
    return stats


# ---- unit scan ----------------------------------------------------------------------------------

def test_scan_one_group(impli, oracle):
    """R = 14: 16 x 16 rows are 64 units, one group: no other group's sums to add, and the group is
    the last one, which writes the totals."""
    R = 14
    assert (R + 2) ** 2 == UNIT_ROWS * GROUP_UNITS
    shape = _ellipsoid()
    st = _check(impli, shape, R, _reference(oracle, shape, R))
    assert st[0]["units"] == GROUP_UNITS and st[0]["nonempty_units"] > 1


SLAB_R, SLAB_CUTS = 18, [1, 14, 21]   # cell layers from 1; slab 0: 13 layers of 20 rows = 260 rows = 65 units
SLAB_LAYERS = SLAB_CUTS[1] - SLAB_CUTS[0]


def test_scan_second_group_of_one_unit(impli, oracle):
    """65 units: the second group, the last, holds one unit, and both groups hold non-empty ones."""
    m = SLAB_R + 2
    assert m * SLAB_LAYERS == UNIT_ROWS * (GROUP_UNITS + 1) and SLAB_CUTS[2] == m + 1
    shape = _ellipsoid(5.0, 5.0, 5.0)   # covers the grid: every boundary cell is non-trivial
    ref = _reference(oracle, shape, SLAB_R)
    cells = _unit_cells(ref[2][:SLAB_LAYERS])
    assert len(cells) == GROUP_UNITS + 1 and cells[-1] > 0 and (cells[:GROUP_UNITS] > 0).sum() > 1
    st = _check(impli, shape, SLAB_R, ref, SLAB_CUTS)
    assert st[0]["units"] == GROUP_UNITS + 1 and st[0]["nonempty_units"] == int((cells > 0).sum())


def test_scan_only_the_last_unit_of_the_last_group(impli, oracle):
    """Slab 0 of the same cut: the one sample inside the solid lies on the slab's top sample layer,
    two rows from the end, so of its 65 units only the last -- the one unit of the last group --
    holds non-trivial cells: the first group is empty and the last group's bases are all zero."""
    k = SLAB_LAYERS
    shape = _one_sample(SLAB_R, 9, SLAB_R, k)
    ref = _reference(oracle, shape, SLAB_R)
    assert len(ref[1]) == 8   # an octahedron about the sample
    cells = _unit_cells(ref[2][:k])
    assert len(cells) == GROUP_UNITS + 1 and cells[-1] > 0 and not cells[:-1].any()
    st = _check(impli, shape, SLAB_R, ref, SLAB_CUTS)
    assert st[0]["nonempty_units"] == 1 and st[0]["act"] == int(cells[-1])


def test_scan_heavy_light_and_small_units(impli, oracle):
    """The flat solid at R = 286 (tests/test_gpu_count_quads.py): 324 groups, so the last ones add
    their sums over more than one 256-lane round, and heavy, light and small units together."""
    R = 286
    shape = _flat()
    ref = _reference(oracle, shape, R)
    cells = _unit_cells(ref[2])
    assert len(cells) > 256 * GROUP_UNITS and (cells > 64).any() and ((cells > 0) & (cells <= 32)).any()
    _check(impli, shape, R, ref)


# ---- faces --------------------------------------------------------------------------------------

def test_faces_fewer_than_256_records(impli, oracle):
    """One partly filled block (one record a block while there are fewer than 2048), the others empty."""
    R = 14
    shape = _ellipsoid(0.5, 0.5, 0.5)
    ref = _reference(oracle, shape, R)
    act = int(ref[2].sum())
    assert 0 < act < 256
    st = _check(impli, shape, R, ref)
    assert st[0]["act"] == act


def test_faces_record_count_not_a_multiple_of_the_blocks(impli, oracle):
    """More than 2048 records and no multiple of it: blocks of ceil(n / 2048) records, the last
    ones short or empty."""
    R = 62
    shape = _ellipsoid()
    ref = _reference(oracle, shape, R)
    act = int(ref[2].sum())
    per = -(-act // FACE_BLOCKS)
    assert act > FACE_BLOCKS and act % FACE_BLOCKS != 0 and per * (FACE_BLOCKS - 1) >= act   # an empty last block
    st = _check(impli, shape, R, ref)
    assert st[0]["act"] == act


def test_faces_zero_records(impli, oracle):
    """A sphere far outside the box: no record, every block's first load clamped away from the
    (empty) record buffer."""
    R = 14
    shape = _ellipsoid(0.5, 0.5, 0.5, t=(40.0, 40.0, 40.0))
    ref = _reference(oracle, shape, R)
    assert len(ref[1]) == 0 and not ref[2].any()
    st = _check(impli, shape, R, ref)
    assert st[0]["act"] == 0 and st[0]["nonempty_units"] == 0


def test_faces_two_slabs_gathered_counts(impli, oracle):
    """emit_faces with the slabs' gathered counts: rank 1 takes its vertex offset from rank 0's row."""
    import torch
    from implisolid_amd import scenes
    R = 13
    shape, mc = _ellipsoid(), scenes.mc_settings(R, 1.0)
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
        assert slabs[1].stats()["halo_own"] > 0
        vs, fs = [], []
        for r, s in enumerate(slabs):
            s.emit_verts()
            s.emit_faces(0, gath.data_ptr(), r)
            nv, nf, of = s.counts()
            assert not of
            v, f = s.download(nv, nf)
            vs.append(v)
            fs.append(f)
    finally:
        for s in slabs:
            s.close()
    assert np.concatenate(fs).tobytes() == ref[1].tobytes()
    assert np.concatenate(vs).tobytes() == ref[0].tobytes()


# ---- refine -------------------------------------------------------------------------------------

BRICK_Z, COARSE_Z = 2, 8   # grid.hpp kBZ, kCZ: a coarse box is 8 bricks of 2 sample layers


def _far_sphere():
    return _ellipsoid(0.5, 0.5, 0.5, t=(40.0, 40.0, 40.0))


def _refine_cases():
    from implisolid_amd import scenes
    tree = scenes.config3()[0]
    return {
        # 18 stored samples per axis: partial bricks in x / y, one coarse box and one brick of a second in z
        "mixed_box_r15": (tree, 15, None),
        # 20 sample layers: 10 bricks, the last coarse box holds 2 of its 8
        "short_last_box_r17": (tree, 17, None),
        # cells [1, 9): 9 sample layers, the last brick holds one; the upper slab's 11 layers too
        "one_layer_last_brick": (tree, 15, [1, 9, 18]),
        "empty_list": (_far_sphere(), 15, None),
    }


_LEVEL0 = {}


def _eval_state(impli, shape, R, cuts, pruned=True):
    """Per slab of the cut: field, signs, the mesh and, of a pruned eval, brick classes (fill bits
    0-1), brick counts and mixed coarse boxes, under the settings in force."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(R, 1.0)
    n = 1 if cuts is None else len(cuts) - 1
    out = []
    for r in range(n):
        s = impli.Slab(shape, mc, r, n, cuts) if cuts is not None else impli.Slab(shape, mc)
        try:
            nv, nf = s.run()
            used = s.used_jit()
            v, f = s.download(nv, nf)
            d = dict(field=s.read_field(), signs=s.read_signs(), mesh=(v.tobytes(), f.tobytes()), used_jit=used)
            d["layers"] = d["signs"].shape[0]
            if pruned:
                d.update(cls=s.read_fill() & 3, bricks=s.brick_stats(), mixed=s.stats()["mixed_coarse_boxes"])
            out.append(d)
        finally:
            s.close()
    return out


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case", ["mixed_box_r15", "short_last_box_r17", "one_layer_last_brick", "empty_list"])
def test_refine_jit_matches_interpreter_and_level0(impli, case, level):
    shape, R, cuts = _refine_cases()[case]
    try:
        if case not in _LEVEL0:
            impli.set_pruning(0)
            _LEVEL0[case] = _eval_state(impli, shape, R, cuts, pruned=False)
        ref0 = _LEVEL0[case]
        impli.set_pruning(level)
        runs = []
        for mode, bake in ((0, False), (1, False), (1, True)):
            impli.set_jit(mode)
            impli.set_jit_bake(bake)
            runs.append(_eval_state(impli, shape, R, cuts))
            assert all(x["used_jit"] == bool(mode) for x in runs[-1])
    finally:
        impli.set_jit(2)
        impli.set_jit_bake(2)
        impli.set_pruning(2)
    interp = runs[0]
    # the case is what it says
    if case == "empty_list":
        assert all(x["mixed"] == 0 for x in interp) and all(len(x["mesh"][1]) == 0 for x in interp)
    else:
        assert all(x["mixed"] >= 1 for x in interp)
    if case == "short_last_box_r17":
        bricks = -(-interp[0]["layers"] // BRICK_Z)
        assert 0 < bricks % COARSE_Z < COARSE_Z
    if case == "one_layer_last_brick":
        assert all(x["layers"] % BRICK_Z == 1 for x in interp)
    for other in runs[1:]:
        for a, b in zip(interp, other):
            assert np.array_equal(a["field"].view(np.uint32), b["field"].view(np.uint32))
            assert np.array_equal(a["signs"], b["signs"])
            assert np.array_equal(a["cls"], b["cls"])
            assert a["bricks"] == b["bricks"] and a["mixed"] == b["mixed"]
    for run in runs:
        for a, z in zip(run, ref0):
            if level == 1:
                assert np.array_equal(a["field"].view(np.uint32), z["field"].view(np.uint32))
            assert np.array_equal(a["signs"], z["signs"])
            assert a["mesh"] == z["mesh"]
