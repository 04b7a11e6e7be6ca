"""GPU parity on general node matrices (tests/matrices.py): rotations, shears, permutations with +-0
translations, mirrors, anisotropic and thin scales -- on leaves of all 14 primitive types, on CSG
nodes and nested three deep.  Every float is compared bit for bit with the CPU oracle, which the CPU
suite pins on the same families against the numpy restatement
(test_oracle_matches_numpy_restatement_on_matrix_families).

The scenes of implisolid_amd/scenes.py only hold dyadic scale + translate matrices, whose inverse
and products are exact: a fused or reordered transform row gives the same bits there, not here.
"""
import json

import numpy as np
import pytest

import matrices
from test_gpu_parity import _field, _needed_samples, _ob02_compare, sync_jit  # noqa: F401  (sync_jit: fixture)

pytestmark = pytest.mark.gpu


def _objects():
    """The 8 objects that also get JIT modules (shape and baked): one tree per family -- twists in
    three of them -- and the zero-translation turns over a twist.  The family trees share two tree
    shapes."""
    out = {}
    for k, fam in enumerate(matrices.FAMILIES):
        out[fam] = matrices.family_tree(fam, seed=k, twist=fam in ("rot", "perm", "mirror"))
    out["perm_zero_twist"] = matrices.perm_zero_twist_tree()
    return out


OBJECTS = _objects()
RANDOM_SEEDS = list(range(40, 48))


def _bits_equal_or_both_nan(a, b):
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def _field_is_oracles(b, ref):
    """The slab stores the samples 1 .. res - 2 of every axis (the outermost sealed layer is implied)."""
    inner = np.ascontiguousarray(ref[1:-1, 1:-1, 1:-1])
    return b.shape == inner.shape and _bits_equal_or_both_nan(np.ascontiguousarray(b), inner)


def _points_reference(oracle, shape, pts):
    tree = oracle.mp5_to_nodes(json.dumps(shape))
    return oracle.eval_implicit(tree, pts), oracle.eval_gradient(tree, pts)


def _assert_points(f, g, f_ref, g_ref, what):
    bad = np.flatnonzero(~((f.view(np.uint32) == f_ref.view(np.uint32)) | (np.isnan(f) & np.isnan(f_ref))))
    assert bad.size == 0, (what, bad.size, bad[:10])
    # a gradient at a singular point (an axis, a cone's tip: the +-0 coordinates reach them) is NaN on
    # both sides; every other component bit for bit
    assert _bits_equal_or_both_nan(g, g_ref), (what, np.flatnonzero((g != g_ref).any(1) & ~np.isnan(g_ref).any(1))[:10])


# ---- 1. points and gradients ----------------------------------------------------------------------
@pytest.mark.parametrize("family", matrices.FAMILIES)
def test_leaf_points_interpreter_bit_exact(impli, oracle, family):
    """Every primitive type under the family's matrix, through the interpreter: values and
    gradients at 20 000 points that include +-0 coordinates and the k/32 lattice."""
    pts = matrices.lattice_points(20000, 11)
    impli.set_jit(0)
    try:
        for i, kind in enumerate(matrices.LEAF_TYPES):
            for seed in ((i, i + 3) if family == "perm" else (i,)):   # perm: more of the +-0 translation kinds
                shape = matrices.family_leaf(kind, family, seed)
                f_ref, g_ref = _points_reference(oracle, shape, pts)
                with impli.ImplicitService(shape) as svc:
                    f, g = svc.eval(pts, gradient=True)
                _assert_points(f, g, f_ref, g_ref, (kind, family, seed))
    finally:
        impli.set_jit(2)


@pytest.mark.parametrize("module", ["interpreter", "shape", "baked"])
@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_tree_points_bit_exact(impli, oracle, sync_jit, name, module):
    """The family on leaves, CSG nodes and nested (twist trees: the gradient goes through every
    matrix above the screw, and +-0 coordinates reach its atan2f): the interpreter, the shape's point
    module and the baked point module."""
    shape = OBJECTS[name]
    pts = matrices.lattice_points(20000, 12)
    f_ref, g_ref = _points_reference(oracle, shape, pts)
    impli.set_jit(0 if module == "interpreter" else 1)
    impli.set_jit_bake(1 if module == "baked" else 0)
    # the engine keeps an object's modules while the same object is set again: another object in
    # between makes it request this one's point module anew, under the mode set above
    with impli.ImplicitService({"type": "iellipsoid", "matrix": matrices.EYE}):
        pass
    before = impli.jit_stats()
    try:
        with impli.ImplicitService(shape) as svc:
            f, g = svc.eval(pts, gradient=True)
    finally:
        impli.set_jit_bake(2)
    after = impli.jit_stats()
    if module != "interpreter":   # a module that failed to compile would fall back to the interpreter
        assert after["modules"] > 0 and after["compiled"] + after["disk_hits"] > 0, after
    if module == "baked":         # one module per object: this one is new to the process
        assert after["compiled"] + after["disk_hits"] > before["compiled"] + before["disk_hits"], (before, after)
    _assert_points(f, g, f_ref, g_ref, (name, module))


# ---- 2. field -------------------------------------------------------------------------------------
def _check_levels(impli, shape, mc):
    b = _field(impli, shape, mc, 0)
    a = _field(impli, shape, mc, 1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.flatnonzero(a != b)[:10]
    c, cs = _field(impli, shape, mc, 2, signs=True)
    assert np.array_equal(cs.astype(bool), b < 0)
    need = _needed_samples(b)
    assert np.array_equal(c[need].view(np.uint32), b[need].view(np.uint32))
    return b


@pytest.mark.parametrize("family", matrices.FAMILIES)
def test_leaf_fields_pruned_identical(impli, oracle, family):
    """Every primitive type under the family's matrix at R = 24 (interpreter): level 1 equals level
    0, level 2 keeps the signs and the needed samples -- and level 0 is the oracle's field."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0)
    impli.set_jit(0)
    try:
        for i, kind in enumerate(matrices.LEAF_TYPES):
            shape = matrices.family_leaf(kind, family, i)
            b = _check_levels(impli, shape, mc)
            ref = oracle.mc_field(oracle.mp5_to_nodes(json.dumps(shape)), 24, [-1, 1] * 3)
            assert _field_is_oracles(b, ref), kind
    finally:
        impli.set_jit(2)


@pytest.mark.parametrize("R", [24, 32, 37])
@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_tree_fields_interpreter_and_jit_agree(impli, oracle, name, R):
    """R = 24, R = 37 (not a multiple of the 8 x 8 x 2 brick) and the dyadic R = 32, whose sample
    coordinates include exact zeros (the sign of a zero through the rows): pruning levels agree, and the
    interpreter, the JIT shape module and the JIT baked module give the same field, signs and
    brick_stats at levels 1 and 2; the level-0 field is the oracle's."""
    from implisolid_amd import scenes
    shape, mc = OBJECTS[name], scenes.mc_settings(R, 1.0)
    impli.set_jit(0)
    try:
        b = _check_levels(impli, shape, mc)
    finally:
        impli.set_jit(2)
    ref = oracle.mc_field(oracle.mp5_to_nodes(json.dumps(shape)), R, [-1, 1] * 3)
    assert _field_is_oracles(b, ref)
    try:
        for level in (1, 2):
            impli.set_pruning(level)
            out = []
            for mode, bake in ((0, False), (1, False), (1, True)):
                impli.set_jit(mode)
                impli.set_jit_bake(bake)
                s = impli.Slab(shape, mc)
                try:
                    s.eval()
                    assert s.used_jit() == bool(mode)
                    out.append((s.read_field(), s.read_signs(), s.brick_stats()))
                finally:
                    s.close()
            fa, sa, ba = out[0]
            for fb, sb, bb in out[1:]:
                assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), np.flatnonzero(fa != fb)[:10]
                assert np.array_equal(sa, sb)
                assert ba == bb
    finally:
        impli.set_jit(2)
        impli.set_jit_bake(2)
        impli.set_pruning(2)


# ---- 3. marching cubes ----------------------------------------------------------------------------
def _mc_compare(impli, oracle, shape, mc):
    v, f = impli.make_geometry(shape, mc)
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    assert f.shape == fr.shape and v.shape == vr.shape, (f.shape, fr.shape, v.shape, vr.shape)
    assert np.array_equal(f, fr)
    assert np.array_equal(v.view(np.uint32), vr.view(np.uint32)), np.abs(v - vr).max()
    return v, f


@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_family_tree_mc(impli, oracle, name):
    from implisolid_amd import scenes
    v, f = _mc_compare(impli, oracle, OBJECTS[name], scenes.mc_settings(33, 1.0))
    assert len(f) > 200


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_matrix_tree_mc(impli, oracle, seed):
    """Random trees of 3 to 8 leaves that draw a matrix family per node (every other one with a twist)."""
    from implisolid_amd import scenes
    v, f = _mc_compare(impli, oracle, matrices.random_matrix_tree(seed, twist=seed % 2 == 1), scenes.mc_settings(33, 1.0))
    assert len(f) > 100


# ---- 4. the full OB02 loop ------------------------------------------------------------------------
def _ob02_trees():
    rot = matrices.matrix("rot", 3, scale=0.9, reach=0.05)
    tw = matrices.leaf("screw", matrices.leaf_matrix("screw", "rot", 5, size=0.5, reach=0.2))
    ball = matrices.leaf("iellipsoid", matrices.leaf_matrix("iellipsoid", "rot", 6, size=0.4, reach=0.3))
    mixed = {"type": "Union", "matrix": matrices.matrix("perm", 7, reach=0.05), "children": [
        {"type": "Difference", "matrix": matrices._unit_size(matrices.matrix("mirror", 2, scale=1.0, reach=0.05)), "children": [
            matrices.leaf("icylinder", matrices.leaf_matrix("icylinder", "mirror", 8, reach=0.2)),
            matrices.leaf("iellipsoid", matrices.leaf_matrix("iellipsoid", "perm", 10, reach=0.3))]},
        matrices.leaf("itorus", matrices.leaf_matrix("itorus", "mirror", 9, reach=0.3))]}
    return {"rot_union_twist": {"type": "Union", "matrix": matrices._unit_size(rot), "children": [tw, ball]},
            "perm_mirror": mixed}


OB02_TREES = _ob02_trees()


@pytest.mark.parametrize("name", sorted(OB02_TREES))
def test_ob02_full_loop(impli, oracle, name):
    """Resampling, projection and QEM, 2 repeats at R = 24: the gradient through non-diagonal
    matrices drives the normals, the projection directions and the QEM planes."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0, vresampl_iters=1, vresampl_c=0.4, projection=1, qem=1, overall_repeats=2)
    v, vr = _ob02_compare(impli, oracle, OB02_TREES[name], mc)
    assert len(v) > 100 and np.isfinite(vr).all(1).mean() > 0.9
