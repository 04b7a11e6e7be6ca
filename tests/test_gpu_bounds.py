"""The bounds of a solid (implisolid_bounds) and the "fit_box" settings key, on the GPU.

The reference is tests/np_bounds.py's plain descent, driven level by level through the interval
probe (debug_intervals, variant 0: the interpreter) with no skipping; the bounds pass must return its
result bit for bit, whatever it skips and however often its lists overflow.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_bounds   # noqa: E402
import np_sdf3d    # noqa: E402
from conftest import mesh_edges   # noqa: E402
from implisolid_amd import scenes   # noqa: E402

pytestmark = pytest.mark.gpu

S = np.array([-1, 1, -1, 1, -1, 1], np.float32)
EYE = scenes.EYE
EGG = {"type": "iellipsoid", "matrix": [0.5, 0, 0, 0.25, 0, 0.25, 0, -0.125, 0, 0, 1, 0.1875]}   # radii 1/4, 1/8, 1/2
# the subtracted ball reaches x = 1, far past what is left of the first one
DIFFERENCE = {"type": "Difference", "matrix": EYE, "children": [
    {"type": "iellipsoid", "matrix": scenes.st(1, -0.125, 0, 0.0625)},
    {"type": "iellipsoid", "matrix": scenes.st(1, 0.5, 0.125, 0)}]}
SHAPES = {
    "egg": EGG,
    "config2": scenes.union_sphere_cube(),
    "difference": DIFFERENCE,
    "twist": scenes.twist(0.5, 0.125, -0.25, 0.0625),
    "sdf3d": np_sdf3d.node(np_sdf3d.sphere_table(), scenes.st(0.5, 0.125, -0.0625, 0.25)),
    # 10 leaves: program depth 6 runs the interpreter's 12-slot stacks, depth 13 its 16-slot ones
    "tree_shallow": scenes.random_tree(16, 10),
    "tree_deep": scenes.random_tree(72, 10),
    "tree_twist": scenes.random_tree(3, 10, twist_leaves=True),
}
# the sphere of radius 0.2 at (0.3, 0.1, -0.2)
SPHERE_C, SPHERE_R = np.array([0.3, 0.1, -0.2]), 0.2
SPHERE = {"type": "iellipsoid", "matrix": scenes.st(0.4, *SPHERE_C)}
# cells of level 6 between the sphere's true extent and its bounds: what the plain descent over the
# interval probe gives on this input (1: the cell the surface ends in), plus one cell of margin
SPHERE_K = 2

_REF = {}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(impli, name, depth, shape=None, search=S):
    key = (name, depth, tuple(float(x) for x in search))
    if key not in _REF:
        _REF[key] = np_bounds.descent(impli, shape if shape is not None else SHAPES[name], search, depth)
    return _REF[key]


def test_stack_classes_of_the_trees(impli):
    assert impli.program_info(SHAPES["tree_shallow"])[1] <= 12 < impli.program_info(SHAPES["tree_deep"])[1]


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bounds_equal_the_plain_descent(impli, name, depth):
    found_r, box_r, info = _ref(impli, name, depth)
    found, box, stats = impli.bounds(SHAPES[name], S, depth)
    print(name, depth, box, stats, info)
    assert found and found_r
    assert np.array_equal(_u32(box), _u32(box_r)), (box, box_r)
    assert stats[3] == 0 and stats[0] + stats[1] <= info["evaluated"]
    assert stats[2] <= max(info["listed"][:-1])
    assert (box[0::2] < box[1::2]).all() and (box[0::2] >= S[0::2]).all() and (box[1::2] <= S[1::2]).all()


def test_difference_bounds_ignore_what_was_removed(impli):
    _, box, _ = impli.bounds(DIFFERENCE, S, 6)
    # the first ball spans x in [-0.625, 0.375]; the second one (to x = 1) only removes
    assert box[1] <= 0.375 + 2 / 32 and box[0] <= -0.625


@pytest.mark.parametrize("name", ["egg", "config2", "tree_deep", "sdf3d"])
def test_short_lists_rerun_to_the_same_bounds(impli, name, monkeypatch):
    _, box_r, _ = _ref(impli, name, 6)
    monkeypatch.setenv("IMPLISOLID_BOUNDS_LIST", "64")
    found, box, stats = impli.bounds(SHAPES[name], S, 6)
    monkeypatch.delenv("IMPLISOLID_BOUNDS_LIST")
    print(name, stats)
    assert found and np.array_equal(_u32(box), _u32(box_r))
    assert stats[3] > 0, "a 64-box list must overflow and rerun"
    assert name != "egg" or stats[1] > 0, "the shortcut is exercised on the rerun path too"
    found2, box2, stats2 = impli.bounds(SHAPES[name], S, 6)
    assert found2 and np.array_equal(_u32(box2), _u32(box_r)) and stats2[3] == 0


def test_the_shortcut_skips_boxes_on_the_egg(impli):
    # (at depth 5 the egg, 1/8 thin in y, has no solid box above the last level: nothing to skip by)
    _, box_r, info = _ref(impli, "egg", 6)
    _, box, stats = impli.bounds(EGG, S, 6)
    assert np.array_equal(_u32(box), _u32(box_r))
    assert stats[1] > 0, "boxes inside the running bounds are skipped"
    assert stats[0] < info["evaluated"], "and their descendants are never bounded"


def _points_outside(box, n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(S[0::2], S[1::2], size=(64 * n, 3)).astype(np.float32)
    out = ((p < box[0::2]) | (p > box[1::2])).any(axis=1)
    return p[out][:n]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bounds_hold_the_solid(impli, oracle, name):
    shape = SHAPES[name]
    _, box, _ = impli.bounds(shape, S, 6)
    v, f = impli.make_geometry(shape, scenes.mc_settings(32, 1.0))
    assert len(v) > 0
    # a side that is the search box's own wall is where seal_exterior closes the surface: its
    # vertices sit on the wall up to the interpolation's rounding
    tol = np.where(box == S, np.float32(1e-6), np.float32(0))
    assert (v >= box[0::2] - tol[0::2]).all() and (v <= box[1::2] + tol[1::2]).all()
    pts = _points_outside(box, 20000, 7)
    if name == "sdf3d":
        fv = np_sdf3d.evaluate(shape, pts[:, 0], pts[:, 1], pts[:, 2])
    else:
        fv = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(shape)), pts)
    print(name, box, len(pts), "points outside the bounds")
    assert len(pts) == 0 or (fv < 0).all(), "a point outside the bounds is outside the solid"


def test_bounds_are_tight_on_a_sphere(impli):
    depth, cell = 6, 2.0 / 64
    lo_t, hi_t = SPHERE_C - SPHERE_R, SPHERE_C + SPHERE_R
    _, box_r, _ = _ref(impli, "sphere", depth, SPHERE)
    k_ref = max(np.ceil((lo_t - box_r[0::2].astype(np.float64)) / cell).max(),
                np.ceil((box_r[1::2].astype(np.float64) - hi_t) / cell).max())
    print("cells between the true extent and the plain descent's bounds:", k_ref)
    assert k_ref + 1 == SPHERE_K
    found, box, _ = impli.bounds(SPHERE, S, depth)
    assert found and np.array_equal(_u32(box), _u32(box_r))
    lo, hi = box[0::2].astype(np.float64), box[1::2].astype(np.float64)
    assert (lo <= lo_t).all() and (hi >= hi_t).all(), "each bound is outside the true extent"
    assert (lo_t - lo <= SPHERE_K * cell).all() and (hi - hi_t <= SPHERE_K * cell).all()


def test_empty_and_unbounded(impli):
    away = np.array([2, 3, 2, 3, 2, 3], np.float32)
    found, box, stats = impli.bounds(EGG, away, 5)
    assert not found and np.array_equal(_u32(box), _u32(away)) and stats[0] >= 512
    found_r, box_r, _ = _ref(impli, "egg_away", 5, EGG, away)
    assert not found_r and np.array_equal(_u32(box_r), _u32(away))
    plane = {"type": "half_plane", "matrix": EYE, "plane_vector": [0, 0, 1], "plane_point": [0, 0, 0.25]}
    found, box, _ = impli.bounds(plane, S, 5)
    _, box_r, _ = _ref(impli, "plane", 5, plane)
    assert found and np.array_equal(_u32(box), _u32(box_r))
    assert np.array_equal(box[:4], S[:4]), "the search box on the axes where the half space is unbounded"
    assert (box[4] == S[4]) != (box[5] == S[5]), "and on its open side of the plane, not the other"


@pytest.mark.parametrize("kw", [dict(depth=2), dict(depth=11), dict(search=[-1, 1, 1, -1, -1, 1]),
                                dict(search=[-1, np.inf, -1, 1, -1, 1]), dict(search=[-1, 1, np.nan, 1, -1, 1]),
                                dict(shape={"type": "rawjscode", "matrix": EYE})])
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError):
        impli.bounds(kw.get("shape", EGG), kw.get("search", S), kw.get("depth", 5))
    assert impli.bounds(EGG, S, 5)[0], "and the next call works"


# ---- the "fit_box" settings key -------------------------------------------------------------------
BOX_KEYS = ["xmin", "xmax", "ymin", "ymax", "zmin", "zmax"]


def _with_box(mc, box):
    mc = dict(mc)
    mc.pop("fit_box", None)
    mc["box"] = {k: float(x) for k, x in zip(BOX_KEYS, box)}
    return mc


@pytest.fixture(scope="module")
def fitted(impli):
    """The sphere at R = 32: fitted build, the box it used, the unfitted build."""
    mc = scenes.mc_settings(32, 1.0, fit_box={"depth": 6})
    v, f = impli.make_geometry(SPHERE, mc)
    box = impli.last_fit_box()
    v0, f0 = impli.make_geometry(SPHERE, scenes.mc_settings(32, 1.0))
    after = impli.last_fit_box()
    return dict(mc=mc, v=v, f=f, box=box, v0=v0, f0=f0, after=after)


def test_fitted_build_equals_the_explicit_box_build(impli, fitted):
    found, b, _ = impli.bounds(SPHERE, S, 6)
    want = impli.fit_box(S, b, 32, 2)
    assert found and fitted["box"] is not None and np.array_equal(_u32(fitted["box"]), _u32(want))
    assert np.array_equal(_u32(want), _u32(np_bounds.fit_box(S, b, 32, 2)))
    v, f = impli.make_geometry(SPHERE, _with_box(fitted["mc"], want))
    assert impli.last_fit_box() is None
    assert v.tobytes() == fitted["v"].tobytes() and f.tobytes() == fitted["f"].tobytes()
    assert fitted["after"] is None, "a build without the key right after a fitted one reports no fitted box"


def test_fitted_mesh_is_closed_and_finer(fitted):
    _, counts = mesh_edges(fitted["f"])
    assert len(fitted["f"]) > 0 and (counts == 2).all(), "every edge in exactly two faces"
    assert len(fitted["v"]) > 4 * len(fitted["v0"]), (len(fitted["v"]), len(fitted["v0"]))

    def err(v):
        return np.abs(np.linalg.norm(v.astype(np.float64) - SPHERE_C, axis=1) - SPHERE_R).max()
    assert err(fitted["v"]) < err(fitted["v0"])


def test_default_depth_and_an_empty_solid(impli):
    v, f = impli.make_geometry(SPHERE, scenes.mc_settings(32, 1.0, fit_box=True))   # depth ceil(log2(32)) = 5
    _, b, _ = impli.bounds(SPHERE, S, 5)
    assert np.array_equal(_u32(impli.last_fit_box()), _u32(impli.fit_box(S, b, 32, 2)))
    mc = scenes.mc_settings(32, 1.0, fit_box=True)
    mc["box"] = {k: x for k, x in zip(BOX_KEYS, [-1.0, -0.5, -1.0, -0.5, 0.5, 1.0])}   # the sphere is not in it
    v, f = impli.make_geometry(SPHERE, mc)
    assert impli.last_fit_box() is None and len(v) == 0 and len(f) == 0


def test_fitted_build_with_normals_and_the_ob02_loop(impli, fitted):
    mc = scenes.mc_settings(32, 1.0, vresampl_iters=1, vresampl_c=0.4, projection=1, qem=1, overall_repeats=3,
                            fit_box={"depth": 6})
    v, f, n = impli.make_geometry(SPHERE, mc, normals=True)
    assert np.array_equal(_u32(impli.last_fit_box()), _u32(fitted["box"]))
    v2, f2, n2 = impli.make_geometry(SPHERE, _with_box(mc, fitted["box"]), normals=True)
    assert impli.last_fit_box() is None
    assert len(v) == len(fitted["v"]) and v.tobytes() != fitted["v"].tobytes(), "the loop moved the vertices"
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes() and n.tobytes() == n2.tobytes()


def test_fitted_build_over_two_slabs(impli, fitted):
    impli.set_devices([0, 0])
    try:
        v, f = impli.make_geometry(SPHERE, fitted["mc"])
        box = impli.last_fit_box()
    finally:
        impli.set_devices(None)
    assert np.array_equal(_u32(box), _u32(fitted["box"]))
    assert v.tobytes() == fitted["v"].tobytes() and f.tobytes() == fitted["f"].tobytes()
