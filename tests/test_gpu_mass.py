"""Mass properties of a solid (implisolid_mass) on the GPU.

The reference is tests/np_mass.py's restatement of the definition on field values that do not come from
the new kernels: the oracle's (eval_implicit) at the sample table's points, or ImplicitService.eval /
np_sdf3d.evaluate for the sdf_3d shapes, which the oracle does not have.  The ten moments and the layer
counts are integers and must equal it exactly, whatever the pruning level skips and however long the
lists are.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_mass   # noqa: E402
import np_sdf3d   # noqa: E402
from implisolid_amd import scenes   # noqa: E402
from test_gpu_slice import DIFFERENCE, EGG   # noqa: E402

pytestmark = pytest.mark.gpu

EYE = scenes.EYE
UNIT = [-1, 1, -1, 1, -1, 1]
NON_DYADIC = [-0.7, 1.3, 0.1, 0.9, -2.1, 0.3]
BOXES = {"unit": UNIT, "non_dyadic": NON_DYADIC}
# radii 1/4, 1/8, 1/2 at (0.25, 0.5, -0.3): inside both boxes
EGG2 = {"type": "iellipsoid", "matrix": [0.5, 0, 0, 0.25, 0, 0.25, 0, 0.5, 0, 0, 1, -0.3]}
SHAPES = {
    "egg": EGG2,
    # a union over a difference: both CSG operators in one tree
    "csg": {"type": "Union", "matrix": EYE, "children": [DIFFERENCE, {"type": "iellipsoid", "matrix": scenes.st(0.5, 0.25, 0.5, -0.5)}]},
    "twist": scenes.twist(0.5, 0.125, 0.5, -0.25),
    "tree_deep": scenes.random_tree(72, 10),   # program depth 13: the interpreter's 16-slot stacks
    "sdf3d": np_sdf3d.node(np_sdf3d.sphere_table(), scenes.st(0.5, 0.125, 0.5, -0.0625)),
}
NAMES = sorted(SHAPES)
SPHERE = {"type": "iellipsoid", "matrix": list(EYE)}                       # radius 0.5 at the origin
BIG = {"type": "iellipsoid", "matrix": scenes.st(20, 0, 0, 0)}             # radius 10: solid throughout +-1
AWAY = {"type": "iellipsoid", "matrix": scenes.st(0.2, 5, 5, 5)}           # radius 0.1 at (5, 5, 5): empty in +-1
OFF_CENTRE = {"type": "iellipsoid", "matrix": scenes.st(1, 0.1, -0.05, 0.2)}

_REF = {}


def _ref(impli, oracle, name, shape, box, depth):
    """np_mass.moments of the independent field values at the sample table; computed once per case"""
    key = (name, tuple(box), depth)
    if key not in _REF:
        pts = np_mass.points(np_mass.mids(box, depth))
        if name == "sdf3d":
            with impli.ImplicitService(shape) as svc:
                F = svc.eval(pts)
        else:
            F = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(shape)), pts)
        N = 1 << depth
        _REF[key] = np_mass.moments(np.asarray(F, np.float32).reshape(N, N, N))
    return _REF[key]


def _at_level(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.mass_moments(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check_bits(got, want):
    mom, layers, stats = got
    m, l = want
    assert mom.dtype == np.uint64 and mom.shape == (10,) and layers.dtype == np.int64 and layers.shape == l.shape
    assert [int(v) for v in mom] == m, ([int(v) for v in mom], m)
    assert np.array_equal(layers, l)
    assert int(layers.sum()) == int(mom[0])


def test_the_deep_tree_runs_the_16_slot_stacks(impli):
    assert impli.program_info(SHAPES["tree_deep"])[1] > 12
    assert impli.program_info(SHAPES["csg"])[1] <= 12, "and the others the 12-slot ones"


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", NAMES)
def test_moments_equal_the_restatement(impli, oracle, name, depth, box, level):
    want = _ref(impli, oracle, name, SHAPES[name], BOXES[box], depth)
    got = _at_level(impli, level, SHAPES[name], BOXES[box], depth)
    print(name, depth, box, level, "moments", [int(v) for v in got[0]], "stats", got[2])
    assert want[0][0] > 0, "the case holds solid cells"
    _check_bits(got, want)
    assert got[2][1] + got[2][2] <= 8 ** depth and got[2][3] == 0
    if level == 0:
        assert got[2][:3] == [0, 0, 8 ** depth]


# ---- -0.0 is solid --------------------------------------------------------------------------------------
ZERO_DEPTH = 5


def zero_node():
    """(an sdf_3d node whose table nodes are the mids of +-1 at depth 5, mask [k][j][i] of its +0.0
    entries): the field there is the entry negated, so those samples are -0.0.  Its properties are
    asserted without a GPU in test_cpu_mass.py."""
    rng = np.random.default_rng(7)
    vals = rng.choice(np.array([-1, -0.5, 0, 0.25, 1], np.float32), size=(32, 32, 32))
    node = np_sdf3d.node(np_sdf3d.Table(vals.reshape(-1), (32, 32, 32), 0.0625, (-0.96875, -0.96875, -0.96875)), EYE)
    return node, vals == 0


@pytest.mark.parametrize("level", [0, 2])
def test_negative_zero_samples_are_solid(impli, level):
    node, zeros = zero_node()
    pts = np_mass.points(np_mass.mids(UNIT, ZERO_DEPTH))
    F = np_sdf3d.evaluate(node, pts[:, 0], pts[:, 1], pts[:, 2]).reshape(32, 32, 32)
    assert np.array_equal(F == 0, zeros) and np.signbit(F[zeros]).all()
    want = np_mass.moments(F)
    got = _at_level(impli, level, node, UNIT, ZERO_DEPTH)
    print("level", level, "n", int(got[0][0]), "of which -0.0", int(zeros.sum()), "stats", got[2])
    _check_bits(got, want)
    assert int(got[0][0]) == int((F > 0).sum() + zeros.sum())


# ---- depths at which the descent starts below level 3 ------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("depth", [3, 4])
def test_small_depths_equal_the_restatement(impli, oracle, depth, level):
    want = _ref(impli, oracle, "sphere", SPHERE, UNIT, depth)
    got = _at_level(impli, level, SPHERE, UNIT, depth)
    print("depth", depth, "level", level, "moments", [int(v) for v in got[0]], "stats", got[2])
    assert want[0][0] > 0
    _check_bits(got, want)
    want = _ref(impli, oracle, "egg", EGG2, NON_DYADIC, depth)
    assert want[0][0] > 0
    _check_bits(_at_level(impli, level, EGG2, NON_DYADIC, depth), want)


# ---- closed forms and 64-bit arithmetic ----------------------------------------------------------------
def test_a_solid_box_at_depth_10_is_counted_in_closed_form(impli):
    N = 1 << 10
    mom, layers, stats = impli.mass_moments(BIG, UNIT, 10, return_stats=True)
    want = np_mass.box_moments(0, N, 0, N, 0, N)
    print("moments", [int(v) for v in mom], "stats", stats)
    assert [int(v) for v in mom] == want and want[4] > 2 ** 48
    assert stats[2] == 0 and stats[1] == 2 ** 30 and stats[0] >= 512
    assert (layers == 2 ** 20).all() and layers.shape == (N,)
    p = impli.mass_properties(BIG, UNIT, 10)
    assert not p["empty"] and abs(p["volume"] - 8.0) <= 1e-12 and np.abs(p["centre"]).max() <= 1e-12
    assert np.abs(p["inertia"] - np.eye(3) * 8.0 * 8.0 / 12.0).max() <= 1e-11 and np.allclose(p["layer_area"], 4.0, rtol=1e-12)


def test_an_empty_box_at_depth_10_gives_zeros(impli):
    fp_ = impli.lib().implisolid_mass
    mom, layers, stats = impli.mass_moments(AWAY, UNIT, 10, return_stats=True)
    assert (mom == 0).all() and (layers == 0).all() and stats[1] == 0 and stats[2] == 0
    import ctypes
    b = np.array(UNIT, np.float32)
    m = np.ones(10, np.uint64)
    rc = fp_(json.dumps(AWAY).encode(), 0, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 10,
             m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None)
    assert rc == 0 and (m == 0).all(), "returns 0; layer_cells and stats may be NULL"
    p = impli.mass_properties(AWAY, UNIT, 10)
    assert p["empty"] and p["volume"] == 0 and (p["centre"] == 0).all() and (p["inertia"] == 0).all() and p["cells"] == 0
    assert (p["layer_area"] == 0).all()


# ---- pruning does work ------------------------------------------------------------------------------------
def test_pruning_counts_solid_boxes_whole_and_drops_outside_ones(impli, oracle):
    # the box corners lie 1.2 radii outside the sphere of radius 0.5 and a central level-3 box lies wholly inside it
    want = _ref(impli, oracle, "sphere", SPHERE, UNIT, 6)
    got0 = _at_level(impli, 0, SPHERE, UNIT, 6)
    got2 = _at_level(impli, 2, SPHERE, UNIT, 6)
    print("level 0", got0[2], "level 2", got2[2])
    _check_bits(got0, want)
    _check_bits(got2, want)
    assert got0[2][2] == 8 ** 6 and got0[2][1] == 0
    assert got2[2][2] < 8 ** 6 and got2[2][1] > 0
    assert got0[2][1] + got0[2][2] <= 8 ** 6 and got2[2][1] + got2[2][2] <= 8 ** 6


# ---- overflow rerun ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["egg", "tree_deep"])
def test_a_short_list_reruns_and_gives_the_same_bits(impli, oracle, name, monkeypatch):
    want = _ref(impli, oracle, name, SHAPES[name], UNIT, 6)
    monkeypatch.setenv("IMPLISOLID_MASS_LIST", "3")
    got = impli.mass_moments(SHAPES[name], UNIT, 6, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_MASS_LIST")
    print(name, "stats", got[2])
    _check_bits(got, want)   # accumulators that are not zeroed before the rerun would count twice
    assert got[2][3] >= 1
    again = impli.mass_moments(SHAPES[name], UNIT, 6, return_stats=True)
    assert again[2][3] == 0 and again[2][1:3] == got[2][1:3]


def test_two_calls_give_identical_integers(impli):
    a = impli.mass_moments(SHAPES["tree_deep"], NON_DYADIC, 6, return_stats=True)
    b = impli.mass_moments(SHAPES["tree_deep"], NON_DYADIC, 6, return_stats=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- sanity against geometry ---------------------------------------------------------------------------------
def test_a_sphere_has_a_sphere_s_volume_centre_and_layer_area(impli):
    r, h = 0.5, 1.0 / 32
    rho = np.sqrt(3.0) * h / 2
    p = impli.mass_properties(OFF_CENTRE, UNIT, 6)
    V = 4.0 / 3.0 * np.pi * r ** 3
    # every cell whose sample can be misclassified lies in the shell r - rho .. r + rho: a derived cap
    cap = 4.0 / 3.0 * np.pi * ((r + rho) ** 3 - (r - rho) ** 3)
    print("volume", p["volume"], "sphere", V, "cap", cap, "centre", p["centre"], "inertia", p["inertia"].tolist())
    assert not p["empty"] and abs(p["volume"] - V) <= cap
    assert p["inertia"].shape == (3, 3) and np.array_equal(p["inertia"], p["inertia"].T)
    assert p["cells"] == int(p["moments"][0]) and p["layer_area"].shape == (64,)
    assert abs(p["layer_area"].sum() * (2.0 / 64) - p["volume"]) <= 1e-12
    k = int(np.floor((0.2 + 1.0) / h))
    mid = float(np_mass.mids(UNIT, 6)[2][k])
    assert mid - h / 2 <= 0.2 < mid + h / 2
    delta = mid - 0.2
    area = np.pi * (r * r - delta * delta)
    print("layer", k, "area", p["layer_area"][k], "disc", area, "bound", 2 * np.pi * r * np.sqrt(2.0) * h)
    assert abs(p["layer_area"][k] - area) <= 2 * np.pi * r * np.sqrt(2.0) * h


# ---- errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(depth=2), dict(depth=11), dict(box=[1, -1, -1, 1, -1, 1]), dict(box=[-1, 1, -1, 1, 0, 0]),
                                dict(box=[-1, np.inf, -1, 1, -1, 1]), dict(shape={"type": "rawjscode", "matrix": EYE})])
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.mass_moments(kw.get("shape", EGG), kw.get("box", UNIT), kw.get("depth", 5))
    assert str(e.value), "with a message"
    if "depth" in kw:   # the C entry refuses it too, before anything is launched
        import ctypes
        b, m = np.array(UNIT, np.float32), np.zeros(10, np.uint64)
        assert impli.lib().implisolid_mass(json.dumps(EGG).encode(), 0, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           kw["depth"], m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None) == -1
        assert impli.last_error()
    assert int(impli.mass_moments(EGG, UNIT, 5)[0][0]) > 0, "and the next call works"
