"""Slices of a solid (implisolid_slice) on the GPU.

The reference is tests/np_slice.py's restatement of the definition on field values that do not come
from the slicing kernels: the oracle's (eval_implicit), or ImplicitService.eval for the sdf_3d shape,
which the oracle does not have.  The slices must equal it bit for bit, whatever the pruning level skips
and however the layers are chunked.  R = 40 gives tiles of 16, 16 and 8 cells: a partial tile on both
axes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_sdf3d   # noqa: E402
import np_slice   # noqa: E402
from implisolid_amd import scenes   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT = np.array([-1, 1, -1, 1], np.float32)
R = 40
# an empty plane, a repeated plane, an unsorted order and a plane near the egg's pole (z = 0.6875)
Z = np.array([-0.9, 0.1875, 0.3, 0.1875, 0.6875, 0.95], np.float32)
EYE = scenes.EYE
EGG = {"type": "iellipsoid", "matrix": [0.5, 0, 0, 0.25, 0, 0.25, 0, -0.125, 0, 0, 1, 0.1875]}   # radii 1/4, 1/8, 1/2
DIFFERENCE = {"type": "Difference", "matrix": EYE, "children": [
    {"type": "iellipsoid", "matrix": scenes.st(1, -0.125, 0, 0.0625)},
    {"type": "iellipsoid", "matrix": scenes.st(1, 0.5, 0.125, 0)}]}
SHAPES = {
    "egg": EGG,
    "config2": scenes.union_sphere_cube(),
    "difference": DIFFERENCE,
    "twist": scenes.twist(0.5, 0.125, -0.25, 0.0625),
    "sdf3d": np_sdf3d.node(np_sdf3d.sphere_table(), scenes.st(0.5, 0.125, -0.0625, 0.25)),
    "tree_deep": scenes.random_tree(72, 10),   # program depth 13: the interpreter's 16-slot stacks
}
NAMES = sorted(SHAPES)

_REF, _GPU = {}, {}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(impli, oracle, name):
    """np_slice.march on the independent field values; computed once per shape"""
    if name not in _REF:
        xs, ys = np_slice.coords(RECT, R)
        pts = np_slice.points(xs, ys, Z)
        if name == "sdf3d":
            with impli.ImplicitService(SHAPES[name]) as svc:
                F = svc.eval(pts)
        else:
            F = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(SHAPES[name])), pts)
        F = np.asarray(F, np.float32).reshape(len(Z), R + 1, R + 1)
        _REF[name] = np_slice.march(F, xs, ys)
    return _REF[name]


def _gpu(impli, name):
    """the default call (pruning level 2, one chunk); computed once per shape"""
    if name not in _GPU:
        _GPU[name] = impli.slice_layers(SHAPES[name], RECT, R, Z, return_stats=True)
    return _GPU[name]


def _same(a, b):
    return (a[0].shape == b[0].shape and np.array_equal(_u32(a[0]), _u32(b[0])) and np.array_equal(a[1], b[1]) and
            np.array_equal(a[2], b[2]))


def test_the_deep_tree_runs_the_16_slot_stacks(impli):
    assert impli.program_info(SHAPES["tree_deep"])[1] > 12


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", NAMES)
def test_slices_equal_the_restatement(impli, oracle, name, level):
    seg_r, keys_r, offs_r = _ref(impli, oracle, name)
    impli.set_pruning(level)
    try:
        seg, keys, offs, stats = impli.slice_layers(SHAPES[name], RECT, R, Z, return_stats=True)
    finally:
        impli.set_pruning(2)
    print(name, level, "segments", len(seg), "per layer", np.diff(offs).tolist(), "stats", stats)
    assert seg.dtype == np.float32 and keys.dtype == np.uint32 and offs.dtype == np.int64
    assert seg.shape == (len(seg_r), 2, 2) and keys.shape == (len(keys_r), 2) and offs.shape == (len(Z) + 1,)
    assert np.array_equal(offs, offs_r), (offs, offs_r)
    assert np.array_equal(keys, keys_r)
    assert np.array_equal(_u32(seg), _u32(seg_r))
    assert len(seg) > 0 and stats[0] == len(Z) * 9 and stats[3] == 1
    # the repeated plane repeats its segments
    assert np.array_equal(_u32(seg[offs[1]:offs[2]]), _u32(seg[offs[3]:offs[4]]))


def test_pruning_skips_tiles_on_the_egg(impli):
    # the egg spans x in [0, 0.5], y in [-0.25, 0]: the tile columns x in [-1, -0.2] and [0.6, 1] lie
    # wholly outside it, and the planes z = -0.9 and z = 0.95 miss it
    stats2 = _gpu(impli, "egg")[3]
    impli.set_pruning(0)
    try:
        stats0 = impli.slice_layers(EGG, RECT, R, Z, return_stats=True)[3]
    finally:
        impli.set_pruning(2)
    print("level 2", stats2, "level 0", stats0)
    assert stats2[1] < stats2[0]
    assert stats0[1] == stats0[0] == 54 and stats0[2] == len(Z) * (R + 3) ** 2   # 17 + 17 + 9 samples per axis
    assert stats2[2] < stats0[2]


@pytest.mark.parametrize("name", ["egg", "tree_deep"])
def test_one_layer_per_chunk_gives_the_same_bits(impli, name, monkeypatch):
    want = _gpu(impli, name)
    monkeypatch.setenv("IMPLISOLID_SLICE_CHUNK", "9")   # one layer's tiles
    got = impli.slice_layers(SHAPES[name], RECT, R, Z, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_SLICE_CHUNK")
    assert got[3][3] == 6 and want[3][3] == 1
    assert _same(got, want)
    assert got[3][:3] == want[3][:3]
    monkeypatch.setenv("IMPLISOLID_SLICE_CHUNK", "1")   # below one layer's tiles: still a layer per chunk
    assert impli.slice_layers(SHAPES[name], RECT, R, Z, return_stats=True)[3][3] == 6


@pytest.mark.parametrize("name", NAMES)
def test_every_layer_chains_into_polylines(impli, name):
    seg, keys, offs, _ = _gpu(impli, name)
    for l in range(len(Z)):
        k = keys[offs[l]:offs[l + 1]]
        order, lo, closed = impli.slice_loops(k)      # raises on a key that starts or ends two segments
        assert np.array_equal(np.sort(order), np.arange(len(k))), "every segment is used once"
        assert lo[0] == 0 and lo[-1] == len(k) and len(closed) == len(lo) - 1
        ro, rf, rc = np_slice.loops(k)
        assert np.array_equal(ro, order) and np.array_equal(rf, lo) and np.array_equal(rc, closed)
        s = seg[offs[l]:offs[l + 1]]
        for p in range(len(closed)):
            idx = order[lo[p]:lo[p + 1]]
            assert np.array_equal(_u32(s[idx[1:], 0]), _u32(s[idx[:-1], 1])), "chained endpoints are the same bits"


def test_the_egg_gives_closed_loops_of_the_right_area(impli):
    lines = impli.slice_polylines(EGG, RECT, R, Z)
    # the egg spans z in [-0.3125, 0.6875]: two planes miss it (z = 0.6875 touches its pole: not asserted)
    assert len(lines) == len(Z) and [len(lines[l]) for l in (0, 1, 2, 3, 5)] == [0, 1, 1, 1, 0]
    assert all(closed for layer in lines for _, closed in layer)
    # z = 0.1875 is the egg's centre plane: the ellipse with semi-axes 1/4 and 1/8.  The contour is a
    # polygon with its vertices on the grid lines, h = 0.05 apart, each within the linear interpolation's
    # error of the ellipse: a chord over an arc of curvature radius rho loses about h^2 / (12 rho) of
    # area per unit length, and rho runs from b^2 / a = 1/16 at the ends to a^2 / b = 1/2 on the flat
    # sides, where most of the perimeter lies -- a few per cent for h against the short radius 1/8;
    # the bound is 5 %
    for l in (1, 3):
        pts, closed = lines[l][0]
        area = np_slice.shoelace(pts)
        print("layer", l, "points", len(pts), "area", area, "ellipse", np.pi * 0.25 * 0.125)
        assert closed and area > 0 and abs(area - np.pi * 0.25 * 0.125) <= 0.05 * np.pi * 0.25 * 0.125


@pytest.mark.parametrize("kw", [dict(R=0), dict(R=4097), dict(z=[]), dict(z=[0.0, np.nan]), dict(rect=[1, -1, -1, 1]),
                                dict(shape={"type": "rawjscode", "matrix": EYE})])
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.slice_layers(kw.get("shape", EGG), kw.get("rect", RECT), kw.get("R", R), kw.get("z", Z))
    assert str(e.value), "with a message"
    # a failed call leaves no result behind
    assert impli.lib().implisolid_slice_copy(None, None) == -1 and impli.last_error()
    assert len(impli.slice_layers(EGG, RECT, R, Z)[0]) > 0, "and the next call works"


def test_copy_before_any_slice_is_an_error():
    code = ("import implisolid_amd as I; L = I.lib(); rc = L.implisolid_slice_copy(None, None); "
            "print('rc', rc, 'msg', bool(I.last_error()))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "rc -1 msg True" in out.stdout, (out.stdout, out.stderr)


def test_two_calls_give_identical_bits(impli):
    a = impli.slice_layers(SHAPES["tree_deep"], RECT, R, Z, return_stats=True)
    b = impli.slice_layers(SHAPES["tree_deep"], RECT, R, Z, return_stats=True)
    assert _same(a, b) and a[3] == b[3] and _same(a, _gpu(impli, "tree_deep"))
