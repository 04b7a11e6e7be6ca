"""Rays against a solid (implisolid_raycast) on the GPU.

The reference is tests/np_raycast.py's restatement of the definition on field values that do not come
from the ray kernels: the oracle's (eval_implicit), or ImplicitService.eval / np_sdf3d.evaluate for the
sdf_3d shapes, which the oracle does not have.  hit is an integer and t, f and the normals are floats
the definition fixes bit for bit, whatever the pruning level skips and however the rays are chunked.
The normals' reference is np_normals.normals_ref (the oracle's gradient under the reference's rule) at
ray_points(o, d, t); for the sdf_3d shape it is ImplicitService.normals, implisolid_eval_normals itself.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raycast   # noqa: E402
import np_sdf3d   # noqa: E402
from np_normals import normals_ref, same_bits   # noqa: E402
import test_gpu_mass as gm   # noqa: E402  (its shapes; its tests are not collected from here)

pytestmark = pytest.mark.gpu

EYE = gm.EYE
SHAPES, NAMES = gm.SHAPES, gm.NAMES
BIG, AWAY, SPHERE = gm.BIG, gm.AWAY, gm.SPHERE
f32 = np.float32
T0 = 0.25
N_RAYS = 257          # four blocks of the finish kernel and one ray; 64 blocks of the march kernel and one wave
STEPS = [1, 64, 65, 130]
ROUNDS = [0, 1, 24]

_CACHE = {}


def _field_fn(impli, oracle, name, shape, ignore_root_matrix=False):
    """points -> field values from a source that is not the ray kernels (test_gpu_raster._field's sources)"""
    if name == "sdf3d":
        def fn(pts):
            with impli.ImplicitService(shape) as svc:
                return np.asarray(svc.eval(pts), f32)
        return fn
    if name == "np_sdf3d":
        return lambda pts: np.asarray(np_sdf3d.evaluate(shape, *np.asarray(pts, f32).T), f32)
    tree = oracle.mp5_to_nodes(json.dumps(shape), ignore_root_matrix)
    return lambda pts: np.asarray(oracle.eval_implicit(tree, np.ascontiguousarray(pts, f32)), f32)


def _normals_at(impli, oracle, name, shape, pts, ignore_root_matrix=False):
    if len(pts) == 0:
        return np.zeros((0, 3), f32)
    if name == "sdf3d":
        with impli.ImplicitService(shape) as svc:
            return svc.normals(pts)
    return normals_ref(oracle, oracle.mp5_to_nodes(json.dumps(shape), ignore_root_matrix), pts)[0]


def _inside_point(impli, oracle, name, shape):
    """the deepest point of a 21^3 grid over +-1"""
    g = np.linspace(-1, 1, 21).astype(f32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    F = _field_fn(impli, oracle, name, shape)(pts)
    assert np.nanmax(F) > 0, "the shape holds a grid point"
    return pts[int(np.nanargmax(F))]


def _rays(inside, n=N_RAYS, seed=5):
    """n rays: five fixed by hand first, then seeded ones from the sphere of radius 2 towards points of the
    box, every third of non-unit length"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = rng.uniform(-0.75, 0.75, size=(n, 3))
    target[0::2] = np.asarray(inside, np.float64) + rng.uniform(-0.2, 0.2, size=(len(target[0::2]), 3))   # half of them near the solid
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[0::3] *= 0.5
    d[1::6] *= 1.75
    o, d = o.astype(f32), d.astype(f32)
    p = np.asarray(inside, f32)
    o[0], d[0] = p - f32(T0) * np.array([0, 1, 0], f32), [0, 1, 0]      # starts inside: sample 0 is the inside point
    o[1], d[1] = [p[0], p[1], 3.0], [0, 0, -1]                         # axis-parallel, two zero components; the farthest origin
    o[2], d[2] = p, [0, 0, 0]                                          # all-zero direction, inside: hit 0
    o[3], d[3] = [2, 2, 2], [1, 0, 0]                                  # misses everything
    o[4], d[4] = [1.5, 1.5, 1.5], [0, 0, 0]                            # all-zero direction, outside: a miss
    return o, d


def _case(impli, oracle, name):
    """(o, d, t1, field_fn): the shape's rays, and a t1 just behind the axis ray's entry, so that its first
    solid sample is the last one at every N"""
    key = ("case", name)
    if key not in _CACHE:
        shape = SHAPES[name]
        fn = _field_fn(impli, oracle, name, shape)
        o, d = _rays(_inside_point(impli, oracle, name, shape))
        fine = np_raycast.cast(fn, o[1:2], d[1:2], np_raycast.params(T0, 4.25, 4000), 24)
        assert fine[0][0] >= 1
        _CACHE[key] = (o, d, float(f32(fine[1][0] + 0.004)), fn)
    return _CACHE[key]


def _ref(impli, oracle, name, shape, fn, o, d, t0, t1, N, B, tag="", ignore_root_matrix=False):
    """np_raycast.cast of the independent field, and the normals' reference; the samples once per (case, N)"""
    fkey = ("F", name, tag, N, len(o))
    ts = np_raycast.params(t0, t1, N)
    if fkey not in _CACHE:
        _CACHE[fkey] = np_raycast.sample_field(fn, o, d, ts)
    key = ("ref", name, tag, N, B, len(o))
    if key not in _CACHE:
        hit, t, f = np_raycast.cast(fn, o, d, ts, B, F=_CACHE[fkey])
        nrm = np.zeros((len(o), 3), f32)
        rows = hit >= 0
        nrm[rows] = _normals_at(impli, oracle, name, shape, np_raycast.points(o, d, t)[rows], ignore_root_matrix)
        _CACHE[key] = (hit, t, f, nrm)
    return _CACHE[key]


def _at_level(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.raycast(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check_bits(impli, got, want, o, d, N):
    hit, t, f, nrm, stats = got
    rh, rt, rf, rn = want
    n = len(o)
    assert hit.dtype == np.int32 and hit.shape == (n,) and t.dtype == f.dtype == np.float32 and t.shape == f.shape == (n,)
    bad = np.flatnonzero(hit != rh)
    assert len(bad) == 0, ("first differing rays", bad[:5].tolist(), hit[bad[:5]].tolist(), rh[bad[:5]].tolist())
    assert same_bits(t, rt), np.flatnonzero(t.view(np.uint32) != rt.view(np.uint32))[:5]
    assert same_bits(f, rf), np.flatnonzero(f.view(np.uint32) != rf.view(np.uint32))[:5]
    if nrm is not None:
        assert nrm.shape == (n, 3) and same_bits(nrm, rn), np.flatnonzero((nrm.view(np.uint32) != rn.view(np.uint32)).any(1))[:5]
        assert not nrm[hit < 0].any(), "zero rows on a miss"
        # the hit positions a caller computes are the points the normals were taken at
        assert same_bits(impli.ray_points(o, d, t), np_raycast.points(o, d, rt))
    nseg = (N + 63) // 64
    assert stats[0] == n * nseg and stats[1] + stats[2] <= stats[0]
    assert stats[3] == int((rh >= 0).sum()) and stats[4] == int((rh == 0).sum())


def _level0_segments(rh, N):
    nseg = (N + 63) // 64
    return int(np.where(rh < 0, nseg, np.maximum(rh - 1, 0) // 64 + 1).sum())


def test_the_deep_tree_runs_the_16_slot_stacks(impli):
    assert impli.program_info(SHAPES["tree_deep"])[1] > 12
    assert impli.program_info(SHAPES["csg"])[1] <= 12, "and the others the smaller ones"


@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_rays_equal_the_restatement(impli, oracle, name, N):
    o, d, t1, fn = _case(impli, oracle, name)
    for B in ROUNDS:
        want = _ref(impli, oracle, name, SHAPES[name], fn, o, d, T0, t1, N, B)
        rh = want[0]
        assert (rh >= 1).any() and (rh < 0).any() and rh[0] == 0 and rh[2] == 0 and rh[3] == -1 and rh[4] == -1, \
            "the case holds hits, misses and rays that start inside"
        assert rh[1] == N, "the axis-parallel ray's first solid sample is the last one"
        if B == 24 and N > 1:
            assert (want[1][rh >= 1] < np_raycast.params(T0, t1, N)[rh[rh >= 1]]).any(), "the bisection moves some t"
        for level in (0, 2):
            got = _at_level(impli, level, SHAPES[name], o, d, T0, t1, N, B)
            print(name, N, B, level, "hits", int((rh >= 0).sum()), "stats", got[4])
            _check_bits(impli, got, want, o, d, N)
            assert got[4][5] == 1
            if level == 0:
                assert got[4][1] == 0 and got[4][2] == _level0_segments(rh, N)


def test_hits_on_both_sides_of_the_first_segment_boundary(impli, oracle):
    # N = 64: a hit on the last sample of segment 0; N = 65: on the only sample segment 1 adds
    for name in NAMES:
        o, d, t1, fn = _case(impli, oracle, name)
        assert (_ref(impli, oracle, name, SHAPES[name], fn, o, d, T0, t1, 64, 0)[0] == 64).any()
        assert (_ref(impli, oracle, name, SHAPES[name], fn, o, d, T0, t1, 65, 0)[0] == 65).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ray_counts(impli, oracle, n):
    o, d, t1, fn = _case(impli, oracle, "csg")
    o, d = o[:n], d[:n]
    want = _ref(impli, oracle, "csg", SHAPES["csg"], fn, o, d, T0, t1, 130, 24)
    assert (want[0] >= 0).any()
    for level in (0, 2):
        _check_bits(impli, _at_level(impli, level, SHAPES["csg"], o, d, T0, t1, 130, 24), want, o, d, 130)


# ---- pruning does work ---------------------------------------------------------------------------------------
def test_pruning_skips_segments_on_a_sphere(impli, oracle):
    N = 1024
    fn = _field_fn(impli, oracle, "sphere", SPHERE)
    o, d = _rays([0, 0, 0])
    ts = impli.ray_params(T0, 3.5, N)
    a, b = impli.ray_points(o[5:6], d[5:6], ts[0])[0], impli.ray_points(o[5:6], d[5:6], ts[64])[0]
    box = [min(a[0], b[0]), max(a[0], b[0]), min(a[1], b[1]), max(a[1], b[1]), min(a[2], b[2]), max(a[2], b[2])]
    iv, _ = impli.debug_intervals(SPHERE, [box])
    print("ray 5, segment 0", box, "bound", iv[0].tolist())
    assert iv[0][1] < 0, "the evaluator proves the ray's first segment outside"
    want = _ref(impli, oracle, "sphere", SPHERE, fn, o, d, T0, 3.5, N, 16)
    assert (want[0] >= 1).any() and (want[0] < 0).any()
    got0 = _at_level(impli, 0, SPHERE, o, d, T0, 3.5, N, 16)
    got2 = _at_level(impli, 2, SPHERE, o, d, T0, 3.5, N, 16)
    print("level 0", got0[4], "level 2", got2[4])
    _check_bits(impli, got0, want, o, d, N)
    _check_bits(impli, got2, want, o, d, N)
    assert got0[4][1] == 0 and got0[4][2] == _level0_segments(want[0], N)
    assert got2[4][1] > 0 and got2[4][1] + got2[4][2] == got0[4][2], "every segment up to the hit is skipped or evaluated"
    for k in range(4):
        assert same_bits(got0[k], got2[k])


def test_rays_away_from_the_solid_evaluate_nothing(impli):
    o, d = _rays([0, 0, 0])
    hit, t, f, nrm, stats = impli.raycast(AWAY, o, d, T0, 3.5, 130, 8, return_stats=True)
    print("stats", stats)
    assert (hit == -1).all() and (t == f32(3.5)).all() and not f.any() and not nrm.any()
    assert stats == [N_RAYS * 3, N_RAYS * 3, 0, 0, 0, 1]


def test_inside_everywhere(impli, oracle):
    o, d = _rays([0, 0, 0])
    for level in (0, 2):
        hit, t, f, nrm, stats = _at_level(impli, level, BIG, o, d, 0.0, 3.0, 130, 8)
        assert (hit == 0).all() and (t == 0).all() and stats[3] == stats[4] == N_RAYS and stats[2] == N_RAYS
        F = _field_fn(impli, oracle, "big", BIG)(o)
        assert same_bits(f, F), "the field at the origins"
        assert same_bits(nrm, _normals_at(impli, oracle, "big", BIG, o))


# ---- -0.0 is solid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
def test_negative_zero_samples_are_solid(impli, level):
    # gm.zero_node(): the table's nodes are 32 per axis from -0.96875 in steps of 1/16; its +0.0 entries give
    # -0.0 there.  Rays along the node lines in x: ts[k] = k / 16 exactly, every sample is a node
    node, zeros = gm.zero_node()
    nodes = (f32(-0.96875) + f32(0.0625) * np.arange(32, dtype=f32)).astype(f32)
    zz, yy = np.meshgrid(nodes, nodes, indexing="ij")
    o = np.stack([np.full(1024, nodes[0], f32), yy.reshape(-1), zz.reshape(-1)], -1).astype(f32)
    d = np.tile(np.array([1, 0, 0], f32), (1024, 1))
    ts = np_raycast.params(0, 1.9375, 31)
    assert np.array_equal(ts, np.arange(32, dtype=f32) * f32(0.0625))
    fn = _field_fn(impli, None, "np_sdf3d", node)
    F = np_raycast.sample_field(fn, o, d, ts)                     # [z][y][x], as the table
    assert np.array_equal((F == 0).reshape(32, 32, 32), zeros) and np.signbit(F[F == 0]).all()
    for B in (0, 3):
        rh, rt, rf = np_raycast.cast(fn, o, d, ts, B, F=F)
        on_zero = (rh >= 0) & (F[np.arange(1024), np.maximum(rh, 0)] == 0)
        assert on_zero.sum() >= 100, "many rays hit first on a -0.0 sample"
        hit, t, f, nrm, stats = _at_level(impli, level, node, o, d, 0.0, 1.9375, 31, B, want_normals=False)
        print("level", level, "B", B, "first hits on -0.0", int(on_zero.sum()), "stats", stats)
        assert np.array_equal(hit, rh) and same_bits(t, rt) and same_bits(f, rf)
        if B == 0:
            assert (f[on_zero] == 0).all() and np.signbit(f[on_zero]).all()


# ---- normals = NULL, chunks, reruns, the root matrix -------------------------------------------------------------
def test_without_normals_the_rest_is_the_same(impli, oracle):
    o, d, t1, fn = _case(impli, oracle, "twist")
    want = _ref(impli, oracle, "twist", SHAPES["twist"], fn, o, d, T0, t1, 130, 24)
    got = impli.raycast(SHAPES["twist"], o, d, T0, t1, 130, 24, want_normals=False, return_stats=True)
    assert got[3] is None
    _check_bits(impli, got, want, o, d, 130)
    assert len(impli.raycast(SHAPES["twist"], o, d, T0, t1, 130, 24)) == 4


@pytest.mark.parametrize("name", ["egg", "tree_deep"])
def test_chunks_give_the_same_bits(impli, oracle, name, monkeypatch):
    o, d, t1, fn = _case(impli, oracle, name)
    want = _ref(impli, oracle, name, SHAPES[name], fn, o, d, T0, t1, 130, 24)
    one = impli.raycast(SHAPES[name], o, d, T0, t1, 130, 24, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_RAY_CHUNK", "100")
    three = impli.raycast(SHAPES[name], o, d, T0, t1, 130, 24, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_RAY_CHUNK", "1")
    five = impli.raycast(SHAPES[name], o[:5], d[:5], T0, t1, 130, 24, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_RAY_CHUNK")
    assert one[4][5] == 1 and three[4][5] == 3 and five[4][5] == 5
    _check_bits(impli, one, want, o, d, 130)
    _check_bits(impli, three, want, o, d, 130)
    assert three[4][:5] == one[4][:5]
    for k in range(4):
        assert same_bits(five[k], one[k][:5])


def test_two_calls_give_identical_bits(impli, oracle):
    o, d, t1, _ = _case(impli, oracle, "tree_deep")
    a = impli.raycast(SHAPES["tree_deep"], o, d, T0, t1, 130, 24, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch
    impli.raycast(BIG, o[:70], d[:70], 0.0, 3.0, 65, 3)
    b = impli.raycast(SHAPES["tree_deep"], o, d, T0, t1, 130, 24, return_stats=True)
    assert np.array_equal(a[0], b[0]) and all(same_bits(a[k], b[k]) for k in (1, 2, 3)) and a[4] == b[4]


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    shape = SHAPES["csg"]
    moved = dict(shape, matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    o, d, t1, fn = _case(impli, oracle, "csg")
    t1 = 3.5
    plain = _ref(impli, oracle, "csg", shape, fn, o, d, T0, t1, 130, 8, tag="long")
    want = _ref(impli, oracle, "csg_ignored", moved, _field_fn(impli, oracle, "csg_ignored", moved, True), o, d, T0, t1, 130, 8,
                ignore_root_matrix=True)
    kept = _ref(impli, oracle, "csg_moved", moved, _field_fn(impli, oracle, "csg_moved", moved), o, d, T0, t1, 130, 8)
    assert np.array_equal(want[0], plain[0]) and same_bits(want[1], plain[1]) and not np.array_equal(kept[0], plain[0]), \
        "the root matrix moves the solid"
    _check_bits(impli, _at_level(impli, level, moved, o, d, T0, t1, 130, 8, ignore_root_matrix=True), want, o, d, 130)
    _check_bits(impli, _at_level(impli, level, moved, o, d, T0, t1, 130, 8), kept, o, d, 130)


# ---- views ---------------------------------------------------------------------------------------------------------
def test_render_view(impli):
    W, H, N, B = 33, 17, 100, 16
    view = dict(eye=(0, 0, 2), target=(0, 0, 0), up=(0, 1, 0), width=W, height=H)
    depth, nrm, mask, stats = impli.render_view(SPHERE, t0=0.5, t1=3.0, steps=N, bisect=B, fov_y=0.7, return_stats=True, **view)
    o, d = impli.view_rays(fov_y=0.7, **view)
    hit, t, f, n2 = impli.raycast(SPHERE, o, d, 0.5, 3.0, N, B)
    assert depth.dtype == np.float32 and depth.shape == mask.shape == (H, W) and nrm.shape == (H, W, 3) and mask.dtype == bool
    assert np.array_equal(mask, (hit >= 0).reshape(H, W)) and 0 < mask.sum() < W * H
    assert np.array_equal(np.isnan(depth), ~mask) and same_bits(depth[mask], t.reshape(H, W)[mask])
    assert same_bits(nrm, n2.reshape(H, W, 3)) and stats[3] == mask.sum()
    # the centre ray meets the sphere of radius 1/2 at distance 3/2, from the solid side of the last bracket
    refined = (2.5 / N) * 2.0 ** -B + 8 * np.spacing(f32(3.0))
    c = depth[H // 2, W // 2]
    assert -8 * np.spacing(f32(3.0)) <= c - 1.5 <= refined, c
    assert np.abs(nrm[H // 2, W // 2] - [0, 0, 1]).max() <= 1e-5, "the normal faces the eye"
    od, _, om = impli.render_view(SPHERE, t0=0.5, t1=3.0, steps=N, bisect=B, ortho_height=2.0, **view)
    assert om[H // 2, W // 2] and not om[0, 0] and abs(od[H // 2, W // 2] - 1.5) <= refined


# ---- errors ----------------------------------------------------------------------------------------------------------
O1 = np.array([[0, 0, 2]], f32)
D1 = np.array([[0, 0, -1]], f32)
BAD = [dict(steps=0), dict(steps=65537), dict(bisect=-1), dict(bisect=33), dict(t0=1.0, t1=1.0), dict(t0=2.0, t1=1.0),
       dict(o=[[np.nan, 0, 2]]), dict(d=[[0, np.inf, -1]]), dict(o=[[0, 0, 2], [0, 0, 3]]),
       dict(shape={"type": "rawjscode", "matrix": EYE})]


@pytest.mark.parametrize("kw", BAD)
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.raycast(kw.get("shape", SPHERE), kw.get("o", O1), kw.get("d", D1), kw.get("t0", 0.5), kw.get("t1", 3.0),
                      kw.get("steps", 64), kw.get("bisect", 8))
    assert str(e.value), "with a message"
    assert impli.raycast(SPHERE, O1, D1, 0.5, 3.0, 64, 8)[0][0] >= 1, "and the next call works"


def test_too_many_rays_are_refused_before_an_array_is_read(impli):
    fp = ctypes.POINTER(ctypes.c_float)
    hit, t, f = np.zeros(1, np.int32), np.zeros(1, f32), np.zeros(1, f32)
    rc = impli.lib().implisolid_raycast(json.dumps(SPHERE).encode(), 0, O1.ctypes.data_as(fp), D1.ctypes.data_as(fp), (1 << 24) + 1,
                                        0.5, 3.0, 64, 8, hit.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp),
                                        f.ctypes.data_as(fp), None, None)
    assert rc == -1 and "2^24" in impli.last_error()
    assert impli.raycast(SPHERE, O1, D1, 0.5, 3.0, 64, 8)[0][0] >= 1, "and the next call works"


def test_no_rays_is_not_an_error(impli):
    hit, t, f, nrm, stats = impli.raycast(SPHERE, np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.5, 3.0, 64, 8, return_stats=True)
    assert hit.shape == (0,) and nrm.shape == (0, 3) and stats == [0] * 6
