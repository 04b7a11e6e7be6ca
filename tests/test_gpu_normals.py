"""GPU: per-vertex normals from the same build (the "normals" settings key, get_n_*,
implisolid_eval_normals, the slab entries) against the reference rule mcc2.cpp:852-871 applied to the
oracle's gradients (np_normals.normals_ref) -- bit for bit, every row, NaN rows by position."""
import ctypes
import json

import numpy as np
import pytest

import matrices
from np_normals import normals_ref, same_bits
from test_gpu_parity import TREES

pytestmark = pytest.mark.gpu


def _general_matrix_tree():
    """A rotated leaf under a sheared CSG node (tests/matrices.py): inexact inverses on both levels."""
    return {"type": "Union", "matrix": matrices._unit_size(matrices.matrix("shear", 3, scale=1.0, reach=0.06)), "children": [
        matrices.family_leaf("itorus", "rot", 5), matrices.family_leaf("iellipsoid", "rot", 6)]}


MC_TREES = {k: TREES[k] for k in ("sphere", "union_sphere_cube", "difference", "intersection", "twist_tbb",
                                  "extrusion_tri", "leaf_itorus")}
MC_TREES["rot_under_shear"] = _general_matrix_tree()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_normals(impli, oracle, tree, v, n):
    ref, bad = normals_ref(oracle, tree, v)
    assert n.shape == v.shape and n.dtype == np.float32
    assert same_bits(n, ref), np.flatnonzero((_u32(n) != _u32(ref)).any(1))[:10]
    assert impli.normals_stats() == (len(v), bad)
    return bad


@pytest.mark.parametrize("name", sorted(MC_TREES))
def test_mc_only_normals(impli, oracle, name):
    from implisolid_amd import scenes
    shape, mc = MC_TREES[name], scenes.mc_settings(24, 1.0)
    before = json.dumps(mc, sort_keys=True)
    v0, f0 = impli.make_geometry(shape, mc)
    v, f, n = impli.make_geometry(shape, mc, normals=True)
    assert json.dumps(mc, sort_keys=True) == before
    assert len(v) % 64 != 0 or len(v) == 0   # (the intersection's surface misses every cell at R = 24: V = 0)
    assert np.array_equal(f, f0) and np.array_equal(_u32(v), _u32(v0))
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape)), v, n)
    # get_n and the get_n_ptr view agree (the views are read before the next build)
    vv, fv, nv = impli.make_geometry_views(shape, mc, normals=True)
    assert impli.views_current(nv) and not nv.flags.writeable
    assert np.array_equal(_u32(nv), _u32(n)) and np.array_equal(_u32(vv), _u32(v)) and np.array_equal(fv, f)
    got = np.empty_like(n)
    L = impli.lib()
    assert L.get_n_size() == len(v)
    L.get_n(got.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(v))
    assert np.array_equal(_u32(got), _u32(n))
    L.finish_geometry()
    impli.make_geometry(shape, mc)
    assert not impli.views_current(nv)


def _config2(R, **kw):
    from implisolid_amd import scenes
    shape, mc = scenes.config2(R)
    assert mc["vresampl"] == {"iters": 1, "c": 0.4} and mc["projection"]["enabled"] and mc["qem"]["enabled"]
    assert mc["overall_repeats"] == 3
    mc.update(kw)
    return shape, mc


@pytest.mark.parametrize("R", [24, 32])
def test_normals_after_the_loop(impli, oracle, R):
    shape, mc = _config2(R)
    v, f, n = impli.make_geometry(shape, mc, normals=True)
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    assert np.array_equal(f, fr) and np.array_equal(_u32(v), _u32(vr))
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape)), v, n)


def test_normals_after_subdivision_with_noise(impli, oracle):
    shape, mc = _config2(24, subdiv={"enabled": 1})
    del mc["debug"]   # the default post_subdiv_noise (0.01)
    # hipRTC draws from the process's rand(), the oracle's generator: the oracle goes first, with no
    # compile in flight (jit_wait: earlier builds' compiles)
    impli.jit_wait()
    oracle.srand(1)
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    impli.srand(1)
    impli.set_jit(0)   # the interpreter kernels: this build starts no compile of its own
    try:
        v, f, n = impli.make_geometry(shape, mc, normals=True)
    finally:
        impli.set_jit(2)
    assert np.array_equal(f, fr) and np.array_equal(_u32(v), _u32(vr))
    assert len(v) > 4 * 1000
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape)), v, n)


def test_normals_ignore_root_matrix(impli, oracle):
    from implisolid_amd import scenes
    shape = dict(scenes.union_sphere_cube(), matrix=scenes.st(0.5, 0.125, 0, 0))
    # the value as the reference's property tree holds it (the oracle compares the text)
    mc = dict(scenes.mc_settings(24, 1.0), ignore_root_matrix="true")
    assert impli.parse_settings(mc)["ignore_root_matrix"] == 1 and oracle.parse_mc_settings(json.dumps(mc)).ignore_root_matrix
    v, f, n = impli.make_geometry(shape, mc, normals=True)
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    assert np.array_equal(f, fr) and np.array_equal(_u32(v), _u32(vr))
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape), True), v, n)
    # ... and the root matrix matters: with it the mesh is another one
    v2, _ = impli.make_geometry(shape, dict(mc, ignore_root_matrix="false"))
    assert v2.shape != v.shape or not np.array_equal(v2, v)


def test_every_evaluator_gives_the_same_normals(impli, oracle):
    """The interpreter kernel, the shape's point module and the baked module on config 3's tree (deeper
    than the shallowest interpreter class) at R = 32 after one repeat."""
    from implisolid_amd import scenes
    shape, mc = scenes.config3(32)
    mc["overall_repeats"] = 1
    out = []
    try:
        for mode, bake in ((0, 0), (1, 0), (1, 1)):
            impli.set_jit(mode)
            impli.set_jit_bake(bake)
            # another object in between: the engine keeps an unchanged object's modules across builds
            impli.make_geometry(TREES["sphere"], scenes.mc_settings(8, 1.0))
            v, f, n = impli.make_geometry(shape, mc, normals=True)
            impli.jit_wait()
            launches = impli.last_build_stats()["jit_launches"]
            assert (launches > 0) == (mode != 0), (mode, bake, launches)
            out.append((v, f, n, impli.normals_stats()))
    finally:
        impli.set_jit(2)
        impli.set_jit_bake(2)
    v, f, n, st = out[0]
    for v2, f2, n2, st2 in out[1:]:
        assert np.array_equal(f2, f) and same_bits(v2, v) and same_bits(n2, n) and st2 == st
    vr, fr = oracle.polygonize(json.dumps(shape), json.dumps(mc))
    assert np.array_equal(f, fr) and same_bits(v, vr)
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape)), v, n)


def test_normals_edges(impli, oracle):
    from implisolid_amd import scenes
    L = impli.lib()
    mc = scenes.mc_settings(24, 1.0)
    far = {"type": "iellipsoid", "matrix": scenes.st(0.25, 3.0, 0, 0)}
    v, f, n = impli.make_geometry_views(far, mc, normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    assert L.get_n_size() == 0 and not L.get_n_ptr() and impli.normals_stats() == (0, 0)
    assert not impli.last_error()
    # a build without the key directly after one with it exposes nothing
    shape = TREES["sphere"]
    v, f, n = impli.make_geometry_views(shape, mc, normals=True)
    assert L.get_n_size() == len(v) > 0 and L.get_n_ptr()
    v2, f2 = impli.make_geometry_views(shape, mc)
    assert L.get_n_size() == 0 and not L.get_n_ptr() and impli.normals_stats() == (0, 0)
    assert len(v2) == len(n)
    # true / false are no ints: the default, off
    impli.make_geometry_views(shape, dict(mc, normals={"enabled": True}))
    assert L.get_n_size() == 0 and not L.get_n_ptr()
    L.finish_geometry()


def test_progress_hook_sees_no_normals(impli, oracle):
    from implisolid_amd import scenes
    shape, mc = _config2(24)
    mc = impli._with_normals(mc, True)
    L = impli.lib()
    seen = []

    def hook(vp, nv, fp_, nf, pid, sid, cid, user):
        seen.append((int(nv), int(L.get_n_size()), bool(L.get_n_ptr())))

    cb = impli.PROGRESS_CALLBACK(hook)
    L.finish_geometry()
    # a build with normals first: the hook of the next build must not see them either
    v0, f0, n0 = impli.make_geometry_views(shape, mc, normals=True)
    n0 = np.array(n0)
    L.finish_geometry()
    L.implisolid_set_progress_callback(cb, None)
    try:
        L.build_geometry_u(json.dumps(shape).encode(), json.dumps(mc).encode(), b"{}")
    finally:
        L.implisolid_set_progress_callback(impli.PROGRESS_CALLBACK(), None)
    assert not impli.last_error()
    assert len(seen) == 1 + 2 * 3 and all(nv > 0 and size == 0 and not ptr for nv, size, ptr in seen), seen
    nv = L.get_v_size()
    assert L.get_n_size() == nv == len(n0)
    n = np.ctypeslib.as_array(ctypes.cast(L.get_n_ptr(), ctypes.POINTER(ctypes.c_float)), shape=(nv, 3)).copy()
    v = np.ctypeslib.as_array(ctypes.cast(L.get_v_ptr(), ctypes.POINTER(ctypes.c_float)), shape=(nv, 3)).copy()
    L.finish_geometry()
    assert same_bits(n, n0)
    _check_normals(impli, oracle, oracle.mp5_to_nodes(json.dumps(shape)), v, n)
    # MC only, with a hook: the same
    seen.clear()
    mc0 = impli._with_normals(scenes.mc_settings(24, 1.0), True)
    L.implisolid_set_progress_callback(cb, None)
    try:
        L.build_geometry_u(json.dumps(shape).encode(), json.dumps(mc0).encode(), b"{}")
    finally:
        L.implisolid_set_progress_callback(impli.PROGRESS_CALLBACK(), None)
    assert seen and all(size == 0 and not ptr for _, size, ptr in seen), seen
    assert L.get_n_size() == L.get_v_size() > 0
    L.finish_geometry()


def _threshold_points():
    """On the unit-matrix sphere |grad f| = 8 |x| along the x axis: the +-64 float patterns around
    x = 1.25e-5 put the norm on both sides of 1e-4; the centre has a zero gradient."""
    c = int(np.float32(1.25e-5).view(np.uint32))
    xs = np.arange(c - 64, c + 65, dtype=np.int64).astype(np.uint32).view(np.float32)
    pts = np.zeros((len(xs) + 1, 3), np.float32)
    pts[1:, 0] = xs
    return pts


@pytest.mark.parametrize("name", ["union_sphere_cube", "config3_tree", "sphere"])
def test_eval_normals(impli, oracle, name):
    shape = TREES[name]
    pts = np.random.default_rng(4321).uniform(-1.1, 1.1, size=(60001, 3)).astype(np.float32)
    if name == "sphere":
        # ... and points whose gradient is not finite, or whose norm overflows: the -42 branch keeps a
        # NaN row NaN, an infinite norm gives the factor -0 (random points of these trees give none)
        odd = np.array([[np.nan, 0, 0], [0.25, np.inf, 0], [1e30, 0, 0], [0, -3e19, 1e-3]], np.float32)
        pts = np.concatenate([_threshold_points(), -_threshold_points(), odd, pts[:1000]])
    tree = oracle.mp5_to_nodes(json.dumps(shape))
    ref, bad = normals_ref(oracle, tree, pts)
    with impli.ImplicitService(shape) as svc:
        n, problems = svc.normals(pts, return_problems=True)
        assert svc.normals(pts[:0]).shape == (0, 3)
        none = ctypes.c_int64(7)
        assert impli.lib().implisolid_eval_normals(None, 0, None, ctypes.byref(none)) == 0 and none.value == 0
        fp = ctypes.POINTER(ctypes.c_float)
        n2 = np.empty_like(n)
        assert impli.lib().implisolid_eval_normals(pts.ctypes.data_as(fp), len(pts), n2.ctypes.data_as(fp), None) == 0
    assert same_bits(n, ref), np.flatnonzero((_u32(n) != _u32(ref)).any(1))[:10]
    assert same_bits(n2, ref)
    assert problems == bad
    if name == "sphere":
        assert 64 < bad < len(_threshold_points()) * 2 - 60   # both sides of the threshold, both signs
        assert n[0].view(np.uint32).tolist() == ref[0].view(np.uint32).tolist()   # the centre: signed zeros
        assert np.isnan(ref).any(1).sum() >= 2 and np.isnan(n).any(1).sum() == np.isnan(ref).any(1).sum()


def test_multi_device_normals(impli, oracle):
    from implisolid_amd import scenes
    shape, mc = _config2(24)
    mc_only = scenes.mc_settings(24, 1.0)
    one = [impli.make_geometry(shape, m, normals=True) + (impli.normals_stats(),) for m in (mc_only, mc)]
    try:
        impli.set_devices([0, 0])
        two = [impli.make_geometry(shape, m, normals=True) + (impli.normals_stats(),) for m in (mc_only, mc)]
    finally:
        impli.set_devices(None)
    for (v, f, n, st), (v2, f2, n2, st2) in zip(one, two):
        assert np.array_equal(f2, f) and np.array_equal(_u32(v2), _u32(v))
        assert same_bits(n2, n) and st2 == st and st[0] == len(v)
    tree = oracle.mp5_to_nodes(json.dumps(shape))
    for v2, f2, n2, st2 in two:
        ref, bad = normals_ref(oracle, tree, v2)
        assert same_bits(n2, ref) and st2 == (len(v2), bad)


@pytest.mark.parametrize("rank", [0, 1])
def test_slab_normals(impli, oracle, rank):
    from implisolid_amd import scenes
    shape, mc = scenes.union_sphere_cube(), scenes.mc_settings(24, 1.0)
    s = impli.Slab(shape, mc, rank, 2)
    try:
        nv, nf = s.run()
        s.emit_normals()
        assert s.normals_ptr()
        v, f = s.download(nv, nf)
        n = s.download_normals(nv)
    finally:
        s.close()
    assert nv > 0
    ref, _ = normals_ref(oracle, oracle.mp5_to_nodes(json.dumps(shape)), v)
    assert same_bits(n, ref), np.flatnonzero((_u32(n) != _u32(ref)).any(1))[:10]
