"""GPU tests of the "sdf_3d" node (a caller-supplied SDF table): values, gradients, interval bounds,
pruning and the JIT tiers, table identity between objects, and the paths through the stack, all
against the independent numpy restatement tests/np_sdf3d.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrices  # noqa: E402
import np_restate  # noqa: E402
import np_sdf3d  # noqa: E402

pytestmark = pytest.mark.gpu

EYE = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
TABLES = {"random": np_sdf3d.random_table, "rabbit": np_sdf3d.rabbit_table, "sphere": np_sdf3d.sphere_table}
f32 = np.float32


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lohi(T):
    return np.array([T.ox, T.oy, T.oz], np.float32), np.array(T.hi(), np.float32)


def _local_points(T, seed, n=6000):
    """Cell interiors, exact cell boundaries, the six box faces, points outside (float32, node frame)."""
    rng = np.random.default_rng(seed)
    lo, hi = _lohi(T)
    c, h = (lo.astype(np.float64) + hi) / 2, (hi.astype(np.float64) - lo) / 2
    p = (c + 1.2 * h * rng.uniform(-1, 1, (n, 3))).astype(np.float32)
    size = np.array([T.sx, T.sy, T.sz])
    # exact cell boundaries: origin + k grid_size in float32 on one or more axes (k = 0 .. size)
    q = p[: n // 3].copy()
    k = np.stack([rng.integers(0, s + 1, len(q)) for s in size], axis=1)
    on = rng.uniform(size=q.shape) < 0.6
    q[on] = (lo + k.astype(np.float32) * T.gs)[on]
    # the six faces, exactly: the lower corner and origin + grid_size * size as the device computes it
    faces = []
    for a in range(3):
        for v in (lo[a], hi[a]):
            r = p[: n // 12].copy()
            r[:, a] = v
            faces.append(r)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    return np.concatenate([p, q] + faces + [corners])


@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("mat", ["eye", "scale", "rot", "shear", "mirror"])
def test_values_and_gradients_bitwise(impli, name, mat):
    T = TABLES[name]()
    lo, hi = _lohi(T)
    extent = float((hi - lo).max())
    m = {"eye": EYE, "scale": [0.125, 0, 0, 0.5, 0, 0.125, 0, 0.375, 0, 0, 0.125, -0.5]}.get(mat) or \
        matrices.matrix(mat, 3, scale=1.0 / extent)
    d = np_sdf3d.node(T, m)
    local = _local_points(T, 17)
    pts = matrices.forward(m, local).astype(np.float32) if mat != "eye" else local
    with impli.ImplicitService(d) as svc:
        f, g = svc.eval(pts, gradient=True)
    fr, gr = np_sdf3d.leaf_value_gradient(d, pts)
    assert np.array_equal(_u32(f), _u32(fr)), np.flatnonzero(_u32(f) != _u32(fr))[:10]
    assert np.array_equal(_u32(g), _u32(gr)), np.flatnonzero((_u32(g) != _u32(gr)).any(axis=1))[:10]
    # the zero-padding rule: every point with a read at a flat index >= N, with those reads as 0
    mi = np_restate._inverse(m)
    X, Y, Z = np_restate._xform(mi, pts[:, 0], pts[:, 1], pts[:, 2])
    inside, idx = np_sdf3d.read_indices(T, X, Y, Z)
    past = np.zeros(len(pts), bool)
    past[inside] = (idx >= T.N).any(axis=1)
    assert past.sum() > 50
    explicit = np_sdf3d.Table(T.values, (T.sx, T.sy, T.sz), T.gs, (T.ox, T.oy, T.oz))
    explicit.padded = np.concatenate([T.values, np.zeros(len(T.padded) - T.N, np.float32)])
    assert np.array_equal(_u32(f[past]), _u32(np_sdf3d.value(explicit, X[past], Y[past], Z[past])))
    assert (f[~inside] == f32(-10000)).all() and not g[~inside].any()


# ---- rabbit equivalence ---------------------------------------------------------------------------------
def _excluded(T, X, Y, Z):
    """points with one of the eight reads on the rabbit's trailing members, indices [N, N + 4)"""
    inside, idx = np_sdf3d.read_indices(T, X, Y, Z)
    ex = np.zeros(len(X), bool)
    ex[inside] = ((idx >= T.N) & (idx < T.N + 4)).any(axis=1)
    return ex


def test_rabbit_table_equals_icube(impli):
    from implisolid_amd import scenes
    T = np_sdf3d.rabbit_table()
    m = scenes.st(0.125, 0.5, 0.375, -0.5)
    lo, hi = _lohi(T)
    c, h = (lo.astype(np.float64) + hi) / 2, (hi.astype(np.float64) - lo) / 2
    local = (c + 1.2 * h * np.random.default_rng(23).uniform(-1, 1, (200000, 3))).astype(np.float32)
    pts = matrices.forward(m, local).astype(np.float32)
    X, Y, Z = np_restate._xform(np_restate._inverse(m), pts[:, 0], pts[:, 1], pts[:, 2])
    ex = _excluded(T, X, Y, Z)
    assert ex.mean() <= 0.01
    with impli.ImplicitService(np_sdf3d.node(T, m)) as svc:
        a = svc.eval(pts)
    with impli.ImplicitService({"type": "icube", "matrix": m}) as svc:
        b = svc.eval(pts)
    assert np.array_equal(_u32(a[~ex]), _u32(b[~ex]))
    assert (~ex).sum() > 190000


def test_config2_mesh_with_the_rabbit_as_sdf3d(impli):
    from implisolid_amd import scenes
    shape = scenes.union_sphere_cube()
    T = np_sdf3d.rabbit_table()
    cube = shape["children"][1]
    assert cube["type"] == "cube"
    swapped = json.loads(json.dumps(shape))
    swapped["children"][1] = np_sdf3d.node(T, cube["matrix"])
    R, box = 32, 1.0
    mc = scenes.mc_settings(R, box)
    # no grid sample of this box reads the rabbit's trailing members
    res = R + 5
    w = (f32(box) - f32(-box)) / f32(R)
    s = np.arange(res).astype(np.float32) * w + f32(-box) - f32(2) * w
    Zg, Yg, Xg = np.meshgrid(s, s, s, indexing="ij")
    X, Y, Z = np_restate._xform(np_restate._inverse(cube["matrix"]), Xg.ravel(), Yg.ravel(), Zg.ravel())
    assert not _excluded(T, X, Y, Z).any()
    v0, f0 = impli.make_geometry(shape, mc)
    v1, f1 = impli.make_geometry(swapped, mc)
    assert len(f0) > 1000 and np.array_equal(f0, f1)
    assert np.array_equal(_u32(v0), _u32(v1))


# ---- intervals --------------------------------------------------------------------------------------------
def _settle(lo, hi):
    """the interval evaluator's output stage for every primitive (ifunc_interval.hpp settle): a
    relative 2^-16 margin on the primitive's bound, in float32"""
    lo, hi = f32(lo), f32(hi)
    s = max(abs(lo), abs(hi)) * f32(1.0 / 65536.0) + f32(1e-30)
    return f32(lo - s), f32(hi + s)


def _boxes(T, seed):
    """(boxes [n, 6], kinds): inside one cell, across 2 to 40 cells, the whole table, straddling
    the box faces, wholly outside."""
    rng = np.random.default_rng(seed)
    lo, hi = _lohi(T)
    lo64, gs = lo.astype(np.float64), float(T.gs)
    size = np.array([T.sx, T.sy, T.sz])
    out, kinds = [], []
    for _ in range(24):   # strictly inside one cell
        c = np.array([rng.integers(0, s) for s in size])
        a = lo64 + (c + rng.uniform(0.1, 0.4, 3)) * gs
        b = lo64 + (c + rng.uniform(0.6, 0.9, 3)) * gs
        out.append(np.stack([a, b], 1).ravel()); kinds.append("cell")
    for span in range(2, 41):   # across `span` cells on the axes that are long enough
        n = np.minimum(span, size)
        c = np.array([rng.integers(0, s - k + 1) for s, k in zip(size, n)])
        a = lo64 + (c + rng.uniform(0.05, 0.95, 3)) * gs
        b = lo64 + (c + n - 1 + rng.uniform(0.05, 0.95, 3)) * gs
        out.append(np.stack([a, np.maximum(a, b)], 1).ravel()); kinds.append("span")
    out.append(np.stack([lo, hi], 1).ravel()); kinds.append("whole")
    out.append(np.stack([lo64 - 1.0, hi.astype(np.float64) + 1.0], 1).ravel()); kinds.append("straddle")
    for a in range(3):   # straddling one face each
        for side in (0, 1):
            b = np.stack([lo64 + 0.3 * gs, lo64 + 2.6 * gs], 1)
            b[a] = (lo64[a] - 0.7 * gs, lo64[a] + 1.2 * gs) if side == 0 else (float(hi[a]) - 1.3 * gs, float(hi[a]) + 0.4 * gs)
            out.append(b.ravel()); kinds.append("straddle")
    for a in range(3):   # wholly outside
        b = np.stack([lo64 + 0.3 * gs, lo64 + 2.6 * gs], 1)
        b[a] = (float(hi[a]) + 0.5 * gs, float(hi[a]) + 3 * gs)
        out.append(b.ravel()); kinds.append("outside")
    return np.array(out).astype(np.float32), kinds


@pytest.mark.parametrize("name", list(TABLES))
def test_interval_bounds(impli, name):
    T = TABLES[name]()
    d = np_sdf3d.node(T, EYE)
    boxes, kinds = _boxes(T, 31)
    ivs = [impli.debug_intervals(d, boxes, variant=v)[0] for v in (0, 1, 2)]
    for other in ivs[1:]:
        assert np.array_equal(_u32(ivs[0]), _u32(other))
    rng = np.random.default_rng(5)
    for (lo, hi), box, kind in zip(ivs[0], boxes, kinds):
        assert lo <= hi, (kind, box)
        # the restated values of 512 points of the box (its corners among them)
        u = rng.uniform(size=(512, 3))
        u[:8] = [[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        b = box.reshape(3, 2).astype(np.float64)
        p = np.clip((b[:, 0] + u * (b[:, 1] - b[:, 0])).astype(np.float32), box[0::2], box[1::2])
        v = np_sdf3d.value(T, p[:, 0], p[:, 1], p[:, 2])
        assert lo <= v.min() and v.max() <= hi, (kind, box, lo, hi, v.min(), v.max())
        cells, all_in, none_in = np_sdf3d.box_cells(T, box)
        assert none_in == (kind == "outside")
        if none_in:
            assert (lo, hi) == _settle(f32(-10000), f32(-10000))
            continue
        # contains the widened range of the readable entries ...
        rlo, rhi = np_sdf3d.widen(*np_sdf3d.readable_range(T, cells), all_in)
        assert lo <= rlo and rhi <= hi, (kind, box)
        # ... and is contained in that of the level-L blocks of the lookup rule
        pmin, pmax, L = np_sdf3d.pyramid_range(T, cells)
        plo, phi = _settle(*np_sdf3d.widen(pmin, pmax, all_in))
        assert plo <= lo and hi <= phi, (kind, box, L)
        if kind == "cell":   # the eight corners' hull, exactly
            assert all_in and L == 0 and all(c0 == c1 for c0, c1 in cells)
            assert (lo, hi) == _settle(*np_sdf3d.widen(*np_sdf3d.readable_range(T, cells), True)), box


# ---- pruning and tiers ------------------------------------------------------------------------------------
def _trees():
    from implisolid_amd import scenes
    S = np_sdf3d.sphere_table()
    Rn = np_sdf3d.random_table()
    union = {"type": "Union", "matrix": EYE, "children": [
        np_sdf3d.node(S, scenes.st(0.5, 0.25, 0.0, 0.125)),
        {"type": "icylinder", "matrix": scenes.st(0.5, -0.375, -0.25, 0.25)},
        {"type": "iellipsoid", "matrix": scenes.st(0.5, 0.5, 0.5, -0.5)}]}
    diff = {"type": "Difference", "matrix": scenes.st(1, 0.0625, 0, 0), "children": [
        {"type": "iellipsoid", "matrix": scenes.st(1.5, 0, 0, 0)},
        {"type": "Union", "matrix": EYE, "children": [np_sdf3d.node(Rn, scenes.st(0.5, 0.125, 0, 0)),
                                                      {"type": "icone", "matrix": scenes.st(0.5, -0.5, 0.25, 0)}]}]}
    return {"union": union, "difference": diff}


@pytest.mark.parametrize("name", ["union", "difference"])
def test_pruning_levels_and_jit_tiers(impli, name):
    from implisolid_amd import scenes
    shape, mc = _trees()[name], scenes.mc_settings(32, 1.0)
    fields, meshes, tiers = [], [], []
    try:
        impli.set_jit(0)
        for level in (0, 1, 2):
            impli.set_pruning(level)
            s = impli.Slab(shape, mc)
            try:
                nv, nf = s.run()
                meshes.append(s.download(nv, nf))
                fields.append(s.read_field())
            finally:
                s.close()
        impli.set_pruning(2)
        for mode, bake in ((0, False), (1, False), (1, True)):
            impli.set_jit(mode)
            impli.set_jit_bake(bake)
            s = impli.Slab(shape, mc)
            try:
                s.eval()
                assert s.used_jit() == bool(mode)
                tiers.append((s.read_field(), s.read_signs(), s.brick_stats()))
            finally:
                s.close()
    finally:
        impli.set_jit(2)
        impli.set_jit_bake(2)
        impli.set_pruning(2)
    assert np.array_equal(_u32(fields[0]), _u32(fields[1]))
    assert len(meshes[0][1]) > 500
    for v, f in meshes[1:]:
        assert np.array_equal(f, meshes[0][1]) and np.array_equal(_u32(v), _u32(meshes[0][0]))
    for fb, sb, bb in tiers[1:]:
        assert np.array_equal(_u32(tiers[0][0]), _u32(fb)), np.flatnonzero(tiers[0][0] != fb)[:10]
        assert np.array_equal(tiers[0][1], sb)
        assert tiers[0][2] == bb
    assert tiers[0][2][1] < tiers[0][2][0]   # the interval pass pruned something


# ---- table identity ---------------------------------------------------------------------------------------
def test_objects_that_differ_only_in_table_values(impli):
    """A, then B (the same node but for its "sdf" values), then A again, on the engine that keeps
    modules and baked code for the object it saw last; repeated past the hot-object threshold."""
    from implisolid_amd import scenes
    S = np_sdf3d.sphere_table()
    m = scenes.st(1, 0, 0, 0)
    A = np_sdf3d.node(S, m)
    B = json.loads(json.dumps(A))
    z, y, x = np.meshgrid(np.arange(S.sz), np.arange(S.sy), np.arange(S.sx), indexing="ij")
    gs = float(S.gs)
    dB = np.sqrt((float(S.ox) + gs * x - 0.1) ** 2 + (float(S.oy) + gs * y) ** 2 + (float(S.oz) + gs * z) ** 2) - 0.45
    B["sdf"] = [float(v) for v in dB.astype(np.float32).reshape(-1)]
    mc = scenes.mc_settings(24, 1.0)
    pts = np.random.default_rng(9).uniform(-1.1, 1.1, (20000, 3)).astype(np.float32)
    fB = np_sdf3d.evaluate(B, pts[:, 0], pts[:, 1], pts[:, 2])
    fA = np_sdf3d.evaluate(A, pts[:, 0], pts[:, 1], pts[:, 2])
    assert not np.array_equal(fA, fB)
    first = {}
    for rnd in range(2):
        for key, shape, want in (("A", A, fA), ("B", B, fB)):
            for build in range(5):   # the fifth build runs the object's baked module (hot after 4)
                v, f = impli.make_geometry(shape, mc)
                if key not in first:
                    first[key] = (v, f)
                assert np.array_equal(f, first[key][1]) and np.array_equal(_u32(v), _u32(first[key][0])), (rnd, key, build)
                impli.jit_wait()
            with impli.ImplicitService(shape) as svc:
                assert np.array_equal(_u32(svc.eval(pts)), _u32(want)), (rnd, key)
    assert len(first["A"][1]) > 200 and len(first["B"][1]) > 200
    assert first["A"][0].shape != first["B"][0].shape or not np.array_equal(first["A"][0], first["B"][0])
    v, f = impli.make_geometry(A, mc)
    assert np.array_equal(f, first["A"][1]) and np.array_equal(_u32(v), _u32(first["A"][0]))


# ---- through the stack --------------------------------------------------------------------------------------
def test_normals_with_one_ob02_repeat(impli):
    from implisolid_amd import scenes
    d = np_sdf3d.node(np_sdf3d.sphere_table(), EYE)
    mc = scenes.mc_settings(32, 1.0, vresampl_iters=1, vresampl_c=0.4, projection=1, qem=1, overall_repeats=1)
    v, f, n = impli.make_geometry(d, mc, normals=True)
    assert len(v) > 500 and n.shape == v.shape
    with impli.ImplicitService(d) as svc:
        want = svc.normals(v)
    assert np.array_equal(_u32(n), _u32(want))


def test_two_tables_in_one_tree(impli):
    from implisolid_amd import scenes
    tree = {"type": "Union", "matrix": scenes.st(1, 0.0625, 0, 0), "children": [
        np_sdf3d.node(np_sdf3d.sphere_table(), scenes.st(0.5, 0.25, 0.25, 0), id=1),
        {"type": "Difference", "matrix": EYE, "children": [
            {"type": "iellipsoid", "matrix": scenes.st(1, -0.375, -0.25, 0.25)},
            np_sdf3d.node(np_sdf3d.random_table(), matrices.matrix("rot", 1, scale=0.5), id=2)]}]}
    pts = np.random.default_rng(4).uniform(-1.1, 1.1, (50000, 3)).astype(np.float32)
    with impli.ImplicitService(tree) as svc:
        f = svc.eval(pts)
        q = svc.query_implicit_values(pts[:4000])
    want = np_sdf3d.evaluate(tree, pts[:, 0], pts[:, 1], pts[:, 2])
    assert np.array_equal(_u32(f), _u32(want))
    assert np.array_equal(_u32(q), _u32(want[:4000]))
    assert len(np.unique(want)) > 1000


def test_two_slab_split(impli):
    from implisolid_amd import scenes
    shape, mc = _trees()["union"], scenes.mc_settings(40, 1.0)
    one = impli.Slab(shape, mc, 0, 1)
    nv, nf = one.run()
    ref_v, ref_f = one.download(nv, nf)
    one.close()
    slabs = [impli.Slab(shape, mc, r, 2) for r in range(2)]
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
        s.close()
    assert all(len(f) > 0 for f in fs) and len(ref_f) > 500
    assert np.array_equal(np.concatenate(fs), ref_f)
    assert np.array_equal(_u32(np.concatenate(vs)), _u32(ref_v))


# ---- object streams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [0, 2])
def test_batch_rejects_sdf3d(impli, n_streams):
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0)
    plain = [{"type": "iellipsoid", "matrix": EYE}, {"type": "icone", "matrix": EYE}]
    with pytest.raises(impli.ImplisolidError) as e:
        impli.Batch(plain + [np_sdf3d.node(np_sdf3d.random_table(), EYE)], mc, n_streams=n_streams)
    assert "sdf_3d" in str(e.value)
    with impli.Batch(plain, mc, n_streams=n_streams) as b:
        b.run()
        v, f = b.download(0)
    ref = impli.make_geometry(plain[0], mc)
    assert np.array_equal(f, ref[1]) and np.array_equal(_u32(v), _u32(ref[0]))
