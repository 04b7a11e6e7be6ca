"""CPU tests of the "sdf_3d" node: the MP5 compiler's parsing and validation (host only), the
scenes helper, and the numpy restatement's own consistency (tests/np_sdf3d.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_sdf3d  # noqa: E402

EYE = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def _node(**over):
    d = np_sdf3d.node(np_sdf3d.random_table(), EYE)
    d.update(over)
    return d


def test_program_info_accepts_a_full_node(impli):
    from implisolid_amd import scenes
    T = np_sdf3d.random_table()
    d = scenes.sdf3d_node(T.values.reshape(T.sz, T.sy, T.sx), T.gs, (T.ox, T.oy, T.oz), EYE, id=7)
    assert d == np_sdf3d.node(T, EYE, id=7)
    flat = scenes.sdf3d_node(list(T.values), T.gs, (T.ox, T.oy, T.oz), EYE, id=7, sizes=(T.sx, T.sy, T.sz))
    assert flat == d
    n_instr, depth, n_mats, mats = impli.program_info(d)
    assert n_instr == 2 and depth == 2
    # the node's inverse matrix, then the parameter rows: sizes, grid size, origin, value range
    assert n_mats >= 3 and np.array_equal(mats[0], np.array(EYE, np.float32))
    prm = mats[1:].reshape(-1)
    assert list(prm[:3]) == [T.sx, T.sy, T.sz]
    assert prm[3] == T.gs and list(prm[4:7]) == [T.ox, T.oy, T.oz]
    assert prm[7] == min(T.values.min(), 0) and prm[8] == max(T.values.max(), 0)
    # in a tree, with the rabbit's table and the sphere's
    for T2 in (np_sdf3d.rabbit_table(), np_sdf3d.sphere_table()):
        u = {"type": "Union", "matrix": EYE, "children": [np_sdf3d.node(T2, EYE), {"type": "iellipsoid", "matrix": EYE}]}
        assert impli.program_info(u)[0] == 6
    # ignore_root_matrix is honoured as for every primitive
    m = [0.5, 0, 0, 0.25, 0, 0.5, 0, 0, 0, 0, 0.5, 0]
    assert np.array_equal(impli.program_info(_node(matrix=m), ignore_root_matrix=True)[3][0], np.array(EYE, np.float32))
    assert impli.program_info(_node(matrix=m))[3][0][0] == 2.0


@pytest.mark.parametrize("over, field", [
    (dict(size_x=1), "size_x"), (dict(size_y=513), "size_y"), (dict(size_z=2.5), "size_z"), (dict(size_z="a"), "size_z"),
    (dict(sdf=[0.0] * 119), "sdf"), (dict(sdf=[0.0] * 121), "sdf"), (dict(sdf=3), "sdf"),
    (dict(sdf=[0.0] * 119 + ["nan"]), "sdf"), (dict(sdf=[0.0] * 119 + ["inf"]), "sdf"), (dict(sdf=[0.0] * 119 + ["x"]), "sdf"),
    (dict(grid_size=0), "grid_size"), (dict(grid_size=-0.25), "grid_size"), (dict(grid_size="inf"), "grid_size"),
    (dict(grid_size="nan"), "grid_size"), (dict(origin_x="nan"), "origin_x"), (dict(origin_y="inf"), "origin_y"),
    (dict(origin_z="-inf"), "origin_z"),
    # a grid below the origin's float spacing (1/16 at 1e6): origin + 5 * 0.008 rounds up to
    # origin + 0.0625, where the cell index would be 7, past the table
    (dict(grid_size=0.008, origin_x=1e6), "grid_size"),
])
def test_validation_names_the_field(impli, over, field):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.program_info(_node(**over))
    assert field in str(e.value), str(e.value)


def test_entry_count_limit(impli):
    # 512 * 512 * 17 > 2^22 (each size is within [2, 512])
    d = _node(size_x=512, size_y=512, size_z=17, sdf=[])
    with pytest.raises(impli.ImplisolidError) as e:
        impli.program_info(d)
    assert "2^22" in str(e.value) and "size_x" in str(e.value)


def test_at_most_eight_nodes(impli):
    leaf = _node()

    def union(n):
        return {"type": "Union", "matrix": EYE, "children": [leaf] * n}
    assert impli.program_info(union(8))[0] == 8 * 2 + 7 * 2
    with pytest.raises(impli.ImplisolidError) as e:
        impli.program_info(union(9))
    assert "sdf_3d" in str(e.value) and "8" in str(e.value)


@pytest.mark.parametrize("missing", ["size_x", "size_y", "size_z", "grid_size", "origin_x", "origin_y", "origin_z", "sdf"])
def test_table_less_node_stays_outside(impli, missing):
    d = _node()
    del d[missing]
    with pytest.raises(impli.ImplisolidError) as e:
        impli.program_info(d)
    assert 'MP5 type "sdf_3d" is outside the implemented node families' in str(e.value)
    assert missing in str(e.value)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.program_info({"type": "sdf_3d", "matrix": EYE})
    assert 'MP5 type "sdf_3d" is outside the implemented node families' in str(e.value)


@pytest.mark.parametrize("make", [np_sdf3d.random_table, np_sdf3d.rabbit_table, np_sdf3d.sphere_table])
def test_restated_gradient_is_the_values_derivative(make):
    """The restatement's float32 gradient against a float64 central difference of the trilinear
    interpolant, at points well inside cells (both difference points in the point's own cell), to
    1e-3 of the gradient's size."""
    T = make()
    rng = np.random.default_rng(11)
    n = 4000
    cell = np.stack([rng.integers(0, s - 1, n) for s in (T.sx, T.sy, T.sz)], axis=1)
    frac = rng.uniform(0.05, 0.95, (n, 3))
    org = np.array([T.ox, T.oy, T.oz], np.float64)
    p = (org + (cell + frac) * float(T.gs)).astype(np.float32)
    g = np_sdf3d.gradient(T, p[:, 0], p[:, 1], p[:, 2]).astype(np.float64)
    h = 0.01 * float(T.gs)
    pd = p.astype(np.float64)
    fd = np.zeros((n, 3))
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd[:, a] = (np_sdf3d.value_f64(T, *(pd + e).T) - np_sdf3d.value_f64(T, *(pd - e).T)) / (2 * h)
    scale = np.abs(fd).max(axis=1, keepdims=True) + 1e-30
    assert (np.abs(g - fd) / scale).max() < 1e-3
    # and the float32 value is the float64 interpolant to float32 accuracy
    v = np_sdf3d.value(T, p[:, 0], p[:, 1], p[:, 2])
    assert np.abs(v - np_sdf3d.value_f64(T, *pd.T)).max() < 1e-5 * max(1.0, float(np.abs(T.values).max()))
    # outside the table box: -10000 and a zero gradient
    far = np.array([[float(T.ox) - 1.0, float(T.oy), float(T.oz)]], np.float32)
    assert np_sdf3d.value(T, *far.T)[0] == np.float32(-10000)
    assert not np_sdf3d.gradient(T, *far.T).any()


def test_restated_rabbit_matches_np_restate():
    """With the rabbit's table the restatement is np_restate.cube wherever no read falls on the
    rabbit's four trailing members (indices N .. N + 3): those read 0 here."""
    import np_restate
    T = np_sdf3d.rabbit_table()
    rng = np.random.default_rng(3)
    lo = np.array([T.ox, T.oy, T.oz], np.float64)
    hi = np.array([float(v) for v in T.hi()])
    c, h = (lo + hi) / 2, (hi - lo) / 2
    p = (c + 1.2 * h * rng.uniform(-1, 1, (200000, 3))).astype(np.float32)
    inside, idx = np_sdf3d.read_indices(T, p[:, 0], p[:, 1], p[:, 2])
    excluded = np.zeros(len(p), bool)
    excluded[inside] = ((idx >= T.N) & (idx < T.N + 4)).any(axis=1)
    assert excluded.mean() <= 0.01
    a = np_sdf3d.value(T, p[:, 0], p[:, 1], p[:, 2])
    b = np_restate.cube(p[:, 0], p[:, 1], p[:, 2])
    assert np.array_equal(a[~excluded].view(np.uint32), b[~excluded].view(np.uint32))


def test_pyramid_rule_covers_the_readable_entries():
    """The lookup rule's blocks contain every entry a box can read, at every box size."""
    rng = np.random.default_rng(2)
    for T in (np_sdf3d.random_table(), np_sdf3d.sphere_table()):
        lo = np.array([T.ox, T.oy, T.oz], np.float64)
        hi = np.array([float(v) for v in T.hi()])
        for _ in range(200):
            a = rng.uniform(lo - 0.2, hi + 0.2, 3)
            b = a + rng.uniform(0, 1, 3) ** 3 * (hi - lo)
            box = np.stack([a, b], axis=1).reshape(-1)
            cells, all_in, none_in = np_sdf3d.box_cells(T, box)
            if none_in:
                continue
            rmin, rmax = np_sdf3d.readable_range(T, cells)
            pmin, pmax, L = np_sdf3d.pyramid_range(T, cells)
            assert pmin <= rmin and rmax <= pmax
            assert all((c1 >> L) - (c0 >> L) <= 1 for c0, c1 in cells)
