"""Host side of the mass properties (implisolid_mass_mids, implisolid_mass_physical) against the
restatement tests/np_mass.py, and the inputs of tests/test_gpu_mass.py.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_bounds   # noqa: E402
import np_mass   # noqa: E402
import np_sdf3d   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("implisolid_mass", "implisolid_mass_mids", "implisolid_mass_physical")
UNIT = [-1, 1, -1, 1, -1, 1]
NON_DYADIC = [-0.7, 1.3, 0.1, 0.9, -2.1, 0.3]
FAR = [1000, 1000.5, -1000.25, -999.75, 1000, 1000.5]   # extent 0.5 at (1000, -1000, 1000)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_declares_the_mass_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("int %s(" % name) in header, name


@pytest.mark.parametrize("box, depth", [(NON_DYADIC, 3), (NON_DYADIC, 6), (NON_DYADIC, 10), (FAR, 3), (FAR, 6),
                                        (FAR, 10), (UNIT, 3), (UNIT, 6), (UNIT, 10)])
def test_mids_equal_the_restatement_and_stay_in_their_cells(impli, box, depth):
    M = impli.mass_mids(box, depth)
    R = np_mass.mids(box, depth)
    N = 1 << depth
    assert M.shape == (3, N) and M.dtype == np.float32
    assert np.array_equal(_u32(M), _u32(R))
    E = impli.bounds_edges(box, depth)
    assert np.array_equal(_u32(E), _u32(np_bounds.edges(box, depth)))
    assert (E[:, :-1] <= M).all() and (M <= E[:, 1:]).all()


def test_mids_on_the_unit_box_are_the_odd_multiples(impli):
    M = impli.mass_mids(UNIT, 5)
    want = ((2 * np.arange(32) + 1) / 32.0 - 1.0).astype(np.float32)
    assert np.array_equal(_u32(M), _u32(np.stack([want] * 3)))


def _check_physical(impli, box, depth, m, cells=None):
    """the library against np_mass (1e-13 of the largest tensor entry: fewer than twenty double roundings
    after exact integers) and, given the cells, against the float64 sum over cuboids (1e-9 relative)"""
    empty, out = impli.mass_physical(box, depth, np.array(m, np.uint64))
    r_empty, ref = np_mass.physical(box, depth, m)
    assert empty == r_empty and not empty
    big = np.abs(ref[4:]).max()
    print("box", box, "depth", depth, "n", m[0], "volume", out[0], "centre", out[1:4], "inertia", out[4:])
    print("  against np_mass: volume", abs(out[0] - ref[0]) / ref[0], "centre", np.abs(out[1:4] - ref[1:4]).max(),
          "tensor / largest", np.abs(out[4:] - ref[4:]).max() / big)
    assert abs(out[0] - ref[0]) <= 1e-13 * ref[0]
    assert np.abs(out[1:4] - ref[1:4]).max() <= 1e-13 * max(1.0, np.abs(ref[1:4]).max())
    assert np.abs(out[4:] - ref[4:]).max() <= 1e-13 * big
    if cells is not None:
        V, com, I = np_mass.cuboid_sum(box, depth, *cells)
        got = np.array([[out[4], out[7], out[9]], [out[7], out[5], out[8]], [out[9], out[8], out[6]]])
        print("  against the cuboid sum: volume", abs(out[0] - V) / V, "centre", np.abs(out[1:4] - com).max(),
              "tensor / largest", np.abs(got - I).max() / np.abs(I).max())
        assert abs(out[0] - V) <= 1e-9 * V
        assert np.abs(out[1:4] - com).max() <= 1e-9 * max(1.0, np.abs(com).max())
        assert np.abs(got - I).max() <= 1e-9 * np.abs(I).max()
    return out


@pytest.mark.parametrize("box", [UNIT, NON_DYADIC])
def test_physical_of_one_cell(impli, box):
    i, j, k = [5], [17], [30]
    m = np_mass.moments_of_cells(i, j, k)
    assert m == [1, 5, 17, 30, 25, 289, 900, 85, 510, 150]
    out = _check_physical(impli, box, 5, m, (i, j, k))
    b = np.asarray(box, np.float32).astype(np.float64).reshape(3, 2)
    d = (b[:, 1] - b[:, 0]) / 32
    # one cuboid: c_ab = 0, the 1/12 terms alone
    assert abs(out[4] - out[0] * (d[1] ** 2 + d[2] ** 2) / 12) <= 1e-13 * out[4] and out[7] == 0 and out[8] == 0 and out[9] == 0


@pytest.mark.parametrize("box, depth", [(UNIT, 5), (NON_DYADIC, 5), (NON_DYADIC, 10)])
def test_physical_of_the_full_box(impli, box, depth):
    N = 1 << depth
    m = np_mass.box_moments(0, N, 0, N, 0, N)
    assert m[0] == N ** 3 and m[1] == N * N * (N * (N - 1) // 2) and m[4] == N * N * ((N - 1) * N * (2 * N - 1) // 6)
    cells = None
    if depth == 5:
        k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
        cells = (i.ravel(), j.ravel(), k.ravel())
        assert np_mass.moments_of_cells(*cells) == m
    out = _check_physical(impli, box, depth, m, cells)
    b = np.asarray(box, np.float32).astype(np.float64).reshape(3, 2)
    L = b[:, 1] - b[:, 0]
    V = L.prod()
    assert abs(out[0] - V) <= 1e-13 * V
    assert np.abs(out[1:4] - b.mean(axis=1)).max() <= 1e-13 * max(1.0, np.abs(b).max())
    want = [V * (L[1] ** 2 + L[2] ** 2) / 12, V * (L[0] ** 2 + L[2] ** 2) / 12, V * (L[0] ** 2 + L[1] ** 2) / 12]
    assert np.abs(out[4:7] - want).max() <= 1e-12 * max(want)
    assert np.abs(out[7:]).max() <= 1e-12 * max(want)


@pytest.mark.parametrize("box", [UNIT, NON_DYADIC])
def test_physical_of_a_random_set_of_cells(impli, box):
    rng = np.random.default_rng(3)
    S = rng.random((32, 32, 32)) < 0.3
    k, j, i = np.nonzero(S)
    m = np_mass.moments_of_cells(i, j, k)
    # the array route of the restatement gives the same integers
    mf, layers = np_mass.moments(np.where(S, np.float32(1), np.float32(-1)))
    assert mf == m and layers.sum() == m[0] and np.array_equal(layers, S.reshape(32, -1).sum(axis=1))
    assert 2 ** 12 < m[0] <= 2 ** 15
    _check_physical(impli, box, 5, m, (i, j, k))


def test_the_restatement_counts_negative_zero_and_nan_as_solid():
    F = np.full((8, 8, 8), -1, np.float32)
    F[1, 2, 3], F[4, 5, 6], F[7, 0, 0] = -0.0, np.nan, 0.25
    m, layers = np_mass.moments(F)
    assert m == np_mass.moments_of_cells([3, 6, 0], [2, 5, 0], [1, 4, 7])
    assert layers.tolist() == [0, 1, 0, 0, 1, 0, 0, 1]


def test_physical_of_nothing_is_zero(impli):
    empty, out = impli.mass_physical(UNIT, 5, np.zeros(10, np.uint64))
    assert empty and (out == 0).all()
    assert impli.lib().implisolid_mass_physical(
        np.array(UNIT, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 5,
        np.zeros(10, np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    r_empty, ref = np_mass.physical(UNIT, 5, [0] * 10)
    assert r_empty and (ref == 0).all()


@pytest.mark.parametrize("box, depth", [(UNIT, 2), (UNIT, 11), ([1, -1, -1, 1, -1, 1], 5), ([-1, 1, 0, 0, -1, 1], 5),
                                        ([-1, np.inf, -1, 1, -1, 1], 5), ([-1, 1, -1, 1, np.nan, 1], 5)])
def test_bad_depth_or_box_is_refused_with_a_message(impli, box, depth):
    L = impli.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    b = np.array(box, np.float32)
    mids = np.zeros(3 * 2048, np.float32)
    assert L.implisolid_mass_mids(b.ctypes.data_as(fp), depth, mids.ctypes.data_as(fp)) == -1 and impli.last_error()
    out = np.zeros(10, np.float64)
    mom = np.ones(10, np.uint64)
    assert L.implisolid_mass_physical(b.ctypes.data_as(fp), depth, mom.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1 and impli.last_error()
    with pytest.raises(impli.ImplisolidError):
        impli.mass_mids(box, depth)
    with pytest.raises(impli.ImplisolidError):
        impli.mass_physical(box, depth, mom)
    assert impli.mass_mids(UNIT, 3).shape == (3, 8), "and the next call works"


# ---- the input of test_gpu_mass.py's -0.0 test --------------------------------------------------------
def test_the_zero_table_puts_negative_zeros_on_known_mids():
    import test_gpu_mass as g
    node, zeros = g.zero_node()
    M = np_mass.mids(UNIT, g.ZERO_DEPTH)
    T = np_sdf3d.Table.from_node(node)
    # the table's nodes are the mids: dyadic, aligned
    assert np.array_equal(_u32(M[0]), _u32(T.ox + T.gs * np.arange(T.sx, dtype=np.float32)))
    F = np_sdf3d.evaluate(node, *np_mass.points(M).T).reshape(T.sz, T.sy, T.sx)
    assert np.array_equal(_u32(F), _u32(-T.values.reshape(T.sz, T.sy, T.sx))), "every sample is a table entry, negated"
    zero = F == 0
    assert zero.sum() == zeros.sum() >= 100 and np.array_equal(zero, zeros) and np.signbit(F[zero]).all()
    # they matter: the count with them differs from the count of the strictly positive samples
    assert np_mass.moments(F)[0][0] == (F > 0).sum() + zeros.sum()
