"""Host side of the layer images (implisolid_raster_coords, implisolid_raster's argument checks) against
the restatement tests/np_raster.py, and the restatement's own rule.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raster   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("implisolid_raster", "implisolid_raster_coords")
UNIT = [-1, 1, -1, 1]
UNEQUAL = [-0.7, 1.3, 0.1, 0.9]              # unequal, non-dyadic steps
FAR = [1000, 1000.5, -1000.25, -1000.0]      # extent 0.5 x 0.25 at (1000, -1000)
EGG = {"type": "iellipsoid", "matrix": [0.5, 0, 0, 0.25, 0, 0.25, 0, -0.125, 0, 0, 1, 0.1875]}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_declares_the_raster_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("int %s(" % name) in header, name


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("W, H", [(40, 33), (33, 17), (1, 16384)])
@pytest.mark.parametrize("rect", [UNIT, UNEQUAL, FAR])
def test_coords_equal_the_restatement_and_stay_in_their_sub_cells(impli, rect, W, H, s):
    mx, my = impli.raster_coords(rect, W, H, s)
    rx, ry = np_raster.coords(rect, W, H, s)
    assert mx.dtype == np.float32 and my.dtype == np.float32 and mx.shape == (W * s,) and my.shape == (H * s,)
    assert np.array_equal(_u32(mx), _u32(rx)) and np.array_equal(_u32(my), _u32(ry))
    ex, ey = np_raster.edges(rect[0], rect[1], W * s), np_raster.edges(rect[2], rect[3], H * s)
    assert ex[0] == np.float32(rect[0]) and ex[-1] == np.float32(rect[1]) and ey[-1] == np.float32(rect[3])
    assert (ex[:-1] <= mx).all() and (mx <= ex[1:]).all()
    assert (ey[:-1] <= my).all() and (my <= ey[1:]).all()
    # the edges are implisolid_slice_coords' with W s cells, where that entry takes the size
    if W * s == H * s <= 4096:
        xs, ys = impli.slice_coords(rect, W * s)
        assert np.array_equal(_u32(xs), _u32(ex)) and np.array_equal(_u32(ys), _u32(ey))


@pytest.mark.parametrize("s", [1, 2, 4])
def test_square_coords_use_the_slice_edges(impli, s):
    xs, ys = impli.slice_coords(UNEQUAL, 24 * s)
    assert np.array_equal(_u32(xs), _u32(np_raster.edges(UNEQUAL[0], UNEQUAL[1], 24 * s)))
    mx, my = impli.raster_coords(UNEQUAL, 24, 24, s)
    assert np.array_equal(_u32(mx), _u32(np_raster.mids(xs))) and np.array_equal(_u32(my), _u32(np_raster.mids(ys)))


def test_coords_equal_the_mass_mids(impli):
    import test_gpu_mass as g
    for box in (g.UNIT, g.NON_DYADIC):
        M = impli.mass_mids(box, 5)
        for W, s in ((32, 1), (16, 2)):
            mx, my = impli.raster_coords(box[:4], W, W, s)
            assert np.array_equal(_u32(mx), _u32(M[0])) and np.array_equal(_u32(my), _u32(M[1])), (box, W, s)


BAD = [dict(W=0), dict(W=16385), dict(H=0), dict(H=16385), dict(s=3), dict(s=0), dict(s=8), dict(rect=[1, -1, -1, 1]),
       dict(rect=[-1, 1, 0.5, 0.5]), dict(rect=[-1, np.inf, -1, 1]), dict(rect=[-1, 1, np.nan, 1])]


@pytest.mark.parametrize("kw", BAD)
def test_bad_sizes_and_rects_are_refused_with_a_message(impli, kw):
    L = impli.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    rect, W, H, s = np.array(kw.get("rect", UNIT), np.float32), kw.get("W", 8), kw.get("H", 8), kw.get("s", 2)
    mx, my = np.zeros(70000, np.float32), np.zeros(70000, np.float32)
    assert L.implisolid_raster_coords(rect.ctypes.data_as(fp), W, H, s, mx.ctypes.data_as(fp), my.ctypes.data_as(fp)) == -1
    assert impli.last_error()
    with pytest.raises(impli.ImplisolidError):
        impli.raster_coords(rect, W, H, s)
    # the device entry refuses them too, before anything is compiled or launched: no GPU is needed to see it
    z = np.zeros(2, np.float32)
    sums = np.zeros(2, np.int64)
    assert L.implisolid_raster(json.dumps(EGG).encode(), 0, rect.ctypes.data_as(fp), W, H, s, z.ctypes.data_as(fp), 2, None,
                               sums.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None) == -1
    assert impli.last_error()
    with pytest.raises(impli.ImplisolidError) as e:
        impli.raster_layers(EGG, rect, W, H, z, s)
    assert str(e.value), "with a message"
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,), "and the next call works"


@pytest.mark.parametrize("z", [[], [0.0, np.nan], [np.inf]])
def test_bad_heights_are_refused_before_the_device(impli, z):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.raster_layers(EGG, UNIT, 8, 8, z, 1)
    assert str(e.value)


def test_a_rect_too_narrow_for_float_is_refused(impli):
    # 65536 sub-cells across two ulps: samples cannot stay inside distinct sub-cells' closed intervals in
    # order -- the step underflows the spacing, and the last sub-cell's edge jumps to xmax
    lo = np.float32(1000)
    hi = np.nextafter(np.nextafter(lo, np.float32(2000)), np.float32(2000))
    ex = np_raster.edges(lo, hi, 16384 * 4)
    mx = np_raster.mids(ex)
    inside = bool(((ex[:-1] <= mx) & (mx <= ex[1:])).all())
    if inside:
        assert impli.raster_coords([lo, hi, -1, 1], 16384, 4, 4)[0].shape == (65536,)
    else:
        with pytest.raises(impli.ImplisolidError):
            impli.raster_coords([lo, hi, -1, 1], 16384, 4, 4)


def test_the_restatement_counts_negative_zero_and_nan_as_solid():
    F = np.full((2, 4, 6), -1, np.float32)
    F[0, 0, 0], F[0, 1, 1], F[0, 2, 5], F[1, 3, 2], F[1, 3, 3] = -0.0, np.nan, 0.0, 0.25, -0.0
    assert np.signbit(F[0, 0, 0]) and not np.signbit(F[0, 2, 5])
    cov, sums = np_raster.coverage(F, 2)
    assert cov.dtype == np.uint8 and cov.shape == (2, 2, 3) and sums.dtype == np.int64
    assert cov.tolist() == [[[2, 0, 0], [0, 0, 1]], [[0, 0, 0], [0, 2, 0]]]
    assert sums.tolist() == [3, 2]
    cov1, sums1 = np_raster.coverage(F, 1)
    assert cov1.shape == (2, 4, 6) and sums1.tolist() == [3, 2] and cov1[0, 0, 0] == 1 and cov1[0, 1, 1] == 1 and cov1[0, 2, 5] == 1
    # a whole pixel of NaN and zeros of either sign is fully covered
    G = np.array([[[np.nan, -0.0], [0.0, np.nan]]], np.float32)
    assert np_raster.coverage(G, 2)[0].tolist() == [[[4]]]


# ---- the inputs of test_gpu_raster.py ---------------------------------------------------------------------
def test_the_zero_table_puts_negative_zeros_on_the_raster_samples():
    import np_sdf3d
    import test_gpu_mass as g
    node, zeros = g.zero_node()
    M = np_raster.coords(UNIT, 32, 32, 1)
    M2 = np_raster.coords(UNIT, 16, 16, 2)
    T = np_sdf3d.Table.from_node(node)
    nodes = T.ox + T.gs * np.arange(T.sx, dtype=np.float32)
    for m in (M[0], M[1], M2[0], M2[1]):
        assert np.array_equal(_u32(m), _u32(nodes)), "the samples are the table's nodes"
    z = nodes
    F = np_sdf3d.evaluate(node, *np_raster.points(M[0], M[1], z).T).reshape(32, 32, 32)
    zero = F == 0
    assert np.array_equal(zero, zeros) and zero.sum() >= 100 and np.signbit(F[zero]).all()
    cov, sums = np_raster.coverage(F, 1)
    assert int(sums.sum()) == int((F > 0).sum() + zeros.sum())
