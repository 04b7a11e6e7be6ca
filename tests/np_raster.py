"""numpy restatement of the layer images of a solid -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_raster, implisolid_raster_coords),
independent of the kernels that compute it:

  inputs    rect {xmin, xmax, ymin, ymax}; W x H pixels; s in {1, 2, 4} sub-samples per axis per pixel;
            the heights z in the caller's order
  edges     ex[k] = xmin + (float)k * ((xmax - xmin) / (float)(W s)) for k < W s, ex[W s] = xmax; ey the
            same with H s
  samples   mx[k] = ex[k] + 0.5f * (ex[k + 1] - ex[k]), my likewise
  coverage  cov[l][py][px] = the number of (a, b) in [0, s)^2 with not (F < 0) at (mx[px s + a],
            my[py s + b], z[l]): -0.0 and NaN are solid; a uint8 in 0 .. s^2; row 0 is the row at ymin
  sums      layer_sum[l] = the sum of cov[l], an int64

The field values are an argument.  One numpy ufunc call is one IEEE operation.
"""
import numpy as np

f32 = np.float32


def edges(lo, hi, n):
    """n + 1 float32 sub-cell edges of one axis"""
    lo, hi = f32(lo), f32(hi)
    step = np.divide(np.subtract(hi, lo, dtype=f32), f32(n), dtype=f32)
    e = np.empty(n + 1, f32)
    off = np.multiply(np.arange(n, dtype=f32), step, dtype=f32)
    e[:n] = np.add(lo, off, dtype=f32)
    e[n] = hi
    return e


def mids(e):
    w = np.subtract(e[1:], e[:-1], dtype=f32)
    half = np.multiply(f32(0.5), w, dtype=f32)
    return np.add(e[:-1], half, dtype=f32)


def coords(rect, W, H, s):
    """(mx float32 (W s,), my float32 (H s,))"""
    return mids(edges(rect[0], rect[1], W * s)), mids(edges(rect[2], rect[3], H * s))


def points(mx, my, z):
    """the sample points (L len(my) len(mx), 3): layer-major, then the y index, then the x index"""
    zz, yy, xx = np.meshgrid(np.asarray(z, f32), my, mx, indexing="ij")
    return np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3), f32)


def coverage(F, s):
    """F (L, H s, W s) indexed [l][y sample][x sample] -> (cov uint8 (L, H, W), layer_sum int64 (L,))"""
    F = np.asarray(F, f32)
    L, Hs, Ws = F.shape
    assert Hs % s == 0 and Ws % s == 0
    solid = ~(F < 0)                      # -0.0 and NaN are solid
    cov = solid.reshape(L, Hs // s, s, Ws // s, s).sum(axis=(2, 4)).astype(np.uint8)
    return cov, cov.reshape(L, -1).sum(axis=1, dtype=np.int64)
