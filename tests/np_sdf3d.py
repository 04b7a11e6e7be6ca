"""numpy float32 restatement of the "sdf_3d" node -- TEST INFRASTRUCTURE ONLY.

The node samples a caller-supplied SDF table exactly as cube.hpp:176-272 samples the rabbit's
(np_restate.cube, generalised here to any sizes, grid size and origin), with every read at a flat
index >= N returning 0.  Written from the issue's definition, independent of the library: the value,
the analytic in-cell gradient, the set of table entries a box of points can read, and the min / max
pyramid lookup the interval bound is allowed to use.  One numpy ufunc call is one IEEE operation.
"""
import json

import numpy as np

import np_restate
from np_restate import RABBIT, RCONST

f32 = np.float32


class Table:
    """values: flat float32 [N], index x + y sx + z sx sy."""

    def __init__(self, values, sizes, grid_size, origin):
        self.sx, self.sy, self.sz = (int(s) for s in sizes)
        self.N = self.sx * self.sy * self.sz
        self.values = np.ascontiguousarray(values, np.float32).reshape(-1)
        assert self.values.size == self.N
        self.gs = f32(grid_size)
        self.ox, self.oy, self.oz = (f32(o) for o in origin)
        # zero padding: every index a cell index <= size per axis can reach
        reach = (self.sx + self.sy * self.sx + self.sz * self.sx * self.sy) + 1 + self.sx + self.sx * self.sy + 1
        self.padded = np.concatenate([self.values, np.zeros(reach - self.N, np.float32)])

    @classmethod
    def from_node(cls, d):
        return cls(np.array(d["sdf"], np.float64).astype(np.float32), (d["size_x"], d["size_y"], d["size_z"]),
                   f32(d["grid_size"]), (f32(d["origin_x"]), f32(d["origin_y"]), f32(d["origin_z"])))

    def hi(self):
        return (self.ox + self.gs * f32(self.sx), self.oy + self.gs * f32(self.sy), self.oz + self.gs * f32(self.sz))


def rabbit_table():
    return Table(RABBIT, (22, 18, 22), RCONST["GRID_SIZE"], (RCONST["ORIGIN_X"], RCONST["ORIGIN_Y"], RCONST["ORIGIN_Z"]))


def random_table(seed=5):
    rng = np.random.default_rng(seed)
    return Table(rng.uniform(-1, 1, 5 * 4 * 6).astype(np.float32), (5, 4, 6), 0.25, (-0.625, -0.5, -0.75))


def sphere_table():
    """33 x 17 x 9 samples of the distance to a sphere of radius 0.6 (positive outside)."""
    sx, sy, sz, gs, org = 33, 17, 9, 0.0625, (-1.0, -0.5, -0.25)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    d = np.sqrt((org[0] + gs * x) ** 2 + (org[1] + gs * y) ** 2 + (org[2] + gs * z) ** 2) - 0.6
    return Table(d.astype(np.float32).reshape(-1), (sx, sy, sz), gs, org)


def node(T, matrix, id=0):
    """The MP5 node of a Table (what scenes.sdf3d_node builds from the same data)."""
    return {"type": "sdf_3d", "id": id, "matrix": [float(v) for v in matrix], "size_x": T.sx, "size_y": T.sy,
            "size_z": T.sz, "grid_size": float(T.gs), "origin_x": float(T.ox), "origin_y": float(T.oy),
            "origin_z": float(T.oz), "sdf": [float(v) for v in T.values]}


def _cell(T, x, y, z):
    """outside mask and, for the inside points: reads base index, the eight reads, the fractions."""
    xm, ym, zm = T.hi()
    out = (xm < x) | (x < T.ox) | (ym < y) | (y < T.oy) | (zm < z) | (z < T.oz)
    i = ~out
    X, Y, Z = x[i], y[i], z[i]
    gs = T.gs
    xg = ((X - T.ox) / gs).astype(np.int64)
    yg = ((Y - T.oy) / gs).astype(np.int64)
    zg = ((Z - T.oz) / gs).astype(np.int64)
    xl = T.ox + xg.astype(np.float32) * gs
    yl = T.oy + yg.astype(np.float32) * gs
    zl = T.oz + zg.astype(np.float32) * gs
    xd, yd, zd = (X - xl) / gs, (Y - yl) / gs, (Z - zl) / gs
    sx, sxy = T.sx, T.sx * T.sy
    b = xg + yg * sx + zg * sxy
    P = T.padded
    r = (P[b], P[b + 1], P[b + sx], P[b + 1 + sx], P[b + sxy], P[b + 1 + sxy], P[b + sx + sxy], P[b + 1 + sx + sxy])
    return out, i, b, r, (xd, yd, zd)


def _lerps(r, d):
    r000, r100, r010, r110, r001, r101, r011, r111 = r
    xd, yd, zd = d
    one = f32(1)
    c00 = r000 * (one - xd) + r100 * xd
    c01 = r001 * (one - xd) + r101 * xd
    c10 = r010 * (one - xd) + r110 * xd
    c11 = r011 * (one - xd) + r111 * xd
    c0 = c00 * (one - yd) + c10 * yd
    c1 = c01 * (one - yd) + c11 * yd
    return c00, c01, c10, c11, c0, c1


def value(T, x, y, z):
    x, y, z = (np.asarray(v, np.float32) for v in (x, y, z))
    out, i, b, r, d = _cell(T, x, y, z)
    res = np.full(x.shape, f32(10000), np.float32)
    c00, c01, c10, c11, c0, c1 = _lerps(r, d)
    res[i] = c0 * (f32(1) - d[2]) + c1 * d[2]
    return -res


def gradient(T, x, y, z):
    """[n, 3]: the analytic gradient of value() inside the cell, (0, 0, 0) outside the table box."""
    x, y, z = (np.asarray(v, np.float32) for v in (x, y, z))
    out, i, b, r, d = _cell(T, x, y, z)
    r000, r100, r010, r110, r001, r101, r011, r111 = r
    xd, yd, zd = d
    one = f32(1)
    c00, c01, c10, c11, c0, c1 = _lerps(r, d)
    e0 = (r100 - r000) * (one - yd) + (r110 - r010) * yd
    e1 = (r101 - r001) * (one - yd) + (r111 - r011) * yd
    g = np.zeros(x.shape + (3,), np.float32)
    g[i, 0] = -((e0 * (one - zd) + e1 * zd) / T.gs)
    g[i, 1] = -(((c10 - c00) * (one - zd) + (c11 - c01) * zd) / T.gs)
    g[i, 2] = -((c1 - c0) / T.gs)
    return g


def read_indices(T, x, y, z):
    """(inside mask, [n_inside, 8] flat indices the inside points read)."""
    x, y, z = (np.asarray(v, np.float32) for v in (x, y, z))
    out, i, b, r, d = _cell(T, x, y, z)
    sx, sxy = T.sx, T.sx * T.sy
    offs = np.array([0, 1, sx, sx + 1, sxy, sxy + 1, sxy + sx, sxy + sx + 1], np.int64)
    return i, b[:, None] + offs[None, :]


def value_f64(T, x, y, z):
    """The trilinear interpolant in float64 (cell picked as value() picks it): the gradient's check."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    gs, ox, oy, oz = float(T.gs), float(T.ox), float(T.oy), float(T.oz)
    xg, yg, zg = np.floor((x - ox) / gs).astype(np.int64), np.floor((y - oy) / gs).astype(np.int64), np.floor((z - oz) / gs).astype(np.int64)
    xd, yd, zd = (x - ox) / gs - xg, (y - oy) / gs - yg, (z - oz) / gs - zg
    sx, sxy = T.sx, T.sx * T.sy
    b = xg + yg * sx + zg * sxy
    P = T.padded.astype(np.float64)
    c00 = P[b] * (1 - xd) + P[b + 1] * xd
    c10 = P[b + sx] * (1 - xd) + P[b + 1 + sx] * xd
    c01 = P[b + sxy] * (1 - xd) + P[b + 1 + sxy] * xd
    c11 = P[b + sx + sxy] * (1 - xd) + P[b + 1 + sx + sxy] * xd
    return -((c00 * (1 - yd) + c10 * yd) * (1 - zd) + (c01 * (1 - yd) + c11 * yd) * zd)


# ---- the entries a box can read, and the pyramid lookup ---------------------------------------------
def _clamped_cells(T, lo, hi, o, m):
    """cell range of one axis for the part of [lo, hi] inside [o, m] (cube_iv's x0, x1)."""
    a = max(f32(lo), o)
    b = min(f32(hi), m)
    return int((a - o) / T.gs), int((b - o) / T.gs)


def box_cells(T, box):
    """box = (xlo, xhi, ylo, yhi, zlo, zhi) in the node's frame -> ((x0, x1), (y0, y1), (z0, z1)),
    all_in, none_in (float32 comparisons, as the point function's)."""
    b = [f32(v) for v in box]
    xm, ym, zm = T.hi()
    all_in = bool(b[0] >= T.ox and b[1] <= xm and b[2] >= T.oy and b[3] <= ym and b[4] >= T.oz and b[5] <= zm)
    none_in = bool(b[0] > xm or b[1] < T.ox or b[2] > ym or b[3] < T.oy or b[4] > zm or b[5] < T.oz)
    if none_in:
        return None, all_in, none_in
    return (_clamped_cells(T, b[0], b[1], T.ox, xm), _clamped_cells(T, b[2], b[3], T.oy, ym),
            _clamped_cells(T, b[4], b[5], T.oz, zm)), all_in, none_in


def readable_range(T, cells):
    """(min, max) over every table entry a point in the cells x0..x1, y0..y1, z0..z1 reads."""
    (x0, x1), (y0, y1), (z0, z1) = cells
    x, y, z = np.meshgrid(np.arange(x0, x1 + 2), np.arange(y0, y1 + 2), np.arange(z0, z1 + 2), indexing="ij")
    v = T.padded[(x + y * T.sx + z * T.sx * T.sy).ravel()]
    return f32(v.min()), f32(v.max())


def pyramid_range(T, cells):
    """(min, max, L) over the <= 2 x 2 x 2 level-L blocks of the lookup rule: the smallest L with
    (x1 >> L) - (x0 >> L) <= 1 on all three axes; a level-L block X covers the cells
    X << L .. (X << L) + 2^L - 1 (clipped to 0 .. size), each cell its eight reads."""
    L = 0
    while any((c1 >> L) - (c0 >> L) > 1 for c0, c1 in cells):
        L += 1
    size = (T.sx, T.sy, T.sz)
    spans = []
    for (c0, c1), s in zip(cells, size):
        lo = (c0 >> L) << L
        hi = min(((c1 >> L) << L) + (1 << L) - 1, s)
        spans.append((lo, hi))
    mn, mx = readable_range(T, spans)
    return mn, mx, L


def widen(vmin, vmax, all_in):
    """The issue's bound from a value range: widened by s, negated, hulled with -10000 unless all_in."""
    vmin, vmax = f32(vmin), f32(vmax)
    s = (np.abs(vmin) + np.abs(vmax)) * f32(1e-4) + f32(1e-6)
    lo, hi = -(vmax + s), -(vmin - s)
    if not all_in:
        lo, hi = min(lo, f32(-10000)), max(hi, f32(-10000))
    return f32(lo), f32(hi)


# ---- trees ---------------------------------------------------------------------------------------------
def _grad_xform(mi, g):                # inv^T g (transformed_union.hpp:76-83): (m_i gx + m_{4+i} gy) + m_{8+i} gz
    return np.stack([mi[i] * g[:, 0] + mi[4 + i] * g[:, 1] + mi[8 + i] * g[:, 2] for i in range(3)], axis=1)


def evaluate(shape, x, y, z):
    """np_restate.evaluate with sdf_3d leaves."""
    d = json.loads(shape) if isinstance(shape, str) else shape
    t = d["type"]
    mi = np_restate._inverse(d["matrix"])
    X, Y, Z = np_restate._xform(mi, x, y, z)
    if t == "sdf_3d":
        return value(Table.from_node(d), X, Y, Z)
    if t in np_restate.PRIMS:
        return np_restate.PRIMS[t](X, Y, Z)
    ch = d["children"]
    acc = evaluate(ch[0], X, Y, Z)
    for k in range(1, len(ch) if t == "Union" else 2):
        f2 = evaluate(ch[k], X, Y, Z)
        if t == "Union":
            acc = np.where(acc > f2, acc, f2)
        elif t == "Intersection":
            acc = np.where(acc > f2, f2, acc)
        elif t == "Difference":
            acc = np.where(acc < -f2, acc, -f2)
        else:
            raise ValueError(t)
    return acc


def leaf_value_gradient(d, pts):
    """(f [n], grad [n, 3]) of one sdf_3d leaf under its node matrix at world points [n, 3]."""
    p = np.asarray(pts, np.float32)
    mi = np_restate._inverse(d["matrix"])
    X, Y, Z = np_restate._xform(mi, p[:, 0], p[:, 1], p[:, 2])
    T = Table.from_node(d)
    return value(T, X, Y, Z), _grad_xform(mi, gradient(T, X, Y, Z))
