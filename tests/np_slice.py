"""numpy restatement of the slices of a solid -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_slice), independent of the kernels that
compute it: the float32 sample coordinates, the marching-squares cases, the interpolated endpoints,
the segment order (layer, tile of 16 x 16 cells row-major, cell row-major, table order), the layer
offsets, and the chaining of one layer's keys into polylines.  The field values are an argument.
One numpy ufunc call is one IEEE operation.  A sample that is not finite gets no special case: a NaN is solid, and
an endpoint on an edge whose mu is NaN (a or b NaN, or both infinite) or +-0 (a finite beside b infinite) is what
the header's formula gives under IEEE arithmetic.
"""
import numpy as np

f32 = np.float32
T = 16   # cells per tile side: part of the interface

# case -> segments (start edge, end edge); e0 bottom, e1 right, e2 top, e3 left; solid on the left
SEGMENTS = {
    1: [(0, 3)], 2: [(1, 0)], 4: [(2, 1)], 8: [(3, 2)],
    14: [(3, 0)], 13: [(0, 1)], 11: [(1, 2)], 7: [(2, 3)],
    3: [(1, 3)], 12: [(3, 1)], 6: [(2, 0)], 9: [(0, 2)],
    5: [(0, 3), (2, 1)], 10: [(1, 0), (3, 2)],
}


def coords(rect, R):
    """xs, ys: R + 1 float32 each."""
    out = []
    for lo, hi in ((rect[0], rect[1]), (rect[2], rect[3])):
        lo, hi = f32(lo), f32(hi)
        step = f32(f32(hi - lo) / f32(R))
        e = np.empty(R + 1, f32)
        e[:R] = lo + np.arange(R, dtype=f32) * step   # one float32 multiply, one float32 add
        e[R] = hi
        out.append(e)
    return out[0], out[1]


def cases(F):
    """F (R + 1, R + 1) indexed [j][i] -> case per cell (R, R); solid iff not (F < 0)."""
    s = ~(F < 0)
    return (s[:-1, :-1].astype(np.uint32) | s[:-1, 1:].astype(np.uint32) << 1 | s[1:, 1:].astype(np.uint32) << 2 |
            s[1:, :-1].astype(np.uint32) << 3)


def _edge(e, i, j, F, xs, ys, W):
    """the point and key on edge e of cell (i, j)"""
    with np.errstate(all="ignore"):
        if e == 0 or e == 2:                      # an x-edge at (i, jj)
            jj = j + (1 if e == 2 else 0)
            a, b = F[jj, i], F[jj, i + 1]
            mu = f32(f32(0) - a) / f32(b - a)
            x = f32(xs[i] + f32(mu * f32(xs[i + 1] - xs[i])))
            return x, ys[jj], 2 * (jj * W + i)
        ii = i + (1 if e == 1 else 0)             # a y-edge at (ii, j)
        a, b = F[j, ii], F[j + 1, ii]
        mu = f32(f32(0) - a) / f32(b - a)
        y = f32(ys[j] + f32(mu * f32(ys[j + 1] - ys[j])))
        return xs[ii], y, 2 * (j * W + ii) + 1


def march_layer(F, xs, ys):
    """One layer: (segments float32 (S, 2, 2), keys uint32 (S, 2)) in the defined order."""
    F = np.asarray(F, f32)
    R = len(xs) - 1
    assert F.shape == (R + 1, R + 1)
    W = R + 1
    c = cases(F)
    seg, keys = [], []
    nt = (R + T - 1) // T
    for ty in range(nt):
        for tx in range(nt):
            for j in range(T * ty, min(T * ty + T, R)):
                for i in range(T * tx, min(T * tx + T, R)):
                    for (es, ee) in SEGMENTS.get(int(c[j, i]), ()):
                        x0, y0, k0 = _edge(es, i, j, F, xs, ys, W)
                        x1, y1, k1 = _edge(ee, i, j, F, xs, ys, W)
                        seg.append(((x0, y0), (x1, y1)))
                        keys.append((k0, k1))
    return np.array(seg, f32).reshape(-1, 2, 2), np.array(keys, np.uint32).reshape(-1, 2)


def march(F, xs, ys):
    """F (L, R + 1, R + 1) -> (segments, keys, layer_offsets int64 (L + 1,))."""
    F = np.asarray(F, f32)
    segs, keys, offs = [], [], [0]
    for l in range(F.shape[0]):
        s, k = march_layer(F[l], xs, ys)
        segs.append(s)
        keys.append(k)
        offs.append(offs[-1] + len(s))
    return np.concatenate(segs).reshape(-1, 2, 2), np.concatenate(keys).reshape(-1, 2), np.array(offs, np.int64)


def points(xs, ys, z):
    """the sample points (L (R + 1)^2, 3), layer-major, then j, then i"""
    zz, yy, xx = np.meshgrid(np.asarray(z, f32), ys, xs, indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(f32)


def loops(keys):
    """One layer's keys (n, 2) -> (order, loop_offsets, closed), or None if a key starts two segments
    or ends two.  Open chains first (from a start no segment ends on, by first segment), then closed
    loops, each from its lowest-indexed segment."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    n = len(keys)
    start = {}
    ends = set()
    for i in range(n):
        s, e = int(keys[i, 0]), int(keys[i, 1])
        if s in start or e in ends:
            return None
        start[s] = i
        ends.add(e)
    used = np.zeros(n, bool)
    order, offs, closed = [], [0], []
    for want_open in (True, False):
        for i in range(n):
            if used[i] or (want_open and int(keys[i, 0]) in ends):
                continue
            k = i
            while k is not None and not used[k]:
                used[k] = True
                order.append(k)
                k = start.get(int(keys[k, 1]))
            offs.append(len(order))
            closed.append(not want_open)
    return np.array(order, np.int64), np.array(offs, np.int64), np.array(closed, bool)


def shoelace(pts):
    """signed area of the closed polygon pts (n, 2), in float64; positive: counter-clockwise"""
    p = np.asarray(pts, np.float64)
    q = np.roll(p, -1, axis=0)
    return 0.5 * float(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]))
