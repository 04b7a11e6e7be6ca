"""numpy restatement of the support tips under the layer stack -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_supports), with loops over cells and no
cleverness, independent of the kernels:

  solid        a pixel of layer l is solid iff cov[l][py][px] >= threshold
  dist         np_distance.field(solid): the brute-force signed squared distance of every layer
  U_l          for l >= 1 the pixels with dist[l] > 0 and dist[l - 1] < -reach2; U_0 is empty
  cell         c = (py // cell) * ncx + px // cell with ncx = ceil(W / cell)
  tip          per (l, c) with a pixel of U_l in c: the pixel of U_l in c with the largest dist[l], the smallest
               p = py W + px among equals
  record       {p, depth = dist[l][p], foot = the largest m < l with cov[m][p] >= threshold or -1, load = |U_l in c|}
  order        by layer, within a layer by c
  layer record {unsupported = |U_l|, tips}
"""
import numpy as np

import np_distance

FIELDS = ("p", "depth", "foot", "load")
REC_FIELDS = ("unsupported", "tips")
NONE = np_distance.NONE


def unsupported(dist, reach2):
    """dist (L, H, W) -> bool (L, H, W)"""
    dist = np.asarray(dist, np.int64)
    U = np.zeros(dist.shape, bool)
    for l in range(1, len(dist)):
        U[l] = (dist[l] > 0) & (dist[l - 1] < -int(reach2))
    return U


def foot(solid, l, py, px):
    for m in range(l - 1, -1, -1):
        if solid[m, py, px]:
            return m
    return -1


def supports(cov, threshold, reach2, cell, dist=None):
    """cov (L, H, W) -> (tips int64 (T, 4), tip_offsets int64 (L + 1,), records int64 (L, 2), U bool (L, H, W))"""
    solid = np.asarray(cov) >= threshold
    if dist is None:
        dist = np_distance.field(solid)
    dist = np.asarray(dist, np.int64)
    L, H, W = solid.shape
    cell = int(cell)
    ncx, ncy = -(-W // cell), -(-H // cell)
    U = unsupported(dist, reach2)
    tips, offs, recs = [], [0], []
    for l in range(L):
        n = 0
        if U[l].any():
            for cy in range(ncy):
                for cx in range(ncx):
                    best = None
                    load = 0
                    for py in range(cy * cell, min((cy + 1) * cell, H)):
                        for px in range(cx * cell, min((cx + 1) * cell, W)):
                            if U[l, py, px]:
                                load += 1
                                d = int(dist[l, py, px])
                                if best is None or d > best[0]:   # in increasing p: the first of the largest stays
                                    best = (d, py, px)
                    if best is not None:
                        d, py, px = best
                        tips.append((py * W + px, d, foot(solid, l, py, px), load))
                        n += 1
        offs.append(offs[-1] + n)
        recs.append((int(U[l].sum()), n))
    return (np.array(tips, np.int64).reshape(-1, 4), np.array(offs, np.int64), np.array(recs, np.int64).reshape(-1, 2), U)


def as_rows(a, fields=FIELDS):
    """a structured array (implisolid_amd.SUPPORT_DTYPE or SUPPORT_REC_DTYPE) as int64 rows"""
    a = np.asarray(a)
    if a.dtype.names:
        assert a.dtype.names == fields
        return np.stack([a[n] for n in fields], axis=1).astype(np.int64).reshape(-1, len(fields))
    return a.astype(np.int64).reshape(-1, len(fields))
