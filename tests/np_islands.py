"""numpy restatement of the islands of the layers -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_islands), independent of the kernels:

  solid      a pixel of layer l is solid iff cov[l][py][px] >= threshold, cov being np_raster.coverage's
  adjacent   two solid pixels of one layer that differ by one step in x or in y (connectivity 4), or by at
             most one step in each (connectivity 8); inside the image only
  component  a class of the transitive closure of adjacency; its seed is its smallest py W + px
  record     {seed, area, below, x0, y0, x1, y1, layer}: the pixel count, the pixels that are solid at the
             same (px, py) in layer l - 1 (all of them for l = 0), the inclusive bounding box
  order      layer by layer in the caller's order, within a layer in increasing seed
  labels     int32 (L, H, W): the pixel's seed, -1 where it is not solid

Components by minimum-label propagation: every solid pixel starts with its own index and takes the
smallest label among itself and its solid neighbours until nothing changes.
"""
import numpy as np

FIELDS = ("seed", "area", "below", "x0", "y0", "x1", "y1", "layer")
STEPS4 = [(0, 1), (0, -1), (1, 0), (-1, 0)]
STEPS8 = STEPS4 + [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def steps(connectivity):
    assert connectivity in (4, 8)
    return STEPS4 if connectivity == 4 else STEPS8


def labels(solid, connectivity):
    """solid bool (L, H, W) -> int32 (L, H, W)"""
    solid = np.asarray(solid, bool)
    L, H, W = solid.shape
    big = H * W
    lab = np.where(solid, np.arange(H * W, dtype=np.int64).reshape(1, H, W), big)
    st = steps(connectivity)
    while True:
        p = np.pad(lab, ((0, 0), (1, 1), (1, 1)), constant_values=big)
        m = lab
        for dy, dx in st:
            m = np.minimum(m, p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        m = np.where(solid, m, big)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(solid, lab, -1).astype(np.int32)


def records(solid, lab):
    """(comp_offsets int64 (L + 1,), comps int32 (C, 8)) of a labelled stack"""
    solid = np.asarray(solid, bool)
    L, H, W = solid.shape
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    offs, rows = [0], []
    for l in range(L):
        held = solid[l] if l == 0 else solid[l] & solid[l - 1]
        for seed in np.unique(lab[l][solid[l]]):
            m = lab[l] == seed
            rows.append([seed, m.sum(), (m & held).sum(), px[m].min(), py[m].min(), px[m].max(), py[m].max(), l])
        offs.append(len(rows))
    return np.array(offs, np.int64), np.array(rows, np.int32).reshape(-1, 8)


def islands(cov, threshold, connectivity):
    """cov uint8 (L, H, W) -> (comp_offsets, comps int32 (C, 8), labels int32 (L, H, W))"""
    solid = np.asarray(cov) >= threshold
    lab = labels(solid, connectivity)
    offs, comps = records(solid, lab)
    return offs, comps, lab


def as_rows(comps):
    """a structured record array (implisolid_amd.COMP_DTYPE) as int32 (C, 8)"""
    comps = np.asarray(comps)
    if comps.dtype.names:
        assert comps.dtype.names == FIELDS
        return np.stack([comps[n] for n in FIELDS], axis=1).astype(np.int32).reshape(-1, 8)
    return comps.astype(np.int32).reshape(-1, 8)
